"""GPU parity of m2d_write_memory (scatter-add form of Model.Write_Memory, Model_Recommender.py:106-220)
with the op-for-op restatement that keeps the reference's dense one-hot matmuls."""
import functools

import numpy as np
import pytest

from helpers import containment_case, random_case, write_case

pytestmark = pytest.mark.gpu


def _close(got, ref, tol=2e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.all(np.abs(got[ok] - ref[ok]) <= tol * np.maximum(1.0, np.abs(ref[ok]))), np.abs(got[ok] - ref[ok]).max()


@pytest.mark.parametrize("U,I,C,E,L,B", [(50, 30, 4, 64, 95, 128), (20, 10, 4, 200, 7, 8), (9, 5, 3, 6, 4, 33), (300, 100, 4, 32, 95, 1000),
                                         (40, 30, 4, 64, 95, 3000),       # > 2048 pairs: the General_Memory assign by atomics
                                         (20, 10, 4, 32, 130, 2500),      # three label masks
                                         (20, 10, 4, 32, 300, 64)])       # more labels than the masks hold: every label walked
def test_write_memory_matches_restatement(U, I, C, E, L, B):
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    PM, RE, CE, users, items, cats = random_case(U, I, C, E, B, seed=U + B, zero_rows=False)
    rng = np.random.default_rng(L)
    GM = (rng.standard_normal((L, C + 1, E)) / 4).astype(np.float32)
    sign = np.where(rng.random(B) < 0.6, 1.0, -1.0).astype(np.float32)
    y = (rng.random((B, L)) < 0.1).astype(np.float32)
    y[y.sum(1) == 0, 0] = 1
    users[:4] = users[0]                                   # duplicate users accumulate (reduce_sum over the batch)
    eng = ScoringEngine(PM, RE, CE)
    gm = torch.as_tensor(GM, device="cuda").clone()
    means = eng.write_memory(torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda"),
                             torch.as_tensor(cats, device="cuda"), torch.as_tensor(sign, device="cuda"),
                             torch.as_tensor(y, device="cuda"), gm, 0.01, 0.02, 0.03, want_means=True)
    PM2, GM2, mp, mg = oracle.write_memory(PM, RE, CE, GM, users, items, cats, sign, y, 0.01, 0.02, 0.03)
    _close(eng.pm.cpu().numpy(), PM2)
    _close(gm.cpu().numpy(), GM2)
    assert abs(means[0] - mp) < 1e-6 and abs(means[1] - mg) < 1e-6
    # the forward now scores with the written memory
    out = eng.score_pairs(torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda"),
                          torch.as_tensor(cats, device="cuda")); eng.check()
    _close(out.cpu().numpy(), oracle.inference_f64(PM2, RE, CE, users, items, cats), 1e-4)


def test_write_memory_edge_cases():
    """0/0 cases.  The reference's DENSE one-hot matmuls multiply a NaN row by the zeros of every other
    user / label, so one pair with an empty mask turns the whole Personal_Memory (row 0) into NaN there.
    The scatter form touches only the rows the pair addresses: NaN lands in that user's block and in that
    pair's labels, nowhere else.  That containment is a deliberate, documented difference."""
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, L, B = 12, 8, 4, 64, 5, 6
    PM, RE, CE, _, items, cats = random_case(U, I, C, E, B, seed=3, zero_rows=False)
    users = np.arange(B, dtype=np.int32)                   # distinct users
    GM = np.random.default_rng(1).standard_normal((L, C + 1, E)).astype(np.float32)
    y = np.eye(L, dtype=np.float32)[np.arange(B) % L]
    sign = np.ones(B, np.float32)
    cats[2] = 0                                            # empty mask: v row 0 = 0/0
    y[3] = 0                                               # user with no label: g = 0/0
    eng = ScoringEngine(PM, RE, CE)
    gm = torch.as_tensor(GM, device="cuda").clone()
    t = lambda a: torch.as_tensor(a, device="cuda")
    eng.write_memory(t(users), t(items), t(cats), t(sign), t(y), gm, 0.01, 0.01, 0.01); eng.check()
    pm2, gm2 = eng.pm.cpu().numpy(), gm.cpu().numpy()
    assert np.isnan(pm2[2, 0]).all() and not np.isnan(pm2[2, 1:]).any()        # only row 0 of user 2
    assert np.isnan(pm2[3]).all()                                              # user 3: label mean is 0/0
    clean = [u for u in range(U) if u not in (2, 3)]
    assert not np.isnan(pm2[clean]).any()
    assert np.isnan(gm2[2 % L, 0]).all() and not np.isnan(gm2[[l for l in range(L) if l != 2 % L]]).any()
    # on the pairs without 0/0 the numbers are the reference's
    keep = np.array([0, 1, 4, 5])
    PMr, GMr, _, _ = oracle.write_memory(PM, RE, CE, GM, users[keep], items[keep], cats[keep], sign[keep], y[keep])
    _close(pm2[[0, 1, 4, 5]], PMr[[0, 1, 4, 5]])
    bad = users.copy(); bad[1] = U
    with pytest.raises(IndexError):
        eng.write_memory(t(bad), t(items), t(cats), t(sign), t(y), gm, 0.01, 0.01, 0.01); eng.check()
    eng.write_memory(t(users[:0]), t(items[:0]), t(cats[:0]), t(sign[:0]), t(y[:0]), gm, 0.01, 0.01, 0.01); eng.check()


@pytest.mark.parametrize("personal,general", [(True, False), (False, True)])
def test_write_memory_runs_only_the_fetched_assigns(personal, general):
    """`personal` depends on the two Personal_Memory assigns only (Model_Recommender.py:167, :198), `general` on the
    General_Memory assign only (:215); the driver's ordinary batch fetches `general` alone
    (Train_recommender.py:195-199) and must leave Personal_Memory bit for bit as it was."""
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, L, B = 40, 20, 4, 64, 9, 50
    PM, RE, CE, users, items, cats = random_case(U, I, C, E, B, seed=77, zero_rows=False)
    rng = np.random.default_rng(5)
    GM = (rng.standard_normal((L, C + 1, E)) / 4).astype(np.float32)
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 1] = 1
    eng = ScoringEngine(PM, RE, CE)
    gm = torch.as_tensor(GM, device="cuda").clone()
    t = lambda a: torch.as_tensor(a, device="cuda")
    means = eng.write_memory(t(users), t(items), t(cats), t(sign), t(y), gm, 0.01, 0.02, 0.03, want_means=True,
                             write_pm=personal, write_gm=general)
    PM2, GM2, mp, mg = oracle.write_memory(PM, RE, CE, GM, users, items, cats, sign, y, 0.01, 0.02, 0.03,
                                           personal=personal, general=general)
    if personal:
        _close(eng.pm.cpu().numpy(), PM2)
        assert np.array_equal(gm.cpu().numpy(), GM) and means[1] is None and abs(means[0] - mp) < 1e-6
    else:
        _close(gm.cpu().numpy(), GM2)
        assert np.array_equal(eng.pm.cpu().numpy(), PM) and means[0] is None and abs(means[1] - mg) < 1e-6
    # a general-only call still refuses a bad id (the gathers are shared by both branches)
    bad = items.copy(); bad[3] = I
    with pytest.raises(IndexError):
        eng.write_memory(t(users), t(bad), t(cats), t(sign), t(y), gm, 0.01, 0.02, 0.03, write_pm=personal, write_gm=general)
        eng.check()
    with pytest.raises(ValueError):
        eng.write_memory(t(users), t(items), t(cats), t(sign), t(y), gm, 0.01, 0.02, 0.03, write_pm=False, write_gm=False)


# ---- the launches and edges of m2d_write.hip, against the scatter restatement (oracle.write_memory_scatter) ----------------
# Which General_Memory form a call takes: B <= 2048 -> m2d_write_gm_gather<false> (both fetches) / <true> (`general` alone);
# B > 2048 -> m2d_write_memory_kernel<1> (both) / <2> (`general` alone).  Personal_Memory is always m2d_write_memory_kernel<0>.

BETAS = (0.01, 0.02, 0.03)
FETCHES = [pytest.param(True, True, id="both"), pytest.param(False, True, id="general")]


def _match(got, ref):
    """_close, and the same infinities at the same positions."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "infinities differ"
    _close(np.where(inf, 0.0, got), np.where(inf, 0.0, ref))


def _write(eng, GM, users, items, cats, sign, y, personal=True, general=True, betas=BETAS, check=True):
    """One write_memory call on a fresh copy of GM -> (Personal_Memory, General_Memory) on the host."""
    import torch
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    gm = t(GM).clone()
    eng.write_memory(t(users), t(items), t(cats), t(sign), t(y), gm, *betas, write_pm=personal, write_gm=general)
    if check:
        eng.check()
    return eng.pm.cpu().numpy(), gm.cpu().numpy()


def _scatter(args, personal, general, betas=BETAS, dtype=np.float64):
    from oracle import m2d_oracle as oracle
    return oracle.write_memory_scatter(*args, *betas, dtype=dtype, personal=personal, general=general)[:2]


def _head(args, n):
    return args[:4] + tuple(a[:n] for a in args[4:])


@functools.lru_cache(maxsize=None)
def _switch_case():
    return write_case(40, 30, 4, 32, 9, 2049, seed=31)


@pytest.mark.parametrize("personal,general", FETCHES)
def test_write_memory_every_general_memory_form_on_the_same_pairs(personal, general):
    """The first 2 048 pairs of one batch take the owner-computes gather, all 2 049 the atomics: with the two fetches that is
    gather<false>, gather<true>, kernel<1> and kernel<2> on the same data.  Each is the scatter restatement, and the two sizes
    differ by the restatement of the one extra pair."""
    from foodrec_amd import ScoringEngine
    args = _switch_case()
    PM, RE, CE, GM = args[:4]
    got = {}
    for B in (2048, 2049):
        eng = ScoringEngine(PM, RE, CE)
        pm, gm = got[B] = _write(eng, GM, *_head(args, B)[4:], personal=personal, general=general)
        PMr, GMr = _scatter(_head(args, B), personal, general)
        _match(pm, PMr)
        _match(gm, GMr)
        if not personal:
            assert np.array_equal(pm, PM)                          # bit for bit
    one = args[:4] + tuple(a[2048:] for a in args[4:])
    dPM, dGM = _scatter((np.zeros_like(PM), RE, CE, GM) + one[4:], personal, general)
    _close(got[2049][0], got[2048][0].astype(np.float64) + (dPM if personal else 0.0))
    _close(got[2049][1], got[2048][1].astype(np.float64) + (dGM - GM))
    assert np.abs(dGM - GM).max() > 1e-3                           # the extra pair is visible at the tolerance


@pytest.mark.parametrize("personal,general", FETCHES)
def test_write_memory_grid_stride_second_pair_per_wave(personal, general):
    """The grid is capped at 8 * num_cu blocks of four waves: with 32 * num_cu + 37 pairs, 37 waves take a second pair."""
    from foodrec_amd import ScoringEngine
    probe = ScoringEngine(np.zeros((1, 5, 16), np.float32), np.zeros((1, 16), np.float32), np.zeros((4, 16), np.float32))
    B = 32 * probe.get_option("num_cu") + 37
    args = write_case(20, 10, 4, 16, 5, B, seed=41)
    eng = ScoringEngine(*args[:3])
    pm, gm = _write(eng, *args[3:], personal=personal, general=general)
    PMr, GMr = _scatter(args, personal, general)
    _match(pm, PMr)
    _match(gm, GMr)


@pytest.mark.parametrize("B", [128, 2100])
@pytest.mark.parametrize("personal,general", FETCHES)
def test_write_memory_fractional_label_and_mask_weights(personal, general, B):
    """The placeholders are float: labels in {0, 0.5, 1, 2}, each pair's mask scaled by uniform(0.5, 2)."""
    from foodrec_amd import ScoringEngine
    args = write_case(40, 30, 4, 32, 9, B, seed=51, weighted=True)
    assert set(np.unique(args[8])) == {0.0, 0.5, 1.0, 2.0}
    eng = ScoringEngine(*args[:3])
    pm, gm = _write(eng, *args[3:], personal=personal, general=general)
    PMr, GMr = _scatter(args, personal, general)
    _match(pm, PMr)
    _match(gm, GMr)
    assert np.abs(GMr - args[3]).max() > 1e-3


@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 129, 256, 257])
@pytest.mark.parametrize("personal,general", FETCHES)
def test_write_memory_label_mask_edges(personal, general, L):
    """The first and last bit of each of the four 64-label lane masks, and L = 257 where the masks give way to the walk over
    every label.  Pair 0 has every label, pair 1 only the last one."""
    from foodrec_amd import ScoringEngine
    B = 70
    PM, RE, CE, GM, users, items, cats, sign, y = write_case(20, 10, 4, 32, L, B, seed=60 + L)
    edges = sorted({i for i in (0, 63, 64, 127, 128, 255, 256) if i < L} | {L - 1})
    y[:] = 0
    for b in range(B):
        y[b, edges[b % len(edges)]] = 1.0
        y[b, edges[(b // len(edges)) % len(edges)]] = 0.5 if b % 3 else 1.0
    y[0] = 1.0
    y[1] = 0; y[1, L - 1] = 1.0
    assert all((y[:, i] != 0).sum() >= 2 for i in edges)
    args = (PM, RE, CE, GM, users, items, cats, sign, y)
    eng = ScoringEngine(PM, RE, CE)
    pm, gm = _write(eng, *args[3:], personal=personal, general=general)
    PMr, GMr = _scatter(args, personal, general)
    _match(pm, PMr)
    _match(gm, GMr)
    assert (np.abs(gm - GM).reshape(L, -1).max(1) > 0).all()              # pair 0 reached every label


@pytest.mark.parametrize("B", [128, 2100])
@pytest.mark.parametrize("personal,general", FETCHES)
def test_write_memory_with_a_user_base(personal, general, B):
    """Rows are addressed as uid - user_base: a shard that starts at user 5 000."""
    import torch
    from foodrec_amd import ScoringEngine
    U, base = 40, 5000
    args = write_case(U, 30, 4, 32, 9, B, seed=71)
    PM, RE, CE, GM, users, items, cats, sign, y = args
    eng = ScoringEngine(PM, RE, CE, user_base=base)
    pm, gm = _write(eng, GM, users + base, items, cats, sign, y, personal=personal, general=general)
    PMr, GMr = _scatter(args, personal, general)
    _match(pm, PMr)
    _match(gm, GMr)
    for bad_id, pos in ((base - 1, 3), (base + U, B - 2)):
        bad = users + base
        bad[pos] = bad_id
        with pytest.raises(IndexError, match=r"user id %d at position %d " % (bad_id, pos)):
            _write(eng, GM, bad, items, cats, sign, y, personal=personal, general=general)
    _write(eng, GM, users + base, items, cats, sign, y, personal=personal, general=general)     # the latch is clear again


@pytest.mark.parametrize("what", ["item", "user"])
def test_write_memory_general_only_bad_id_above_2048(what):
    """m2d_write_memory_kernel<2> latches id errors itself: nothing is written for the bad pair, everything for the others,
    Personal_Memory stays as it was, and the next call is clean."""
    from foodrec_amd import ScoringEngine
    U, I, B, pos = 40, 30, 2100, 2077
    args = write_case(U, I, 4, 32, 9, B, seed=81)
    PM, RE, CE, GM, users, items, cats, sign, y = args
    bad_u, bad_i = users.copy(), items.copy()
    if what == "item":
        bad_i[pos] = I
    else:
        bad_u[pos] = U
    eng = ScoringEngine(PM, RE, CE)
    pm, gm = _write(eng, GM, bad_u, bad_i, cats, sign, y, personal=False, general=True, check=False)
    with pytest.raises(IndexError, match=r"%s id %d at position %d " % (what, I if what == "item" else U, pos)):
        eng.check()
    without = args[:4] + tuple(np.delete(a, pos, axis=0) for a in args[4:])
    _match(gm, _scatter(without, False, True)[1])
    assert np.array_equal(pm, PM) and np.array_equal(eng.pm.cpu().numpy(), PM)
    pm, gm = _write(eng, *args[3:], personal=False, general=True)           # check() inside: no error left over
    _match(gm, _scatter(args, False, True)[1])
    assert np.array_equal(pm, PM)


HOT_BETAS = (0.01, 0.02, 0.005)


@functools.lru_cache(maxsize=None)
def _hot_case():
    """3 000 pairs, one user, one label.  The atomic order is free, so the INPUTS have to make the float32 sum insensitive to
    it: the float32 restatement in two permuted pair orders stays within a quarter of _close's bound of the float64 one and of
    each other (measured: 0.16).  That takes more than a small alpha.  With 0/1 masks half the pairs add the SAME value
    alpha * g into the row of a category they lack, the rounding errors of equal addends do not cancel, and 3 000 of them
    put the float32 restatement itself 1.3 to 2.2 bounds from the float64 one at every alpha from 1e-5 to 5e-3 (0.1 at
    alpha = 0).  So every pair here has its own weight in (0.5, 2) for every category: no two addends are equal."""
    B = 3000
    PM, RE, CE, GM, users, items, cats, sign, y = write_case(40, 30, 4, 32, 9, B, seed=91)
    cats = np.random.default_rng(93).uniform(0.5, 2.0, cats.shape).astype(np.float32)
    users[:] = 17
    y[:] = 0; y[:, 6] = 1.0
    args = (PM, RE, CE, GM, users, items, cats, sign, y)
    ref = _scatter(args, True, True, HOT_BETAS)
    rng = np.random.default_rng(92)
    runs = []
    for _ in range(2):
        o = rng.permutation(B)
        runs.append(_scatter(args[:4] + tuple(a[o] for a in args[4:]), True, True, HOT_BETAS, dtype=np.float32))
    frac = lambda got, want, T: float((np.abs(np.asarray(got, np.float64) - want) / (2e-5 * np.maximum(1.0, np.abs(T)))).max())
    worst = max([frac(r[t], ref[t], ref[t]) for r in runs for t in (0, 1)] + [frac(runs[0][t], runs[1][t], ref[t]) for t in (0, 1)])
    return args, ref, worst


@pytest.mark.parametrize("personal,general", FETCHES)
def test_write_memory_hot_rows(personal, general):
    """Every pair adds into the same Personal_Memory block and the same General_Memory block: the worst case for the atomics."""
    from foodrec_amd import ScoringEngine
    args, (PMr, GMr), worst = _hot_case()
    print("float32 order sensitivity: %.3f of the bound" % worst)
    assert worst <= 0.25
    assert np.abs(PMr[17]).max() > 1.0 and len(np.unique(args[7])) == 2
    eng = ScoringEngine(*args[:3])
    pm, gm = _write(eng, *args[3:], personal=personal, general=general, betas=HOT_BETAS)
    if personal:
        _match(pm, PMr)
    else:
        assert np.array_equal(pm, args[0])
    _match(gm, GMr)


@pytest.mark.parametrize("bad,zero", [(np.inf, 0.0), (np.nan, 0.0), (np.inf, -0.0), (0.25, -0.0)],
                         ids=["inf", "nan", "inf-negzero", "finite-negzero"])
@pytest.mark.parametrize("B", [128, 2100])
@pytest.mark.parametrize("personal,general", FETCHES)
def test_write_memory_non_finite_dish_row_at_a_zero_weight_category(personal, general, B, bad, zero):
    """One pair, both sides of the gather / atomics switch: Recipe_Embedding[5, 3] is inf (NaN) and the pair that writes dish 5
    has mask [1, 0, 1, 0].  Model_Recommender.py:111 multiplies the dish row by every weight, so rows 2 and 4 of the pair's user
    and label receive 0 * inf = NaN in EVERY form -- the same pair must not give another table because more pairs share its
    batch.  A weight of -0.0 is a zero: NaN beside an inf, and nothing added to a finite row.
    (Before the atomics passes consulted the engine's non-finite word, B = 2 100 left General_Memory rows (4, 2) and (4, 4)
    finite.)"""
    import torch
    from foodrec_amd import ScoringEngine
    U, I, C = 40, 30, 4
    args = containment_case(U, I, C, 32, 9, B, seed=8, bad=bad, zero=zero)
    PM, RE, CE, GM = args[:4]
    eng = ScoringEngine(PM, RE, CE)
    pm, gm = _write(eng, *args[3:], personal=personal, general=general)
    PMr, GMr = _scatter(args, personal, general)
    for T, row in ((GMr, 4),) + (((PMr, U - 1),) if personal else ()):
        want = np.zeros(T.shape, bool)
        if not np.isfinite(bad):
            want[row, 1:, 3] = True
            assert np.isnan(T[row, 2, 3]) and np.isnan(T[row, 4, 3])
        assert np.array_equal(~np.isfinite(T), want)               # the expected value itself: contained
    _match(gm, GMr)
    _match(pm, PMr)
    if not personal:
        assert np.array_equal(pm, PM)
    if np.isfinite(bad):                                           # -0.0 x finite: the rows are what they were without the pair
        rest = args[:4] + tuple(np.delete(a, 7, axis=0) for a in args[4:])
        _close(gm[4, [2, 4]], _scatter(rest, False, True)[1][4, [2, 4]])
    elif personal:
        # Personal_Memory now holds inf / NaN: retrieval takes the literal kernel
        dish_cats = (np.random.default_rng(3).integers(1, 16, I)[:, None] >> np.arange(C)[None, :] & 1).astype(np.float32)
        eng.set_dish_categories(dish_cats)
        eng.topk_users(torch.arange(U, dtype=torch.int32, device="cuda"), 5); eng.check()
        assert eng.last_kernel() == "m2d_topk_literal"
