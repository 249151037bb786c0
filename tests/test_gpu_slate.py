"""GPU tests of slate scoring (m2d_score_slate, m2d_topk_slate): the [users x slate] score matrix and the k
best dishes of a slate per user -- bit for bit on exact tables at every width, at the edges of the kernel's tiles with poisoned
output, independent of how a call is cut, against float64 under a derived rounding bound, as lists, through the generic kernel, the
errors and refusals, and after the engine's writers.  Inputs, references, bounds and comparisons: tests/slate_cases.py.

Slowest case: see README.md (status row "slate scoring")."""
import numpy as np
import pytest

import seen_dish_cases as sd
import slate_cases as sc
from helpers import COEFS, assert_scores_close

pytestmark = pytest.mark.gpu

MFMA, GENERIC = "m2d_score_slate_mfma", "m2d_score_slate_generic"
POISON = 0x7FC12345                                          # a NaN no kernel computes


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(PM, RE, CE, cats, coef, user_base=0):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(PM, RE, CE, coef=coef, user_base=user_base)
    if cats is not None:
        eng.set_dish_categories(cats)
    return eng


def _scores(eng, users, slate):
    out = eng.score_slate(_dev(np.asarray(users, np.int32)), _dev(np.asarray(slate, np.int32)))
    eng.check()
    return out.cpu().numpy()


def _lists(eng, users, slate, k):
    s, i = eng.topk_slate(_dev(np.asarray(users, np.int32)), _dev(np.asarray(slate, np.int32)), k)
    eng.check()
    return s.cpu().numpy(), i.cpu().numpy()


def _raw(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _assert_exact(got, ref, what=""):
    """bit-equal to the float64 oracle's value, NaN where it is NaN"""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ" % what
    g, w = sc.bits(np.where(nan, 0, got)), sc.bits(np.where(nan, 0, ref))
    assert np.array_equal(g, w), "%s: %d of %d words differ" % (what, int((g != w).sum()), g.size)


def _assert_lists_are_matrix_words(s, i, matrix, slate, what=""):
    """a listed score is the word score_slate wrote for that (user, dish)"""
    col = np.searchsorted(slate, i)
    assert np.array_equal(np.asarray(slate)[col], i), what
    assert np.array_equal(_raw(s), _raw(np.take_along_axis(matrix, col, 1))), what


# ---- 1. exact tables, every width ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", sc.WIDTHS)
def test_exact_tables_bit_equal_at_every_width(E):
    r = sc.exact_recipe(E)
    eng = _engine(r.PM, r.RE, r.CE, r.cats, r.coef)
    got = _scores(eng, r.users, r.slate)
    assert eng.last_kernel() == MFMA
    _assert_exact(got, r.ref, "E = %d" % E)
    assert np.isnan(got).all(0).sum() == len(sd.LAUNCH_EMPTY)
    for k in (10, 64):
        s, i = _lists(eng, r.users, r.slate, k)
        assert eng.last_kernel() == MFMA
        ws, wi = sc.exact_lists(r.ref, r.slate, k)
        assert np.array_equal(i, wi), "E = %d, k = %d: ids of %d users differ" % (E, k, int((i != wi).any(1).sum()))
        _assert_exact(s, ws, "E = %d, k = %d" % (E, k))
        _assert_lists_are_matrix_words(s, i, got, r.slate, "E = %d, k = %d" % (E, k))
        sc.compare_lists(s, i, r.ref, np.zeros_like(r.ref), r.slate, k, what="E = %d, k = %d" % (E, k))
    # a list that reaches the NaN columns: NaN entries last, in id order
    finite = [int(d) for d in r.slate if d not in sd.LAUNCH_EMPTY][:8]
    s, i = _lists(eng, r.users[:4], finite + list(sd.LAUNCH_EMPTY[2:]), 10)
    assert np.isnan(s[:, 8:]).all() and np.array_equal(i[:, 8:], np.broadcast_to(sd.LAUNCH_EMPTY[2:], (4, 2)))
    eng.close()


# ---- 2. tile edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", (64, 200))
def test_tile_edges_write_every_element_and_nothing_else(E):
    import torch
    r = sd.launch_recipe(E)
    eng = _engine(r.PM, r.RE, r.CE, r.cats, r.coef)
    rng = np.random.default_rng(E)
    slates = [np.sort(rng.choice(r.I, min(nD, r.I), replace=False)) for nD in sc.ND_EDGES]
    slates += [np.asarray([r.I - 1]), np.arange(r.I)]       # the last dish alone, the whole catalogue
    for slate in slates:
        nD = len(slate)
        sl = _dev(slate.astype(np.int32))
        for nU in sc.NU_EDGES:
            users = (rng.permutation(max(nU, r.U))[:nU] % r.U).astype(np.int32)
            buf = torch.full(((nU + 1) * nD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
            out = eng.score_slate(_dev(users), sl, out=buf[:nU * nD].view(nU, nD))
            eng.check()
            assert eng.last_kernel() == MFMA
            whole = buf.cpu().numpy()
            assert (whole.view(np.int32)[nU * nD:] == POISON).all(), "nU = %d, nD = %d: the guard row was written" % (nU, nD)
            got = out.cpu().numpy()
            assert (got.view(np.int32) != POISON).all(), "nU = %d, nD = %d: %d elements not written" % (
                nU, nD, int((got.view(np.int32) == POISON).sum()))
            _assert_exact(got, r.S[users][:, slate], "nU = %d, nD = %d" % (nU, nD))
    eng.close()


# ---- 3. shape independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", (64, 200))
def test_bits_do_not_depend_on_how_a_call_is_cut(E):
    r = sc.normal_recipe(E, U=64, I=500, nD=300)
    eng = _engine(r.PM, r.RE, r.CE, r.cats, 0.5)
    users = np.arange(r.U, dtype=np.int32)
    whole = _scores(eng, users, r.slate)
    assert np.isfinite(whole).mean() > 0.9 and np.unique(_raw(whole)).size > whole.size // 2
    pieces = np.concatenate([_scores(eng, users, r.slate[a:b]) for a, b in ((0, 50), (50, 177), (177, 300))], axis=1)
    assert np.array_equal(_raw(pieces), _raw(whole)), "the slate in three pieces"
    rows = np.concatenate([_scores(eng, users[j:j + 1], r.slate) for j in range(r.U)])
    assert np.array_equal(_raw(rows), _raw(whole)), "the users one by one"
    perm = np.random.default_rng(3).permutation(r.U)
    perm[5] = perm[0]                                        # a user repeated
    assert np.array_equal(_raw(_scores(eng, users[perm], r.slate)), _raw(whole[perm])), "rows permuted, one repeated"
    # a single column, a single user: the small-tile kernel against the large one
    assert np.array_equal(_raw(_scores(eng, users, r.slate[40:41])), _raw(whole[:, 40:41]))
    want = None
    for P in (256, 300 * 3, 1 << 22):
        eng.set_option("slate_chunk_pairs", P)
        assert eng.get_option("slate_chunk_pairs") == P
        s, i = _lists(eng, users, r.slate, 10)
        _assert_lists_are_matrix_words(s, i, whole, r.slate, "chunk %d" % P)
        if want is None:
            want = (s, i)
        assert np.array_equal(i, want[1]) and np.array_equal(_raw(s), _raw(want[0])), "chunk %d" % P
    for bad in (255, (1 << 24) + 1, 0, -1):
        with pytest.raises(ValueError):
            eng.set_option("slate_chunk_pairs", bad)
    assert eng.get_option("slate_chunk_pairs") == 1 << 22
    eng.close()


# ---- 4. normal tables against float64 ----------------------------------------------------------------------------------------------
def _against_float64(r, coef, kernel, pairs=True):
    eng = _engine(r.PM, r.RE, r.CE, r.cats, coef)
    got = _scores(eng, r.users, r.slate)
    assert eng.last_kernel() == kernel
    ref, bound = sc.reference_and_bound(r.PM, r.RE, r.CE, r.cats, coef, r.users, r.slate)
    worst = sc.assert_within(got, ref, bound, "E = %d, C = %d, coef = %g" % (r.E, r.C, coef))
    if pairs:                                                # the project's bar between two of its own paths
        uu, dd = np.repeat(r.users, len(r.slate)), np.tile(r.slate, len(r.users))
        by = eng.score_pairs_bydish(_dev(uu), _dev(dd))
        eng.check()
        assert_scores_close(got.reshape(-1), by.cpu().numpy(), what="score_slate vs score_pairs_bydish, E = %d coef = %g" % (r.E, coef))
    eng.close()
    return worst


@pytest.mark.parametrize("E", sc.WIDTHS)
def test_normal_tables_within_the_derived_bound(E):
    r = sc.normal_recipe(E)
    worst = [_against_float64(r, coef, MFMA) for coef in COEFS]
    print("E = %d: largest err / bound per blend %s" % (E, ["%.3f" % w for w in worst]))


def test_weighted_masks_within_the_derived_bound():
    r = sc.normal_recipe(64, weighted=True)
    assert set(np.unique(r.cats)) == {0.0, 0.5, 1.0, 2.0}
    for coef in COEFS:
        _against_float64(r, coef, MFMA)


# ---- 5. lists on normal tables -----------------------------------------------------------------------------------------------------
def _check_lists(E, nD, k, C, kernel):
    r = sc.list_recipe(E, nD, k, C)
    assert r.sharp.mean() >= sc.MIN_SHARP, "inputs refused: %.2f sharp" % r.sharp.mean()
    eng = _engine(r.PM, r.RE, r.CE, r.cats, r.coef)
    s, i = _lists(eng, r.users, r.slate, k)
    assert eng.last_kernel() == kernel
    sharp = sc.compare_lists(s, i, r.ref, r.bound, r.slate, k, what="E = %d, slate %d, k = %d" % (E, nD, k))
    if nD >= 64:                                             # k = 64 under (a)-(c); exact ids for the (few) users sharp over 65 scores
        s64, i64 = _lists(eng, r.users[:32], r.slate, 64)
        assert np.array_equal(i64[:, :k], i[:32]) and np.array_equal(_raw(s64[:, :k]), _raw(s[:32]))
        sc.compare_lists(s64, i64, r.ref[:32], r.bound[:32], r.slate, 64, what="E = %d, slate %d, k = 64" % (E, nD))
    eng.close()
    return float(sharp.mean())


@pytest.mark.parametrize("E", sc.LIST_WIDTHS)
def test_lists_on_normal_tables(E):
    shares = [_check_lists(E, nD, sc.list_k(E, k), 4, MFMA) for nD, k in sc.LIST_SLATES]
    print("E = %d: sharp users per slate %s" % (E, ["%.2f" % x for x in shares]))


# ---- 6. the generic kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,E", sc.GENERIC_SHAPES)
def test_generic_kernel(C, E):
    r = sc.normal_recipe(E, C=C)
    for coef in (0.5, 0.99):
        _against_float64(r, coef, GENERIC)
    _check_lists(E, 97, sc.list_k(E, 10), C, GENERIC)


def test_variant_9_forces_the_generic_kernel_on_an_mfma_shape():
    r = sc.normal_recipe(64)
    eng = _engine(r.PM, r.RE, r.CE, r.cats, 0.5)
    eng.set_option("variant", 9)
    got = _scores(eng, r.users, r.slate)
    assert eng.last_kernel() == GENERIC
    ref, bound = sc.reference_and_bound(r.PM, r.RE, r.CE, r.cats, 0.5, r.users, r.slate)
    sc.assert_within(got, ref, bound, "variant 9")
    eng.close()


# ---- 7. errors and refusals ----------------------------------------------------------------------------------------------------------
def test_id_errors_are_latched_with_code_and_index_and_the_engine_stays_usable():
    r = sc.exact_recipe(64)
    eng = _engine(r.PM, r.RE, r.CE, r.cats, r.coef)
    users = (np.arange(300) % r.U).astype(np.int32)         # past one block of 128 users

    def good():
        _assert_exact(_scores(eng, users, r.slate), r.S[users][:, r.slate], "after an error")

    for pos in (0, 299):
        for bad_id in (r.U, -1):
            bad = users.copy()
            bad[pos] = bad_id
            for call in (lambda u: eng.score_slate(_dev(u), _dev(r.slate)), lambda u: eng.topk_slate(_dev(u), _dev(r.slate), 10)):
                call(bad)
                with pytest.raises(IndexError, match=r"user id %d at position %d " % (bad_id, pos)):
                    eng.check()
                good()
    eng.set_option("slate_chunk_pairs", 256)                 # user blocks of one row: the position is the caller's, not the block's
    bad = users.copy()
    bad[77] = r.U + 5
    eng.topk_slate(_dev(bad), _dev(r.slate), 10)
    with pytest.raises(IndexError, match=r"user id %d at position 77 " % (r.U + 5)):
        eng.check()
    eng.set_option("slate_chunk_pairs", 1 << 22)
    n = len(r.slate)
    for pos, bad_id in ((n - 1, r.I), (0, -1), (n // 2, r.I + 7)):
        sl = r.slate.copy()
        sl[pos] = bad_id
        eng.score_slate(_dev(users), _dev(sl))
        with pytest.raises(IndexError, match=r"item id %d at position %d " % (bad_id, pos)):
            eng.check()
        good()
    for pos, what in ((150, "two equal neighbours"), (n - 1, "a descending pair at the last position")):
        sl = r.slate.copy()
        sl[pos] = sl[pos - 1] if pos == 150 else sl[pos - 1] - 1
        eng.topk_slate(_dev(users), _dev(sl), 10)
        with pytest.raises(ValueError, match=r"not ascending: value %d at position %d " % (sl[pos], pos)):
            eng.check()
        good()
    eng.close()


def test_argument_errors():
    import ctypes
    import torch
    from foodrec_amd import _native
    r = sc.exact_recipe(64)
    eng = _engine(r.PM, r.RE, r.CE, r.cats, r.coef)
    u, sl = _dev(r.users), _dev(r.slate)
    lib = _native.lib()
    out = torch.empty((len(r.users), len(r.slate)), dtype=torch.float32, device="cuda")
    oi = torch.empty((len(r.users), 64), dtype=torch.int32, device="cuda")
    nU, nD = len(r.users), len(r.slate)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    INV = _native.M2D_ERR_INVALID_ARG
    assert lib.m2d_score_slate(eng._h, P(u), nU, P(sl), 0, P(out), None) == INV
    assert lib.m2d_score_slate(eng._h, P(u), nU, P(sl), r.I + 1, P(out), None) == INV
    assert lib.m2d_score_slate(eng._h, P(u), -1, P(sl), nD, P(out), None) == INV
    for args in ((None, nU, P(sl), nD, P(out)), (P(u), nU, None, nD, P(out)), (P(u), nU, P(sl), nD, None)):
        assert lib.m2d_score_slate(eng._h, *args, None) == INV
    assert lib.m2d_score_slate(eng._h, None, 0, None, nD, None, None) == 0          # nU == 0: nothing is launched
    for k in (0, -1, 65):
        assert lib.m2d_topk_slate(eng._h, P(u), nU, P(sl), nD, k, P(out), P(oi), None) == INV
    assert lib.m2d_topk_slate(eng._h, P(u), nU, P(sl), 5, 6, P(out), P(oi), None) == INV   # k > nD
    assert lib.m2d_topk_slate(eng._h, P(u), nU, P(sl), nD, 10, P(out), None, None) == INV
    assert lib.m2d_topk_slate(eng._h, P(u), nU, P(sl), nD, 10, None, P(oi), None) == INV
    assert lib.m2d_topk_slate(eng._h, None, 0, None, nD, 10, None, None, None) == 0
    with pytest.raises(ValueError):
        eng.topk_slate(u, sl[:5], 6)
    with pytest.raises(TypeError):
        eng.score_slate(u.to(torch.int64), sl)
    with pytest.raises(TypeError):
        eng.topk_slate(u, sl.cpu(), 3)
    with pytest.raises(ValueError):
        eng.score_slate(u, sl, out=out[:, :5])
    assert eng.score_slate(u[:0], sl).shape == (0, nD)
    s, i = eng.topk_slate(u[:0], sl, 3)
    assert s.shape == i.shape == (0, 3)
    ts = torch.ops.m2d.score_slate(eng.id, u, sl)
    tk = torch.ops.m2d.topk_slate(eng.id, u, sl, 10)
    eng.check()
    _assert_exact(ts.cpu().numpy(), r.ref, "torch op")
    assert np.array_equal(tk[1].cpu().numpy(), sc.exact_lists(r.ref, r.slate, 10)[1])
    eng.close()
    no_masks = _engine(r.PM, r.RE, r.CE, None, r.coef)
    with pytest.raises(ValueError, match="m2d_set_dish_categories"):
        no_masks.score_slate(u, sl)
    with pytest.raises(ValueError, match="m2d_set_dish_categories"):
        no_masks.topk_slate(u, sl, 3)
    no_masks.close()


def test_refusals_name_their_condition_and_end_with_it():
    import torch
    from helpers import mlp_head
    r = sc.exact_recipe(64)
    u, sl = _dev(r.users), _dev(r.slate)
    eng = _engine(r.PM, r.RE, r.CE, r.cats, r.coef)
    rng = np.random.default_rng(1)

    def served():
        _assert_exact(_scores(eng, r.users, r.slate), r.ref, "served again")
        assert np.array_equal(_lists(eng, r.users, r.slate, 10)[1], sc.exact_lists(r.ref, r.slate, 10)[1])

    def refused(match):
        for call in (lambda: eng.score_slate(u, sl), lambda: eng.topk_slate(u, sl, 10)):
            with pytest.raises(ValueError, match=match):
                call()

    served()
    off = np.arange(r.I + 1, dtype=np.int32)
    eng.set_ingredients((rng.integers(-4, 5, (7, 64)) / 4).astype(np.float32), off, rng.integers(0, 7, r.I).astype(np.int32))
    refused("m2d_(score|topk)_slate: the ingredient table is set")
    eng.clear_ingredients()
    served()
    eng.set_mlp_head(*mlp_head(320, 256, 64, rng))
    refused("m2d_(score|topk)_slate: the MLP head is set")
    eng.clear_mlp_head()
    served()
    keep = eng.pm[3, 1, 7].item()
    eng.pm[3, 1, 7] = float("inf")
    eng.tables_updated()
    refused("m2d_(score|topk)_slate: needs finite tables \\(a table value is not finite\\)")
    eng.pm[3, 1, 7] = keep
    eng.tables_updated()
    served()
    eng.close()
    assert torch.cuda.is_available()


def test_user_base_and_the_model_calls():
    import types
    import torch
    import foodrec_amd
    r = sc.exact_recipe(64)
    base = 7000
    eng = _engine(r.PM, r.RE, r.CE, r.cats, r.coef, user_base=base)
    _assert_exact(_scores(eng, r.users + base, r.slate), r.ref, "user_base")
    assert np.array_equal(_lists(eng, r.users + base, r.slate, 10)[1], sc.exact_lists(r.ref, r.slate, 10)[1])
    eng.score_slate(_dev(r.users), _dev(r.slate))            # local ids on a shard: out of range
    with pytest.raises(IndexError, match="user id"):
        eng.check()
    eng.close()
    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    dishes = [str(d) for d in (17, 3, 599, 17, 250, 3, 5)]  # str ids, the caller's order, repeats, two empty masks
    users = [str(x) for x in (4, 0, 31, 4)]
    got = model.score_slate(users, dishes)
    assert got.shape == (4, 7)
    _assert_exact(got, r.S[[4, 0, 31, 4]][:, [17, 3, 599, 17, 250, 3, 5]], "Model.score_slate")
    among = [599, 17, 3, 250, 5, 17, 400, 401, 402]
    s, i = model.topk([4, 0, 31], 5, among=among)
    slate = np.unique(among)
    ws, wi = sc.exact_lists(r.S[[4, 0, 31]][:, slate], slate, 5)
    assert np.array_equal(i, wi)
    _assert_exact(s, ws, "Model.topk(among)")
    for kw in ({"exclude": [[1], [2], [3]]}, {"head": True}, {"head": True, "candidates": 8}):
        with pytest.raises(ValueError, match="among"):
            model.topk([4, 0, 31], 5, among=among, **kw)


# ---- 8. after writers ------------------------------------------------------------------------------------------------------------------
def test_slate_vectors_follow_the_engines_writers():
    """score_slate after write_memory and after a train_step equals a fresh engine built from the written tables, bit for bit, and
    differs from before: the slate vectors are rebuilt, not served stale."""
    import torch
    r = sc.normal_recipe(64, U=64, I=500, nD=300)
    eng = _engine(r.PM.copy(), r.RE.copy(), r.CE.copy(), r.cats, 0.5)
    users = np.arange(r.U, dtype=np.int32)
    rng = np.random.default_rng(5)
    t = lambda a: torch.as_tensor(a, device="cuda")

    def snapshot(e):
        m = _scores(e, users, r.slate)
        return m, _lists(e, users, r.slate, 10)

    def fresh():
        f = _engine(eng.pm.cpu().numpy(), eng.re.cpu().numpy(), eng.ce.cpu().numpy(), r.cats, 0.5)
        out = snapshot(f)
        f.close()
        return out

    def changed(a, b, what):
        fin = np.isfinite(a[0])
        assert (a[0][fin] != b[0][fin]).mean() > 0.5, what

    def same(a, b, what):
        assert np.array_equal(_raw(a[0]), _raw(b[0])) and np.array_equal(a[1][1], b[1][1]) and np.array_equal(_raw(a[1][0]), _raw(b[1][0])), what

    before = snapshot(eng)
    B, L = 600, 7
    wu = (np.arange(B) % r.U).astype(np.int32)
    masked = np.flatnonzero(r.cats.sum(1) > 0)              # (a pair with an empty mask writes 0 / 0 into the tables)
    wi = rng.choice(masked, B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, r.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(r.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    after_write = snapshot(eng)
    changed(before, after_write, "write_memory changed nothing")
    same(after_write, fresh(), "after write_memory")
    eng.train_begin("sgd", 200.0)
    tu = (rng.permutation(256) % r.U).astype(np.int32)
    ti = rng.choice(masked, 256).astype(np.int32)
    eng.train_step(t(tu), t(ti), t(r.cats[ti]), t(rng.integers(0, 2, 256).astype(np.float32))); eng.check()
    after_step = snapshot(eng)
    changed(after_write, after_step, "train_step changed nothing")
    same(after_step, fresh(), "after train_step")
    eng.train_end()
    eng.close()
