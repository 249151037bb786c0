"""GPU parity of the build-defined 3-layer scoring head (m2d_set_mlp_head / m2d_score_pairs_mlp) against
the build's own float64 restatement.  The reference has no MLP: this pins only
the documented extension and its reduction to the reference score when the head contributes nothing."""
import numpy as np
import pytest

import functools

from helpers import COEFS, TOL, assert_mlp_scores, assert_scores_close, mlp_case, mlp_head, random_case

pytestmark = pytest.mark.gpu

_head = mlp_head


_MLP_SHAPES = [(128, 4, 256, 64, "m2d_mlp_mfma"), (64, 4, 256, 64, "m2d_mlp_mfma"), (256, 4, 256, 64, "m2d_mlp_mfma"),
               (32, 5, 256, 64, "m2d_mlp_mfma"),
               # K = (C + 1) E not a multiple of 64 (200 is the reference's default embed_size): zero-padded chunks
               (200, 4, 256, 64, "padded"), (100, 4, 256, 64, "padded"), (40, 4, 256, 64, "padded"), (240, 4, 256, 64, "padded"),
               (36, 3, 256, 64, "padded"),
               (64, 4, 128, 32, "m2d_mlp_generic"), (6, 3, 10, 7, "m2d_mlp_generic"), (30, 4, 256, 64, "m2d_mlp_generic")]
# split-bf16 MFMA: producer / consumer kernel (default), every-wave-gathers kernel; exact-f32 MFMA.  The padded form
# exists for the every-wave-gathers kernel only (either arithmetic), the generic kernel has one form.
_MLP_FORMS = {"m2d_mlp_mfma": [(1, 0), (1, 1), (0, 0)], "padded": [(1, 0), (0, 0)], "m2d_mlp_generic": [(1, 0)]}
_MLP_CASES = [shape + form for shape in _MLP_SHAPES for form in _MLP_FORMS[shape[4]]]


@pytest.mark.parametrize("E,C,H1,H2,kernel,x3,form", _MLP_CASES)
def test_mlp_scores_match_restatement(E, C, H1, H2, kernel, x3, form):
    """One test per (shape, arithmetic, kernel form); the batch sizes -- 1, around one and two tiles of 128 pairs, 3000 -- are
    looped inside (8 cases each, the blend coefficient varying with them)."""
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I = 300, 200
    for B in (1, 127, 128, 129, 255, 256, 257, 3000):
        PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=E + B)
        rng = np.random.default_rng(E + H1)
        dish_cats = rng.integers(0, 2, (I, C)).astype(np.float32)
        dish_cats[dish_cats.sum(1) == 0, 0] = 1
        dish_cats[3] = 0                                      # NaN dish
        K = (C + 1) * E
        head = _head(K, H1, H2, rng, scale=4.0)              # large enough that the head matters
        coef = ([0.99] + COEFS)[(E // 2 + B) % 6]            # the blend coefficient enters the head through z = PM[u] * Dt[d]
        eng = ScoringEngine(PM, RE, CE, coef=coef)
        ut, it = torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda")
        with pytest.raises(ValueError):
            eng.score_pairs_mlp(ut, it)
        eng.set_dish_categories(dish_cats)
        eng.set_mlp_head(*head)
        eng.set_option("mlp_bf16x3", x3)
        eng.set_option("mlp_form", form)
        got = eng.score_pairs_mlp(ut, it); eng.check()
        if kernel == "padded":
            want = "m2d_mlp_mfma_bf16x3" if x3 else "m2d_mlp_mfma"
        else:
            want = kernel if kernel == "m2d_mlp_generic" or not x3 else ("m2d_mlp_mfma_bf16x3" if form else "m2d_mlp_pc_bf16x3")
        assert eng.last_kernel() == want
        ref = oracle.inference_mlp(PM, RE, CE, dish_cats, *head, users, items, coef=coef)
        base = oracle.inference_f64(PM, RE, CE, users, items, dish_cats[items], coef)
        ok = ~np.isnan(ref)
        if ok.sum() > 10:
            assert np.abs(ref[ok] - base[ok]).mean() > 1e-2, "head too small to be tested"
        assert_scores_close(got.cpu().numpy(), ref, what="E%d B%d" % (E, B))
        eng.close()


@pytest.mark.parametrize("E", [64, 128])
def test_mlp_large_table_instantiation_gives_the_same_bits(E):
    """m2d_mlp_pc<KCH, OFF32>: tables under 4 GiB take 32-bit byte offsets and scalar-base row loads, larger ones (up to 64 GiB)
    offsets in units of 16 B -- the same loads, the same arithmetic.  "variant" = 16 runs the second form on small tables: the same
    scores bit for bit, a bad id reported alike."""
    import torch
    from foodrec_amd import ScoringEngine
    U, I, C, B = 3000, 500, 4, 40000
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=E + 5)
    rng = np.random.default_rng(E)
    dish_cats = rng.integers(0, 2, (I, C)).astype(np.float32)
    dish_cats[dish_cats.sum(1) == 0, 1] = 1
    eng = ScoringEngine(PM, RE, CE)
    eng.set_dish_categories(dish_cats)
    eng.set_mlp_head(*_head((C + 1) * E, 256, 64, rng, scale=3.0))
    ut, it = torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda")
    a = eng.score_pairs_mlp(ut, it); eng.check()
    assert eng.last_kernel() == "m2d_mlp_pc_bf16x3"
    eng.set_option("variant", 16)
    b = eng.score_pairs_mlp(ut, it); eng.check()
    assert eng.last_kernel() == "m2d_mlp_pc_bf16x3"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    bad = users.copy(); bad[123] = U + 7
    with pytest.raises(IndexError, match="user id %d at position 123" % (U + 7)):
        eng.score_pairs_mlp(torch.as_tensor(bad, device="cuda"), it); eng.check()
    eng.set_option("variant", 0)


@pytest.mark.parametrize("coef", [0.99] + COEFS)
def test_mlp_reduces_to_reference_and_reports_bad_ids(coef):
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, B = 200, 100, 4, 128, 2000
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=1)
    dish_cats = np.random.default_rng(3).integers(0, 2, (I, C)).astype(np.float32)
    dish_cats[dish_cats.sum(1) == 0, 2] = 1
    rng = np.random.default_rng(2)
    W1, b1, W2, b2, w3, b3 = _head((C + 1) * E, 256, 64, rng)
    eng = ScoringEngine(PM, RE, CE, coef=coef); eng.set_dish_categories(dish_cats)
    eng.set_mlp_head(W1, b1, W2, b2, np.zeros_like(w3), 0.0)          # head contributes exactly 0
    ut, it = torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda")
    got = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
    assert_scores_close(got, oracle.inference_f64(PM, RE, CE, users, items, dish_cats[items], coef), 1e-5, "zero head")
    assert_scores_close(got, eng.score_pairs_bydish(ut, it).cpu().numpy(), 1e-5, "vs reference kernel")
    bad = users.copy(); bad[77] = U
    with pytest.raises(IndexError, match="user id %d at position 77" % U):
        eng.score_pairs_mlp(torch.as_tensor(bad, device="cuda"), it); eng.check()
    eng.clear_mlp_head()
    with pytest.raises(ValueError):
        eng.score_pairs_mlp(ut, it)


def test_mlp_with_ingredient_table():
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, R, B = 100, 80, 4, 64, 50, 1000
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=9)
    rng = np.random.default_rng(5)
    dish_cats = np.ones((I, C), np.float32)
    ING = (rng.standard_normal((R, E)) / 8).astype(np.float32)
    lens = rng.integers(1, 12, I); off = np.zeros(I + 1, np.int32); off[1:] = np.cumsum(lens)
    ids = rng.integers(0, R, off[-1]).astype(np.int32)
    head = _head((C + 1) * E, 256, 64, rng, scale=3.0)
    eng = ScoringEngine(PM, RE, CE); eng.set_dish_categories(dish_cats)
    eng.set_ingredients(ING, off, ids); eng.set_mlp_head(*head)
    got = eng.score_pairs_mlp(torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda")); eng.check()
    H = oracle.dish_high_vectors(ING, off, ids)
    assert_scores_close(got.cpu().numpy(), oracle.inference_mlp(PM, RE, CE, dish_cats, *head, users, items, dish_high=H))


@pytest.mark.parametrize("E,B", [(128, 300_001), (64, 200_000), (32, 150_017)])
def test_mlp_many_tiles_per_block(E, B):
    """Batches of several tiles per workgroup: the producer / consumer kernel's steady state (row requests, ring stages
    and z sets that cross tile boundaries, the id conversion two tiles ahead) -- the small cases above run one tile per
    workgroup.  Every score against the every-wave-gathers kernel (an independent implementation), a sample against the
    float64 restatement, and an out-of-range id deep in the batch."""
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    C = 4 if E != 32 else 5
    U, I = 5000, 3000
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=E)
    rng = np.random.default_rng(E + 7)
    dish_cats = rng.integers(0, 2, (I, C)).astype(np.float32)
    dish_cats[dish_cats.sum(1) == 0, 1] = 1
    dish_cats[::5] *= rng.uniform(0.25, 3.0, (len(dish_cats[::5]), C)).astype(np.float32)     # weighted masks: the pattern is "weight != 0"
    dish_cats[11] = 0                                                                          # a dish without categories: NaN, its own bucket
    head = _head((C + 1) * E, 256, 64, rng, scale=4.0)
    coef = {128: 0.99, 64: 0.5, 32: 1.25}[E]
    eng = ScoringEngine(PM, RE, CE, coef=coef); eng.set_dish_categories(dish_cats); eng.set_mlp_head(*head)
    ut, it = torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda")
    got = eng.score_pairs_mlp(ut, it); eng.check()
    assert eng.last_kernel() == "m2d_mlp_pc_bf16x3"
    # the same kernel without the grouping by mask pattern (every k-block of every tile): the skipped terms are zeros
    eng.set_option("skip_masked", 0)
    plain = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
    eng.set_option("skip_masked", 1)
    gg = got.cpu().numpy()
    assert np.array_equal(np.isnan(gg), np.isnan(plain)) and np.isnan(gg).sum() == (items == 11).sum()
    assert np.nanmax(np.abs(gg - plain) / np.maximum(1.0, np.abs(plain))) < 2e-6
    eng.set_option("mlp_form", 1)
    other = eng.score_pairs_mlp(ut, it); eng.check()
    assert eng.last_kernel() == "m2d_mlp_mfma_bf16x3"
    eng.set_option("mlp_form", 0)
    g, o = got.cpu().numpy(), other.cpu().numpy()
    ok = items != 11
    assert np.isfinite(g[ok]).all() and np.isnan(o[~ok]).all()
    assert np.max(np.abs(g[ok] - o[ok]) / np.maximum(1.0, np.abs(o[ok]))) < 5e-5      # two split-bf16 kernels, different summation orders
    pick = np.concatenate([np.arange(0, 300), rng.integers(0, B, 3000), np.arange(B - 300, B)])
    ref = oracle.inference_mlp(PM, RE, CE, dish_cats, *head, users[pick], items[pick], coef=coef)
    assert_scores_close(g[pick], ref, what="E%d sample" % E)                # NaN rows (dish 11) must agree too
    bad = items.copy(); pos = B - 12_345; bad[pos] = I + 3
    with pytest.raises(IndexError, match="item id %d at position %d" % (I + 3, pos)):
        out = eng.score_pairs_mlp(ut, torch.as_tensor(bad, device="cuda")); eng.check()


# ---- every launch of m2d_mlp.hip past its first loop iteration, the low-level blocks visible ---------------------------------
# From here on every comparison with the oracle is helpers.assert_mlp_scores: the 1e-4 bound AND the condition on the inputs
# that a lost 32-value period of any block moves 80 % of the pairs it touches by more than 10 bounds (blend 0.5; the tests
# above keep the blends they had, where the low-level blocks carry weight 0.01 and the bound cannot see them).
PC_SHAPES = [(32, 5), (64, 2), (64, 4), (128, 4), (256, 4)]           # every (E, C) with an m2d_mlp_pc instantiation: kch 3, 3, 5, 10, 20
NAN_DISH = 11                                                         # a dish without categories: NaN, the all-blocks bucket
MLP_COEF = 0.5


def _patterns(cats):
    return ((np.asarray(cats) != 0) << np.arange(cats.shape[1])).sum(axis=1)


@functools.lru_cache(maxsize=None)
def _pattern_model(E, C, U=5000, I=3000):
    """Tables, masks and head of the pattern-built batches.  random_case's tables TIMES TWO: a batch of the all-categories
    pattern alone misses the visibility condition at (256, 4) on random_case's scale, each low-level block entering with
    weight 0.5 / 4 (tests/test_mlp_checks_cpu.py::test_doubled_tables_make_the_all_categories_pattern_visible).  Dish d has the
    mask pattern 1 + d % (2^C - 1), so every non-empty pattern has I / (2^C - 1) dishes; one dish has no category, and the
    first all-categories dish after it has weights that are not 0 / 1 (the pattern is "weight != 0")."""
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=E + C)
    PM, RE, CE = PM * np.float32(2), RE * np.float32(2), CE * np.float32(2)
    npat = 2 ** C - 1
    pat = 1 + np.arange(I) % npat
    cats = ((pat[:, None] >> np.arange(C)[None, :]) & 1).astype(np.float32)
    cats[NAN_DISH] = 0
    weighted = int(np.flatnonzero((pat == npat) & (np.arange(I) > NAN_DISH))[0])
    cats[weighted] = np.array([0.5, 2.0, 0.25, 3.0, 1.5], np.float32)[:C]
    head = mlp_head((C + 1) * E, 256, 64, np.random.default_rng(E + 7), scale=4.0)
    return PM, RE, CE, cats, head, weighted


def _pattern_engine(E, C):
    from foodrec_amd import ScoringEngine
    PM, RE, CE, cats, head, _ = _pattern_model(E, C)
    eng = ScoringEngine(PM, RE, CE, coef=MLP_COEF)
    eng.set_dish_categories(cats)
    eng.set_mlp_head(*head)
    return eng


def _pattern_batch(E, C, counts, seed, nan_pairs=0, weighted_pairs=0):
    """A shuffled batch with counts[q] pairs of mask pattern q; `nan_pairs` of the all-categories count go to the dish without
    categories (m2d_mlp_pg_scatter puts them into that bucket), `weighted_pairs` to the weighted dish.  Returns the case
    (with .pat, the pattern per pair, 0 for the dish without categories)."""
    PM, RE, CE, cats, head, weighted = _pattern_model(E, C)
    U, I, npat = PM.shape[0], RE.shape[0], 2 ** C - 1
    rng = np.random.default_rng(seed)
    dish_pat = _patterns(cats)
    items, pats = [], []
    for q, n in sorted(counts.items()):
        dishes = np.flatnonzero(dish_pat == q)
        it = dishes[rng.integers(0, len(dishes), n)]
        if q == npat:
            it[:nan_pairs] = NAN_DISH
            it[nan_pairs:nan_pairs + weighted_pairs] = weighted
        items.append(it)
        pats.append(np.where(it == NAN_DISH, 0, q))
    order = rng.permutation(sum(counts.values()))
    items = np.concatenate(items)[order].astype(np.int32)
    users = rng.integers(0, U, len(items)).astype(np.int32)
    case = mlp_case(PM, RE, CE, cats, head, users, items, MLP_COEF)
    case.pat = np.concatenate(pats)[order]
    return case


def _pattern_pick(case, seed, per_pattern=256, ends=300, at_least=8192):
    """At least 256 pairs of every pattern present (all of a smaller bucket), the first and last 300 positions, every pair of
    the dish without categories, random positions up to 8 192."""
    rng = np.random.default_rng(seed)
    B = len(case.items)
    parts = [np.arange(min(ends, B)), np.arange(max(0, B - ends), B), np.flatnonzero(case.pat == 0)]
    for q in np.unique(case.pat[case.pat > 0]):
        pos = np.flatnonzero(case.pat == q)
        parts.append(pos if len(pos) <= per_pattern else rng.choice(pos, per_pattern, replace=False))
    pick = np.unique(np.concatenate(parts))
    if len(pick) < at_least:
        pick = np.unique(np.concatenate([pick, rng.choice(B, min(B, 2 * at_least), replace=False)]))
    assert len(pick) >= min(at_least, B)
    return pick


@functools.lru_cache(maxsize=None)
def _tile_batches(E, C, num_cu):
    """The three batches of test_mlp_pc_every_instantiation_many_tiles, 15 tiles of 128 pairs per workgroup each."""
    npat, tiles = 2 ** C - 1, 15 * num_cu
    rng = np.random.default_rng(E * 31 + C)
    B = tiles * 128 + 1
    out = {}
    if E != 32:            # (E = 32: a block is one period, the launch never groups -- the pattern of a pair changes nothing)
        one = {1 << c: B // C + (1 if c < B % C else 0) for c in range(C)}
        out["one_category"] = _pattern_batch(E, C, one, seed=E + 1)
    out["all_categories"] = _pattern_batch(E, C, {npat: B}, seed=E + 2)
    # every pattern, bucket sizes r 128 + 1 (every bucket ends in a tile of one pair), the r summing to 15 num_cu: B is then
    # 15 . 128 . num_cu + (2^C - 1), the nearest a batch of such buckets comes to the other two
    r = 1 + rng.multinomial(tiles - npat, np.full(npat, 1.0 / npat))
    every = {q + 1: int(r[q]) * 128 + 1 for q in range(npat)}
    out["every_pattern"] = _pattern_batch(E, C, every, seed=E + 3, nan_pairs=37, weighted_pairs=50)
    assert sum(every.values()) == B - 1 + npat and (out["every_pattern"].pat == 0).sum() == 37
    for name, case in out.items():
        case.pick = _pattern_pick(case, seed=len(name))
    return out


_PC_BITS = {}       # (E, C, batch) -> the scores of "variant" 0, which the "variant" 16 case must reproduce bit for bit


def _assert_same_as_other_form(got, other, what):
    """Two split-bf16 kernels with different summation orders: test_mlp_many_tiles_per_block's bound, NaN at the same pairs."""
    assert np.array_equal(np.isnan(got), np.isnan(other)), what
    ok = ~np.isnan(other)
    err = np.abs(got[ok] - other[ok]) / np.maximum(1.0, np.abs(other[ok]))
    assert err.max() < 5e-5, "%s: %.3e at %d" % (what, err.max(), np.flatnonzero(ok)[err.argmax()])


def _assert_bad_ids_reported(eng, users, items, U, I, pos_user, pos_item):
    import torch
    t = lambda a: torch.as_tensor(a, device="cuda")
    bad = items.copy(); bad[pos_item] = I + 3
    with pytest.raises(IndexError, match="item id %d at position %d " % (I + 3, pos_item)):
        eng.score_pairs_mlp(t(users), t(bad)); eng.check()
    bad = users.copy(); bad[pos_user] = U + 7
    with pytest.raises(IndexError, match="user id %d at position %d " % (U + 7, pos_user)):
        eng.score_pairs_mlp(t(bad), t(items)); eng.check()


@pytest.mark.parametrize("variant", [0, 16])
@pytest.mark.parametrize("E,C", PC_SHAPES)
def test_mlp_pc_every_instantiation_many_tiles(E, C, variant):
    """m2d_mlp_pc<KCH, OFF32> for every KCH the launcher reaches and both offset forms ("variant" 16: the large-table one), 15
    tiles per workgroup -- the 7 ring phases times the 2 tile parities -- in three batches built by mask pattern:

      one_category    every tile has two blocks.  The ring phase advances by 2 (nper + 2) mod 7 per tile: 0 for an E = 256 tile
                      with all five blocks (nper = 40), so only shorter tiles move it -- here nper = 16, advance 1, all seven.
      all_categories  the longest tile, every block of every pair non-zero.
      every_pattern   all 2^C - 1 patterns in buckets of r 128 + 1 pairs, the dish without categories, the weighted dish.
                      (E = 32 runs it ungrouped, as it runs everything; one_category is left out there.)

    Per batch: every score against the every-wave-gathers kernel (mlp_form = 1, an independent implementation) at 5e-5; the
    pick of _pattern_pick against the float64 restatement under assert_mlp_scores; "variant" 16 bit-equal to "variant" 0; an
    item id and a user id out of range deep in the batch reported by id and position."""
    import torch
    eng = _pattern_engine(E, C)
    U, I = eng.U, eng.I
    for name, case in _tile_batches(E, C, eng.get_option("num_cu")).items():
        what = "E%d C%d %s variant %d" % (E, C, name, variant)
        ut, it = torch.as_tensor(case.users, device="cuda"), torch.as_tensor(case.items, device="cuda")

        def run(v):
            eng.set_option("variant", v)
            res = eng.score_pairs_mlp(ut, it); eng.check()
            assert eng.last_kernel() == "m2d_mlp_pc_bf16x3"
            return res.cpu().numpy()

        got = run(variant)
        if variant == 0:
            _PC_BITS[(E, C, name)] = got
        else:
            base = _PC_BITS.pop((E, C, name), None)
            base = run(0) if base is None else base              # (this case run on its own)
            eng.set_option("variant", variant)
            assert np.array_equal(got.view(np.int32), base.view(np.int32)), what
        eng.set_option("mlp_form", 1)
        other = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
        assert eng.last_kernel() == "m2d_mlp_mfma_bf16x3"
        eng.set_option("mlp_form", 0)
        assert np.isnan(got).sum() == (case.pat == 0).sum()
        _assert_same_as_other_form(got, other, what)
        assert_mlp_scores(got, case, case.pick, what=what)
        assert_mlp_scores(other, case, case.pick, what=what + " (every-wave-gathers)")       # m2d_mlp_mfma<KCH, true>, 7.5 tiles of 256 per workgroup
        if variant == 0 and name == "every_pattern":                                          # ... and <KCH, false>, the exact-f32 form
            eng.set_option("mlp_bf16x3", 0)
            exact = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
            assert eng.last_kernel() == "m2d_mlp_mfma"
            eng.set_option("mlp_bf16x3", 1)
            assert_mlp_scores(exact, case, case.pick, what=what + " (exact f32)")
        B = len(case.items)
        _assert_bad_ids_reported(eng, case.users, case.items, U, I, B // 2 + 777, B - 12_345)
    eng.close()


def test_mlp_pg_scatter_grid_stride_loop():
    """m2d_mlp_pg_scatter takes chunks of 4 096 pairs on a grid of at most 8 num_cu blocks (m2d_mlp_pg_hist: 256 pairs a block
    on the same grid): one pair more than a whole second round of chunks.  (64, 2), the cheapest K; every pattern present."""
    import torch
    E, C = 64, 2
    eng = _pattern_engine(E, C)
    B = 8 * eng.get_option("num_cu") * 4096 + 4097
    case = _pattern_batch(E, C, {1: B // 2, 2: B // 3, 3: B - B // 2 - B // 3}, seed=5, nan_pairs=37, weighted_pairs=50)
    ut, it = torch.as_tensor(case.users, device="cuda"), torch.as_tensor(case.items, device="cuda")
    got = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
    assert eng.last_kernel() == "m2d_mlp_pc_bf16x3"
    eng.set_option("mlp_form", 1)
    other = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
    assert eng.last_kernel() == "m2d_mlp_mfma_bf16x3"
    _assert_same_as_other_form(got, other, "scatter loop")
    assert np.isnan(got).sum() == 37
    assert_mlp_scores(got, case, _pattern_pick(case, seed=1), what="scatter loop")
    eng.close()


def _small_model(E, C, H1, H2, U=300, I=200, seed=0):
    """Tables (random_case's times two, as _pattern_model's), masks of every non-empty pattern, one dish without categories, a head."""
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=E + seed)
    PM, RE, CE = PM * np.float32(2), RE * np.float32(2), CE * np.float32(2)
    rng = np.random.default_rng(E + H1 + seed)
    cats = ((rng.integers(1, 2 ** C, I)[:, None] >> np.arange(C)[None, :]) & 1).astype(np.float32)
    cats[NAN_DISH] = 0
    return PM, RE, CE, cats, mlp_head((C + 1) * E, H1, H2, rng, scale=4.0)


def _small_case(model, B, seed, users=None):
    PM, RE, CE, cats, head = model
    rng = np.random.default_rng(seed)
    users = rng.integers(0, PM.shape[0], B).astype(np.int32) if users is None else users
    return mlp_case(PM, RE, CE, cats, head, users, rng.integers(0, RE.shape[0], B).astype(np.int32), MLP_COEF)


def _engine_of(model, PM=None, user_base=0):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(model[0] if PM is None else PM, model[1], model[2], coef=MLP_COEF, user_base=user_base)
    eng.set_dish_categories(model[3])
    eng.set_mlp_head(*model[4])
    return eng


def _score(eng, case, kernel=None):
    import torch
    got = eng.score_pairs_mlp(torch.as_tensor(case.users, device="cuda"), torch.as_tensor(case.items, device="cuda")); eng.check()
    if kernel is not None:
        assert eng.last_kernel() == kernel, eng.last_kernel()
    return got.cpu().numpy()


def test_mlp_generic_grid_stride_loop():
    """m2d_mlp_generic: one wave per pair on a grid of at most 4 num_cu blocks of four waves -- five pairs into the second round."""
    model = _small_model(6, 3, 10, 7)
    eng = _engine_of(model)
    case = _small_case(model, 16 * eng.get_option("num_cu") + 5, seed=1)
    assert_mlp_scores(_score(eng, case, "m2d_mlp_generic"), case, what="generic loop")
    eng.close()


@pytest.mark.parametrize("E", [64, 128])
def test_mlp_grouping_threshold(E):
    """Batches of 16 384 pairs and more are bucketed by mask pattern (three more launches, tiles of one pattern), smaller ones
    run as they come: both sides of the threshold, with and without skip_masked, every pair against the oracle."""
    model = _small_model(E, 4, 256, 64, U=2000, I=700)
    eng = _engine_of(model)
    for B in (16383, 16384):
        case = _small_case(model, B, seed=B)
        for skip in (1, 0):
            eng.set_option("skip_masked", skip)
            assert_mlp_scores(_score(eng, case, "m2d_mlp_pc_bf16x3"), case, what="E%d B%d skip_masked %d" % (E, B, skip))
    eng.close()


def test_mlp_launch_sequence_on_one_engine():
    """The grouping scratch (mlp_pg: histogram, tile words, slot -> pair table; grown, never shrunk) and the head's three W1
    images over launches of different sizes on ONE engine: 20 000 -> 300 000 -> 16 384 -> 40 000 pairs with other items each
    time, an every-wave-gathers call and an exact-f32 call in between (the split-bf16 and plain W1 images), then a second head
    (every image rebuilt) on the first launch's pairs."""
    E, C = 64, 4
    model = _small_model(E, C, 256, 64, U=5000, I=3000)
    eng = _engine_of(model)
    first = first_got = None
    for step, B in enumerate((20_000, 300_000, 16_384, 40_000)):
        case = _small_case(model, B, seed=100 + step)
        pick = None if B <= 40_000 else np.unique(np.concatenate([np.arange(300), np.arange(B - 300, B),
                                                                  np.random.default_rng(step).integers(0, B, 16_384)]))
        got = _score(eng, case, "m2d_mlp_pc_bf16x3")
        assert_mlp_scores(got, case, pick, what="launch %d of %d pairs" % (step, B))
        if step == 0:
            first, first_got = case, got
            eng.set_option("mlp_form", 1)
            small = _small_case(model, 3000, seed=200)
            assert_mlp_scores(_score(eng, small, "m2d_mlp_mfma_bf16x3"), small, what="every-wave-gathers in between")
            eng.set_option("mlp_form", 0)
        if step == 1:
            eng.set_option("mlp_bf16x3", 0)
            small = _small_case(model, 3000, seed=201)
            assert_mlp_scores(_score(eng, small, "m2d_mlp_mfma"), small, what="exact f32 in between")
            eng.set_option("mlp_bf16x3", 1)
    head2 = mlp_head((C + 1) * E, 256, 64, np.random.default_rng(77), scale=4.0)
    eng.set_mlp_head(*head2)
    again = mlp_case(*model[:4], head2, first.users, first.items, MLP_COEF)
    got2 = _score(eng, again, "m2d_mlp_pc_bf16x3")
    assert_mlp_scores(got2, again, what="second head")
    ok = ~np.isnan(got2)
    moved = np.abs(got2[ok] - first_got[ok]) > 10 * TOL * np.maximum(1.0, np.abs(first_got[ok]))
    assert moved.mean() >= 0.9, moved.mean()
    eng.close()


def _ingredient_model():
    from oracle import m2d_oracle as oracle
    U, I, C, E, R = 100, 80, 4, 64, 50
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=9)
    rng = np.random.default_rng(5)
    cats = ((rng.integers(1, 2 ** C, I)[:, None] >> np.arange(C)[None, :]) & 1).astype(np.float32)
    ING = (rng.standard_normal((R, E)) / 8).astype(np.float32)
    lens = rng.integers(1, 12, I); off = np.zeros(I + 1, np.int32); off[1:] = np.cumsum(lens)
    ids = rng.integers(0, R, off[-1]).astype(np.int32)
    head = mlp_head((C + 1) * E, 256, 64, rng, scale=3.0)
    return (PM, RE, CE, cats, head), (ING, off, ids), oracle.dish_high_vectors(ING, off, ids)


def test_mlp_with_ingredient_table_even_blend():
    """test_mlp_with_ingredient_table at blend 0.5 and with mixed mask patterns, 20 000 pairs (grouped by pattern): block 0 of the
    dish vector is the ingredient table's, the visibility condition is asked of the low-level blocks."""
    model, ing, H = _ingredient_model()
    eng = _engine_of(model)
    eng.set_ingredients(*ing)
    for B in (1000, 20_000):
        case = _small_case(model, B, seed=B)
        case.dish_high = H
        assert_mlp_scores(_score(eng, case, "m2d_mlp_pc_bf16x3"), case, what="ingredient table, %d pairs" % B)
    eng.close()


@pytest.mark.parametrize("E", [40, 100, 200, 240])
def test_mlp_padded_second_tile(E):
    """m2d_mlp_mfma<5 / 10 / 16 / 20, *, PADK = true> (K = 5 E no multiple of 64): tiles of 256 pairs on a grid of at most num_cu
    blocks -- 300 pairs into the second round of tiles, both arithmetics."""
    model = _small_model(E, 4, 256, 64, U=2000, I=700)
    eng = _engine_of(model)
    B = 256 * eng.get_option("num_cu") + 300
    case = _small_case(model, B, seed=E)
    pick = np.unique(np.concatenate([np.arange(300), np.arange(B - 600, B), np.random.default_rng(E).integers(0, B, 8192)]))
    for x3, kernel in ((1, "m2d_mlp_mfma_bf16x3"), (0, "m2d_mlp_mfma")):
        eng.set_option("mlp_bf16x3", x3)
        assert_mlp_scores(_score(eng, case, kernel), case, pick, what="E%d padded, bf16x3 %d" % (E, x3))
    eng.close()


# (name, E, C, H1, H2, B, options, kernel)
_SHARD_FORMS = [("pc_grouped", 64, 4, 256, 64, 20_000, {}, "m2d_mlp_pc_bf16x3"),
                ("pc", 64, 4, 256, 64, 3000, {}, "m2d_mlp_pc_bf16x3"),
                ("every_wave_gathers", 64, 4, 256, 64, 3000, {"mlp_form": 1}, "m2d_mlp_mfma_bf16x3"),
                ("exact_f32", 64, 4, 256, 64, 3000, {"mlp_bf16x3": 0}, "m2d_mlp_mfma"),
                ("padded", 200, 4, 256, 64, 3000, {}, "m2d_mlp_mfma_bf16x3"),
                ("generic", 6, 3, 10, 7, 3000, {}, "m2d_mlp_generic")]


@pytest.mark.parametrize("name,E,C,H1,H2,B,options,kernel", _SHARD_FORMS, ids=[f[0] for f in _SHARD_FORMS])
def test_mlp_user_base(name, E, C, H1, H2, B, options, kernel):
    """ul = uid - user_base in m2d_mlp_pc, m2d_mlp_mfma and m2d_mlp_generic: an engine over rows 1000 .. 2199 of a 3 000-user table
    with user_base = 1000 gives the whole table's engine's scores bit for bit, the restatement's under assert_mlp_scores, and
    reports the ids just outside its range -- 999 and 2200 -- as the GLOBAL ids they were given as."""
    import torch
    lo, hi = 1000, 2200
    model = _small_model(E, C, H1, H2, U=3000, I=500)
    case = _small_case(model, B, seed=3, users=np.random.default_rng(4).integers(lo, hi, B).astype(np.int32))
    case.users[:2] = (lo, hi - 1)                                  # the shard's first and last row
    full, shard = _engine_of(model), _engine_of(model, PM=model[0][lo:hi], user_base=lo)
    for eng in (full, shard):
        for k, v in options.items():
            eng.set_option(k, v)
    a, b = _score(full, case, kernel), _score(shard, case, kernel)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert_mlp_scores(b, case, what="shard " + name)
    t = lambda x: torch.as_tensor(x, device="cuda")
    for uid, pos in ((lo - 1, B // 2 + 1), (hi, B - 7)):
        bad = case.users.copy(); bad[pos] = uid
        with pytest.raises(IndexError, match="user id %d at position %d " % (uid, pos)):
            shard.score_pairs_mlp(t(bad), t(case.items)); shard.check()
        full.score_pairs_mlp(t(bad), t(case.items)); full.check()          # (a row the whole table has)
    bad = case.items.copy(); bad[B // 3] = -5
    with pytest.raises(IndexError, match="item id -5 at position %d " % (B // 3)):
        shard.score_pairs_mlp(t(case.users), t(bad)); shard.check()
    full.close(); shard.close()


def _lds_model(H2):
    """E = 1 984, C = 4: K = 9 920, with H1 = 256 the generic kernel's 4 (K + H1 + H2) floats of LDS are 160 KiB at H2 = 64."""
    E, C, U, I = 1984, 4, 40, 30
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=9)
    rng = np.random.default_rng(10)
    cats = ((rng.integers(1, 2 ** C, I)[:, None] >> np.arange(C)[None, :]) & 1).astype(np.float32)
    return PM, RE, CE, cats, mlp_head((C + 1) * E, 256, H2, rng, scale=4.0)


def _assert_small_scores(eng, model, head, B=5):
    from oracle import m2d_oracle as oracle
    rng = np.random.default_rng(B)
    case = mlp_case(*model[:4], head, rng.integers(0, 40, B).astype(np.int32), rng.integers(0, 30, B).astype(np.int32), MLP_COEF)
    got = _score(eng, case, "m2d_mlp_generic")
    ref = oracle.inference_mlp(*model[:4], *head, case.users, case.items, coef=MLP_COEF)
    assert np.isfinite(ref).all()
    assert_scores_close(got, ref, what="generic kernel, K = 9920")


def test_mlp_generic_refuses_more_than_160_kib_of_lds():
    """4 (K + H1 + H2) floats: K + H1 + H2 = 10 241 is one float per wave too many.  The refusal is an error of the call, not of the
    engine: the same engine with a small head scores."""
    import torch
    model = _lds_model(65)
    eng = _engine_of(model)
    ids = torch.zeros(5, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="too large for the generic kernel"):
        eng.score_pairs_mlp(ids, ids)
    small = mlp_head(9920, 10, 7, np.random.default_rng(11), scale=4.0)
    eng.set_mlp_head(*small)
    _assert_small_scores(eng, model, small)
    eng.close()


def test_mlp_generic_at_exactly_160_kib_of_lds():
    """K + H1 + H2 = 10 240: the whole LDS of a compute unit as one block's dynamic allocation."""
    model = _lds_model(64)
    assert 4 * (9920 + 256 + 64) * 4 == 160 * 1024
    eng = _engine_of(model)
    _assert_small_scores(eng, model, model[4])
    eng.close()
