"""Tables that hold inf / NaN (a diverged training run): the DEFAULT configuration returns what the reference graph
returns.  Model_Recommender.py:82 multiplies the Personal_Memory row of every category a dish does not have by 0, and
0 * inf = NaN, so a score is NaN wherever such a row is not finite.  The kernels that leave those rows out (option
skip_masked = 1, the pattern-grouped forms) read the engine's "a table value is not finite" word and stop doing so:
the word is set by the table scan queued at m2d_create / m2d_tables_updated and by the engine's own writers.

Two parts.  The first plants its poison in low-level Personal_Memory rows and follows the word through the engine's writers.  The
second (from test_every_table_and_column_on_the_pair_launches on) plants one element in every table -- U_high, a low-level row,
Recipe_Embedding, Category_Embedding, the ingredient table -- in the float4 column that idle lanes read again and in the last
one, +inf, -inf and NaN, on every pair launch and on retrieval; its inputs are helpers.nonfinite_case, whose own conditions
tests/test_nonfinite_cases_cpu.py asserts."""
import numpy as np
import pytest

from helpers import (NONFINITE_COLS, NONFINITE_E_FULL, NONFINITE_E_PARTIAL, NONFINITE_I, NONFINITE_TABLES, NONFINITE_VALUES, TOL,
                     assert_scores_close, assert_scores_match_nonfinite, nonfinite_case, random_case)

pytestmark = pytest.mark.gpu


def _masks(rng, B, C):
    m = (rng.integers(1, 2 ** C, B)[:, None] >> np.arange(C)[None, :] & 1).astype(np.float32)     # non-empty 0/1 masks
    m[::7] *= rng.uniform(0.5, 2.0, (len(m[::7]), C)).astype(np.float32)                          # some weighted
    return m


# c4 throughput / latency forms (full and partial lane groups), the C != 4 vectorised form, the generic kernel
@pytest.mark.parametrize("C,E,B", [(4, 64, 20000), (4, 64, 700), (4, 200, 9000), (4, 24, 300), (3, 16, 9000), (6, 32, 12000),
                                   (4, 7, 500), (9, 64, 300)])
@pytest.mark.parametrize("poison", [np.inf, -np.inf, np.nan])
def test_default_scores_equal_the_reference_graph_on_nonfinite_tables(C, E, B, poison):
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I = 400, 300
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=E + C)
    rng = np.random.default_rng(E)
    cats = _masks(rng, B, C)
    ut, it, ct = (torch.as_tensor(x, device="cuda") for x in (users, items, cats))
    eng = ScoringEngine(PM, RE, CE)
    clean = eng.score_pairs(ut, it, ct).cpu().numpy(); eng.check()
    eng.set_option("skip_masked", 0)
    assert np.array_equal(clean, eng.score_pairs(ut, it, ct).cpu().numpy())          # finite tables: same bits either way
    # poison low-level rows of a few users: every pair of theirs whose dish lacks that category is NaN in the graph
    PM2 = PM.copy()
    for u in rng.choice(U, 5, replace=False):
        PM2[u, 1 + rng.integers(0, C), rng.integers(0, E)] = poison
    ref = oracle.inference_f64(PM2, RE, CE, users, items, cats)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    eng2 = ScoringEngine(PM2, RE, CE)
    assert eng2.get_option("skip_masked") == 1                                       # the default configuration
    got = eng2.score_pairs(ut, it, ct).cpu().numpy(); eng2.check()
    assert_scores_match_nonfinite(got, ref, what="default options, non-finite Personal_Memory")
    hb = eng2.score_pairs_host(users[:51], items[:51], cats[:51])                   # the reference-shaped host call
    assert_scores_match_nonfinite(hb, ref[:51], what="host feed")


def test_in_place_edits_are_rescanned_after_tables_updated():
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, B = 300, 200, 4, 64, 20000
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=3)
    cats = _masks(np.random.default_rng(1), B, C)
    pmt = torch.as_tensor(PM, device="cuda")
    eng = ScoringEngine(pmt, RE, CE)                     # the engine borrows pmt
    ut, it, ct = (torch.as_tensor(x, device="cuda") for x in (users, items, cats))
    a = eng.score_pairs(ut, it, ct).cpu().numpy(); eng.check()
    assert_scores_close(a, oracle.inference_f64(PM, RE, CE, users, items, cats))
    pmt[17, 2, 5] = float("inf")
    eng.tables_updated()
    PM2 = PM.copy(); PM2[17, 2, 5] = np.inf
    assert_scores_match_nonfinite(eng.score_pairs(ut, it, ct).cpu().numpy(), oracle.inference_f64(PM2, RE, CE, users, items, cats))
    pmt[17, 2, 5] = 0.25                                 # repaired: the next scan clears the word, rows are skipped again
    eng.tables_updated()
    PM2[17, 2, 5] = 0.25
    got = eng.score_pairs(ut, it, ct).cpu().numpy(); eng.check()
    assert not np.isnan(got).any()
    assert_scores_close(got, oracle.inference_f64(PM2, RE, CE, users, items, cats))
    # Recipe_Embedding / Category_Embedding are part of the scan (the grouped MLP / retrieval forms depend on them)
    ret = torch.as_tensor(RE, device="cuda")
    eng3 = ScoringEngine(PM, ret, CE)
    eng3.score_pairs(ut, it, ct); eng3.check()
    ret[5, 3] = float("nan")
    eng3.tables_updated()
    RE2 = RE.copy(); RE2[5, 3] = np.nan
    assert_scores_close(eng3.score_pairs(ut, it, ct).cpu().numpy(), oracle.inference_f64(PM, RE2, CE, users, items, cats))


@pytest.mark.parametrize("learner", ["adam", "adagrad"])
def test_a_training_step_that_writes_nonfinite_values_sets_the_word(learner):
    """No tables_updated() is needed after the engine's own writers.  The divergence is planted in an optimizer slot (Adam's
    m, Adagrad's accumulator) so that one step writes a non-finite value into a low-level row of user 17 only."""
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, B = 200, 100, 4, 32, 9000
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=8)
    cats = _masks(np.random.default_rng(2), B, C)
    ut, it, ct = (torch.as_tensor(x, device="cuda") for x in (users, items, cats))
    pmt = torch.as_tensor(PM.copy(), device="cuda")
    eng = ScoringEngine(pmt, RE, CE)
    assert not np.isnan(eng.score_pairs(ut, it, ct).cpu().numpy()).any()       # scanned: finite
    eng.train_begin(learner, lr=0.001)
    slot = torch.zeros_like(pmt) if learner == "adam" else torch.full_like(pmt, 0.1)
    slot[17, 2, 5] = float("inf") if learner == "adam" else float("nan")
    eng.train_slot(0, 0, restore=slot)
    tu = torch.full((64,), 17, dtype=torch.int32, device="cuda")              # user 17 is in the batch (adagrad touches its rows only)
    eng.train_step(tu, it[:64], torch.ones((64, C), device="cuda"), torch.ones(64, device="cuda"))
    eng.check()
    pm_now = pmt.cpu().numpy()
    assert not np.isfinite(pm_now[17, 2, 5]) and np.isfinite(np.delete(pm_now[17].ravel(), 2 * E + 5)).all()
    ref = oracle.inference_f64(pm_now, eng.re.cpu().numpy(), eng.ce.cpu().numpy(), users, items, cats)
    lacking = (users == 17) & (cats[:, 1] == 0)
    assert lacking.any() and np.isnan(ref[lacking]).all()
    got = eng.score_pairs(ut, it, ct).cpu().numpy(); eng.check()
    assert_scores_match_nonfinite(got, ref, what="after a diverged %s step" % learner)


def test_write_memory_that_adds_inf_sets_the_word():
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, B, L = 200, 100, 4, 32, 9000, 7
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=8)
    items = (items % (I - 1)).astype(np.int32)                                 # dish I - 1 is written from, never scored
    RE = RE.copy(); RE[I - 1, 2] = 3e38                                        # finite, but 10 x it is not
    cats = _masks(np.random.default_rng(2), B, C)
    ut, it, ct = (torch.as_tensor(x, device="cuda") for x in (users, items, cats))
    pmt = torch.as_tensor(PM.copy(), device="cuda")
    eng = ScoringEngine(pmt, RE, CE)
    assert not np.isnan(eng.score_pairs(ut, it, ct).cpu().numpy()).any()       # the scan has run, the word is clear
    gm = torch.zeros((L, C + 1, E), device="cuda")
    wu = torch.arange(8, dtype=torch.int32, device="cuda")
    wi = torch.full((8,), I - 1, dtype=torch.int32, device="cuda")
    wc = torch.zeros((8, C), device="cuda"); wc[:, 0] = 1                      # category 0 only: row 1 of the user block
    lab = torch.zeros((8, L), device="cuda"); lab[:, 0] = 1
    eng.write_memory(wu, wi, wc, torch.full((8, 1), 10.0, device="cuda"), lab, gm, 1.0, 0.1, 0.1, write_pm=True, write_gm=False)
    eng.check()
    pm_now = pmt.cpu().numpy()
    assert np.isinf(pm_now[:8, 1, 2]).all() and np.isfinite(pm_now[:8, 2:]).all() and np.isfinite(pm_now[8:]).all()
    ref = oracle.inference_f64(pm_now, RE, CE, users, items, cats)
    lacking = (users < 8) & (cats[:, 0] == 0)
    assert lacking.any() and np.isnan(ref[lacking]).all()
    got = eng.score_pairs(ut, it, ct).cpu().numpy(); eng.check()
    assert_scores_match_nonfinite(got, ref, what="after Write_Memory added inf")


def test_scan_covers_the_last_values_of_a_table_whose_size_is_not_a_multiple_of_four():
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, B = 401, 301, 4, 7, 9000                                       # 14 035 / 2 107 floats: 3 beyond the last float4
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=12)
    cats = _masks(np.random.default_rng(3), B, C)
    PM[-1, -1, -1] = np.inf
    users[:50] = U - 1
    eng = ScoringEngine(PM, RE, CE)
    got = eng.score_pairs(*(torch.as_tensor(x, device="cuda") for x in (users, items, cats))).cpu().numpy(); eng.check()
    assert_scores_match_nonfinite(got, oracle.inference_f64(PM, RE, CE, users, items, cats))


@pytest.mark.parametrize("with_ingredients", [False, True])
def test_grouped_mlp_head_keeps_every_block_when_it_has_to(with_ingredients):
    """The pattern-grouped producer / consumer kernel (B >= 16384): a non-finite table value, and a dish whose weights
    sum to 0 (NaN blocks even where m_c = 0 -- with an ingredient table block 0 stays finite, so nothing else makes the
    score NaN), run every k-block: same NaN positions as the ungrouped kernel and the restatement."""
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    U, I, C, E, B = 300, 200, 4, 64, 20000
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=31)
    rng = np.random.default_rng(4)
    dish_cats = (rng.integers(1, 16, I)[:, None] >> np.arange(C)[None, :] & 1).astype(np.float32)
    dish_cats[3] = 0                                      # empty mask
    dish_cats[9] = [1, -1, 0, 0]                          # weights that sum to 0
    K = (C + 1) * E
    W1 = (rng.standard_normal((K, 256)) / np.sqrt(K)).astype(np.float32)
    b1 = (rng.standard_normal(256) * 0.1).astype(np.float32)
    W2 = (rng.standard_normal((256, 64)) / 16).astype(np.float32)
    b2 = (rng.standard_normal(64) * 0.1).astype(np.float32)
    w3 = (rng.standard_normal(64) / 8).astype(np.float32)
    ut, it = torch.as_tensor(users, device="cuda"), torch.as_tensor(items, device="cuda")

    def run(pm):
        eng = ScoringEngine(pm, RE, CE)
        eng.set_dish_categories(dish_cats)
        eng.set_mlp_head(W1, b1, W2, b2, w3, 0.25)
        if with_ingredients:
            R = 50
            lens = np.random.default_rng(5).integers(1, 6, I)
            off = np.zeros(I + 1, np.int32); off[1:] = np.cumsum(lens)
            eng.set_ingredients((np.random.default_rng(6).standard_normal((R, E)) / 8).astype(np.float32), off,
                                np.random.default_rng(7).integers(0, R, int(off[-1])).astype(np.int32))
        g = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
        assert eng.last_kernel() == "m2d_mlp_pc_bf16x3"
        eng.set_option("mlp_form", 1)                      # the ungrouped every-wave-gathers kernel
        u = eng.score_pairs_mlp(ut, it).cpu().numpy(); eng.check()
        return g, u

    g, u = run(PM)
    assert np.array_equal(np.isnan(g), np.isnan(u))
    assert np.isnan(g[(items == 3) | (items == 9)]).all() and not np.isnan(g[(items != 3) & (items != 9)]).any()
    assert np.allclose(g[~np.isnan(g)], u[~np.isnan(u)], rtol=1e-4, atol=1e-4)
    if not with_ingredients:
        assert_scores_close(g, oracle.inference_mlp(PM, RE, CE, dish_cats, W1, b1, W2, b2, w3, 0.25, users, items))
    PM2 = PM.copy()
    PM2[users[0], 1 + int(np.flatnonzero(dish_cats[items[0]] == 0)[0]) if (dish_cats[items[0]] == 0).any() else 1, 2] = np.inf
    g2, u2 = run(PM2)
    assert np.array_equal(np.isnan(g2), np.isnan(u2)) and np.isnan(g2).sum() > np.isnan(g).sum()


def test_retrieval_takes_the_dense_kernel_on_nonfinite_tables():
    """w_P = sum of the pattern's U_low rows leaves out the 0 * U_low[c] products: with a non-finite table value the
    pattern-grouped retrieval kernels are not used (the literal kernel, m2d_topk_literal, multiplies everything, like the pair
    path; the factored dense kernel does not: see test_retrieval_on_nonfinite_tables_returns_the_graphs_lists)."""
    import torch
    from foodrec_amd import ScoringEngine
    U, I, C, E, k = 200, 500, 4, 64, 10
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=5)
    rng = np.random.default_rng(9)
    dish_cats = (rng.integers(1, 16, I)[:, None] >> np.arange(C)[None, :] & 1).astype(np.float32)
    pmt = torch.as_tensor(PM, device="cuda")
    eng = ScoringEngine(pmt, RE, CE)
    eng.set_dish_categories(dish_cats)
    users = torch.arange(U, dtype=torch.int32, device="cuda")
    s0, i0 = eng.topk_users(users, k); eng.check()
    assert eng.last_kernel().startswith("m2d_topk_grouped")
    pmt[7, 2, 0] = float("inf")
    eng.tables_updated()
    s1, i1 = eng.topk_users(users, k); eng.check()
    assert eng.last_kernel() == "m2d_topk_literal"
    s0, s1, i0, i1 = (x.cpu().numpy() for x in (s0, s1, i0, i1))
    keep = np.arange(U) != 7
    assert np.array_equal(i0[keep], i1[keep])             # the other users are untouched
    # user 7: every dish without category 1 scores NaN in the graph and can never enter a list
    ut = torch.full((I,), 7, dtype=torch.int32, device="cuda")
    it = torch.arange(I, dtype=torch.int32, device="cuda")
    pair = eng.score_pairs(ut, it, torch.as_tensor(dish_cats, device="cuda")).cpu().numpy(); eng.check()
    assert np.isnan(pair[dish_cats[:, 1] == 0]).all()
    finite = np.flatnonzero(~np.isnan(pair))
    best = finite[np.argsort(-pair[finite], kind="stable")][:k]
    assert set(i1[7][:min(k, len(best))]) == set(best)


def test_retrieval_after_write_memory_added_inf_takes_the_dense_kernel():
    """The sorted dish rows of the pattern-grouped retrieval survive a Write_Memory on Personal_Memory (it touches no dish
    row), but the word "a table value is inf / NaN" may have been set by it: the next m2d_topk_users reads it again, takes the
    literal kernel and keeps the dishes whose score is NaN in the graph (0 * inf, Model_Recommender.py:82) out of the lists --
    the same answer as the pair path (`score_pairs`) gives for those users."""
    import torch
    from foodrec_amd import ScoringEngine
    U, I, C, E, k, L = 200, 500, 4, 64, 10, 7
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=15)
    RE = RE.copy(); RE[I - 1, 2] = 3e38                                        # finite, but 10 x it is not
    rng = np.random.default_rng(19)
    dish_cats = (rng.integers(1, 16, I)[:, None] >> np.arange(C)[None, :] & 1).astype(np.float32)
    pmt = torch.as_tensor(PM.copy(), device="cuda")
    eng = ScoringEngine(pmt, RE, CE)
    eng.set_dish_categories(dish_cats)
    users = torch.arange(U, dtype=torch.int32, device="cuda")
    s0, i0 = eng.topk_users(users, k); eng.check()
    assert eng.last_kernel().startswith("m2d_topk_grouped")                   # the grouped tables are built, the word is clear
    gm = torch.zeros((L, C + 1, E), device="cuda")
    wu = torch.arange(8, dtype=torch.int32, device="cuda")
    wi = torch.full((8,), I - 1, dtype=torch.int32, device="cuda")
    wc = torch.zeros((8, C), device="cuda"); wc[:, 0] = 1                      # category 0 only: row 1 of the user block
    lab = torch.zeros((8, L), device="cuda"); lab[:, 0] = 1
    eng.write_memory(wu, wi, wc, torch.full((8, 1), 10.0, device="cuda"), lab, gm, 1.0, 0.1, 0.1, write_pm=True, write_gm=False)
    eng.check()
    assert np.isinf(pmt[:8, 1, 2].cpu().numpy()).all()
    s1, i1 = eng.topk_users(users, k); eng.check()
    assert eng.last_kernel() == "m2d_topk_literal"
    s1, i1, s0, i0 = s1.cpu().numpy(), i1.cpu().numpy(), s0.cpu().numpy(), i0.cpu().numpy()
    # users that were not written to: the same lists (another kernel, another rounding: where two dishes change places their
    # scores are closer than the split-bf16 product's error)
    differ = i0[8:] != i1[8:]
    close = np.abs(s0[8:] - s1[8:]) <= 3e-5 * np.maximum(1.0, np.abs(s1[8:]))        # (dish I - 1 scores ~1e36 for everybody)
    assert differ.mean() < 0.02 and np.all(close)
    it = torch.arange(I, dtype=torch.int32, device="cuda")
    ct = torch.as_tensor(dish_cats, device="cuda")
    for u in range(8):
        pair = eng.score_pairs(torch.full((I,), u, dtype=torch.int32, device="cuda"), it, ct).cpu().numpy(); eng.check()
        assert np.isnan(pair[dish_cats[:, 0] == 0]).all()                      # dishes without category 0: 0 * inf
        ranked = np.flatnonzero(~np.isnan(pair))
        best = ranked[np.argsort(-pair[ranked], kind="stable")][:k]
        assert set(i1[u][:len(best)].tolist()) == set(best.tolist()), u
        assert not (set(i1[u][:len(best)].tolist()) & set(np.flatnonzero(dish_cats[:, 0] == 0).tolist()))


# ---- one element of every table, both columns, +-inf and NaN ------------------------------------------------------------------
def _launch(name, C, E, B, kernel, **opts):
    return pytest.param(C, E, B, kernel, opts, id=name)


# c4 throughput form (B = 9000) and latency form (B = 300) at partial and full lane groups; each once under its forcing option;
# the prefetch / temporal-load instantiations; the C != 4 vectorised form; the generic kernel
PAIR_LAUNCHES = (
    [_launch("c4-E%d-B9000" % E, 4, E, 9000, "m2d_score_pairs_c4") for E in NONFINITE_E_PARTIAL + NONFINITE_E_FULL] +
    [_launch("c4small-E%d-B300" % E, 4, E, 300, "m2d_score_pairs_c4_small") for E in NONFINITE_E_PARTIAL + NONFINITE_E_FULL] +
    [_launch("c4-E24-B300-variant11", 4, 24, 300, "m2d_score_pairs_c4", variant=11),
     _launch("c4small-E24-B9000-variant12", 4, 24, 9000, "m2d_score_pairs_c4_small", variant=12)] +
    [_launch("c4-E%d-B9000-pf%d-nt0" % (E, pf), 4, E, 9000, "m2d_score_pairs_c4", prefetch=pf, nt_loads=0) for E in (24, 64) for pf in (1, 4)] +
    [_launch("cn-C3-E16-B9000", 3, 16, 9000, "m2d_score_pairs_cn"), _launch("cn-C6-E36-B9000", 6, 36, 9000, "m2d_score_pairs_cn"),
     _launch("generic-C4-E7-B300", 4, 7, 300, "m2d_score_pairs_generic"), _launch("generic-C9-E64-B300", 9, 64, 300, "m2d_score_pairs_generic")])


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()            # (a copy: the case builder's arrays are read-only and shared)


def _same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _dish_table(C, d, seed):
    """Masks by dish for `score_pairs_bydish`: random non-empty 0/1 patterns, the poisoned dish has every category."""
    t = (np.random.default_rng(seed).integers(1, 2 ** C, NONFINITE_I)[:, None] >> np.arange(C)[None, :] & 1).astype(np.float32)
    t[d] = 1
    return t


@pytest.mark.parametrize("table", NONFINITE_TABLES)
@pytest.mark.parametrize("C,E,B,kernel,opts", PAIR_LAUNCHES)
def test_every_table_and_column_on_the_pair_launches(C, E, B, kernel, opts, table):
    """One (launch, table): the element at `col` set to each of +inf, -inf, NaN in place (tables_updated), per-pair masks and
    masks by dish.  NaN at the graph's pairs, the graph's infinities, the rest inside the 1e-4 bound; pairs whose user and dish the
    poison does not reach: the clean engine's bits."""
    from foodrec_amd import ScoringEngine
    seed = E + C
    base = nonfinite_case(C, E, B, table, "first", np.nan, seed)
    dish_cats = _dish_table(C, base.d, seed)
    pm, re_, ce = _dev(base.PM0), _dev(base.RE0), _dev(base.CE0)
    eng = ScoringEngine(pm, re_, ce)
    eng.set_dish_categories(dish_cats)
    for name, v in opts.items():
        eng.set_option(name, v)
    ut, it, ct = _dev(base.users), _dev(base.items), _dev(base.cats)
    clean = eng.score_pairs(ut, it, ct).cpu().numpy()
    assert eng.last_kernel() == kernel
    clean_bd = eng.score_pairs_bydish(ut, it).cpu().numpy(); eng.check()
    assert eng.last_kernel() == kernel
    assert_scores_close(clean, base.ref0, what="clean")
    tensor, at = {"U_high": (pm, (base.u, 0)), "U_low": (pm, (base.u, 1 + base.c)), "RE": (re_, (base.d,)), "CE": (ce, (base.c,))}[table]
    for col in NONFINITE_COLS:
        for value in NONFINITE_VALUES:
            case = nonfinite_case(C, E, B, table, col, value, seed)
            case_bd = nonfinite_case(C, E, B, table, col, value, seed, dish_cats=dish_cats)
            what = "%s %s %s %r" % (kernel, table, col, value)
            was = float(tensor[at + (case.e,)])
            tensor[at + (case.e,)] = float(value)
            eng.tables_updated()
            got = eng.score_pairs(ut, it, ct).cpu().numpy()
            got_bd = eng.score_pairs_bydish(ut, it).cpu().numpy(); eng.check()
            host = eng.score_pairs_host(base.users[:51], base.items[:51], base.cats[:51]) if E == 200 else None
            tensor[at + (case.e,)] = was
            assert_scores_match_nonfinite(got, case.ref, what=what)
            assert_scores_match_nonfinite(got_bd, case_bd.ref, what=what + ", masks by dish")
            ok = ~case.touched
            assert _same_bits(got[ok], clean[ok]) and _same_bits(got_bd[ok], clean_bd[ok]), what + ": a pair the poison does not reach moved"
            if host is not None:                            # the reference-shaped host call
                assert_scores_match_nonfinite(host, case.ref[:51], what=what + ", host feed")
    eng.close()


def _ingredients(I, E, d, seed):
    """A small ingredient table: R = 50 rows, 1..5 ingredients a dish, weights in (0.5, 2); dish d's first ingredient is `r`."""
    rng = np.random.default_rng(seed)
    R = 50
    lens = rng.integers(1, 6, I)
    off = np.zeros(I + 1, np.int32); off[1:] = np.cumsum(lens)
    ids = rng.integers(0, R, int(off[-1])).astype(np.int32)
    w = rng.uniform(0.5, 2.0, len(ids)).astype(np.float32)
    ING = (rng.standard_normal((R, E)) / np.sqrt(E)).astype(np.float32)
    return ING, off, ids, w, int(ids[off[d]])


@pytest.mark.parametrize("table", ["U_high", "RE", "ING"])
@pytest.mark.parametrize("E,B,kernel", [(24, 9000, "m2d_score_pairs_c4_hv"), (24, 300, "m2d_score_pairs_c4_small_hv"),
                                        (64, 9000, "m2d_score_pairs_c4_hv"), (64, 300, "m2d_score_pairs_c4_small_hv")])
def test_every_table_with_the_ingredient_vector_on_the_pair_launches(E, B, kernel, table):
    """The ingredient forms (high = <U_high, H[d]>) against oracle.inference_ingredients: poison in U_high, in Recipe_Embedding
    and in the ingredient table itself (H[d] is rebuilt by m2d_set_ingredients)."""
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    seed = E + 4
    base = nonfinite_case(4, E, B, "U_high", "first", np.nan, seed)
    ING, off, ids, w, r = _ingredients(NONFINITE_I, E, base.d, seed)
    has_r = np.array([r in ids[off[i]:off[i + 1]] for i in range(NONFINITE_I)])
    touched = {"U_high": base.users == base.u, "RE": base.items == base.d, "ING": has_r[base.items]}[table]
    t = np.flatnonzero(touched)
    assert 64 <= len(t) < B // 2
    pm, re_ = _dev(base.PM0), _dev(base.RE0)
    eng = ScoringEngine(pm, re_, np.array(base.CE0))
    eng.set_ingredients(ING, off, ids, w)
    ut, it, ct = _dev(base.users), _dev(base.items), _dev(base.cats)
    clean = eng.score_pairs_ingredients(ut, it, ct).cpu().numpy(); eng.check()
    assert eng.last_kernel() == kernel
    ref0 = oracle.inference_ingredients(base.PM0, base.RE0, ING, off, ids, w, base.users, base.items, base.cats)
    assert_scores_close(clean, ref0, what="clean")
    for col in NONFINITE_COLS:
        e = 1 if col == "first" else E - 1
        for value in NONFINITE_VALUES:
            what = "%s %s %s %r" % (kernel, table, col, value)
            PM, RE, ING2 = base.PM0, base.RE0, ING
            if table == "U_high":
                PM = base.PM0.copy(); PM[base.u, 0, e] = value
                pm[base.u, 0, e] = float(value)
            elif table == "RE":
                RE = base.RE0.copy(); RE[base.d, e] = value
                re_[base.d, e] = float(value)
            else:
                ING2 = ING.copy(); ING2[r, e] = value
                eng.set_ingredients(ING2, off, ids, w)
            eng.tables_updated()
            got = eng.score_pairs_ingredients(ut, it, ct).cpu().numpy(); eng.check()
            pm[base.u, 0, e] = float(base.PM0[base.u, 0, e]); re_[base.d, e] = float(base.RE0[base.d, e])
            ref = ref0.copy()
            ref[t] = oracle.inference_ingredients(PM, RE, ING2, off, ids, w, base.users[t], base.items[t], base.cats[t])
            assert np.isnan(ref[t]).any() or np.isinf(ref[t]).any()
            if np.isinf(value):
                assert np.isinf(ref[:8]).any() and np.isinf(ref[56:64]).any(), what     # first and last lane group of the hand-built wave
            assert_scores_match_nonfinite(got, ref, what=what)
            assert _same_bits(got[~touched], clean[~touched]), what + ": a pair the poison does not reach moved"
    eng.close()


@pytest.mark.parametrize("table", ["U_high", "CE"])
@pytest.mark.parametrize("E", [24, 64])
def test_user_high_table_on_nonfinite_tables(E, table):
    """Option user_high_table = 1 at 2^18 + 77 pairs: the high-level sum from <U_high[u], CE_c> (m2d_build_user_high has the
    pair kernels' lane layout, idle lanes included).  Reference on the 64 hand-built pairs and every 97th pair."""
    from foodrec_amd import ScoringEngine
    B = 2 ** 18 + 77
    sel = np.r_[0:64, 64:B:97]
    seed = E + 4
    base = nonfinite_case(4, E, B, table, "first", np.nan, seed, ref_on=sel)
    pm, ce = _dev(base.PM0), _dev(base.CE0)
    eng = ScoringEngine(pm, np.array(base.RE0), ce)
    eng.set_option("user_high_table", 1)
    ut, it, ct = _dev(base.users), _dev(base.items), _dev(base.cats)
    clean = eng.score_pairs(ut, it, ct).cpu().numpy(); eng.check()
    assert eng.last_kernel() == "m2d_score_pairs_c4_uh"
    assert_scores_close(clean[sel], base.ref0, what="clean")
    tensor, at = (pm, (base.u, 0)) if table == "U_high" else (ce, (base.c,))
    reached = (base.users == base.u) if table == "U_high" else np.ones(B, bool)
    for col in NONFINITE_COLS:
        for value in NONFINITE_VALUES:
            case = nonfinite_case(4, E, B, table, col, value, seed, ref_on=sel)
            what = "user_high_table E%d %s %s %r" % (E, table, col, value)
            was = float(tensor[at + (case.e,)])
            tensor[at + (case.e,)] = float(value)
            eng.tables_updated()
            got = eng.score_pairs(ut, it, ct).cpu().numpy(); eng.check()
            tensor[at + (case.e,)] = was
            assert eng.last_kernel() == "m2d_score_pairs_c4_uh"
            assert_scores_match_nonfinite(got[sel], case.ref, what=what)
            assert _same_bits(got[~reached], clean[~reached]), what + ": a pair the poison does not reach moved"
    eng.close()


def test_evaluate_model_with_an_inf_in_one_test_users_high_row():
    """evaluate_model on E = 200 tables (partial lane groups) where one test user's U_high holds +inf in the float4 column idle
    lanes read again: that user's candidates score +inf (every category) or NaN, the segment is flagged and goes through the
    reference's host sequence; HR / NDCG of every user equal the oracle's evaluator over the float32 restatement."""
    import types
    import torch
    from foodrec_amd import Model, Session, clear_eval_plans, evaluate_model
    from oracle import m2d_oracle as oracle
    U, I, C, E, K, bad = 12, 160, 4, 200, 10, 5
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=41)
    CE[:, 1] = np.abs(CE[:, 1])
    PM[bad, 0, 1] = np.inf
    rng = np.random.default_rng(42)
    pat = rng.integers(1, 16, I); pat[::3] = 15
    d2c = {str(i): [[float(pat[i] >> c & 1)] for c in range(C)] for i in range(I)}
    ratings = {str(u): [int(rng.integers(0, I))] for u in range(U)}
    negatives = {str(u): [int(x) for x in rng.permutation(I)[:100]] for u in range(U)}
    ratings[str(bad)] = [int(np.flatnonzero(pat == 15)[7])]            # the held-out dish of that user scores +inf
    args = types.SimpleNamespace(num_categories=C, num_users=U, embed_size=E, high_level_score_coefficient=0.99)
    model = Model(args, PM, RE, CE, None)
    clear_eval_plans()
    hits, ndcgs = evaluate_model(Session(model), model, ratings, negatives, K, d2c)
    fn = lambda u, i, c: oracle.inference_f32(PM, RE, CE, u, i, c)
    rh, rn = oracle.evaluate_model(fn, ratings, negatives, K, d2c)
    sc = fn([bad] * 51, oracle.candidate_batch(bad, ratings, negatives), [d2c[str(i)] for i in oracle.candidate_batch(bad, ratings, negatives)])
    assert np.isposinf(sc).sum() >= 5 and np.isnan(sc).sum() >= 5 and not np.isfinite(sc).any()
    assert hits == rh and ndcgs == rn
    users = torch.arange(U, dtype=torch.int32, device="cuda")
    items = torch.as_tensor(np.array([oracle.candidate_batch(u, ratings, negatives) for u in range(U)], np.int32), device="cuda")
    s, ids, flags = model.engine.rank_candidates(users, items, K); model.engine.check()
    assert flags.cpu().numpy().tolist() == [1 if u == bad else 0 for u in range(U)]      # the NaN flag, that user alone
    clear_eval_plans()


# ---- retrieval --------------------------------------------------------------------------------------------------------------
def _assert_list_is_the_graphs(s, ids, ref, ref_s, ref_i, what):
    """One user's list against oracle.topk_catalogue's (ref_s, ref_i) and the float64 scores of the whole catalogue (`ref`).
    Positions whose reference score is +-inf or NaN: the oracle's id and its score (ties to the lower id, NaN after -inf).
    The others: test_gpu_catalogue._check's rules -- the score of the returned dish inside the bound, descending order,
    nothing left out that beats the last listed score, bit-equal scores in id order."""
    k = len(ref_i)
    odd = ~np.isfinite(ref_s)
    assert np.array_equal(ids[odd], ref_i[odd]), (what, ids, ref_i, ref_s)
    assert np.array_equal(s[odd], ref_s[odd].astype(np.float32), equal_nan=True), (what, s, ref_s)
    assert len(set(ids.tolist())) == k and ids.min() >= 0 and ids.max() < len(ref)
    fin = ~odd
    if fin.any():
        assert np.isfinite(s[fin]).all(), (what, s)
        assert_scores_close(s[fin], ref[ids[fin]], what=what)
        assert np.all(s[fin][:-1] >= s[fin][1:]), what + ": not descending"
        rest = np.delete(ref, ids)
        assert not np.isposinf(rest).any(), what
        rest = rest[np.isfinite(rest)]
        if odd[np.flatnonzero(fin)[-1] + 1:].any():          # -inf / NaN listed behind the finite scores: no finite score is left out
            assert rest.size == 0, what
        else:                                                # the list ends inside the finite scores: nothing left out beats its last
            last = s[fin][-1]
            assert rest.size == 0 or rest.max() <= last + TOL * max(1.0, abs(last)), (what, rest.max(), last)
        for a in np.flatnonzero(fin[:-1] & fin[1:]):
            if s[a] == s[a + 1]:
                assert ids[a] < ids[a + 1], what


TOPK_SHAPES = [(32, 10, False), (64, 10, False), (64, 16, False), (64, 17, False), (128, 10, False), (24, 10, False), (200, 10, False),
               (64, 10, True)]


@pytest.mark.parametrize("I", [333, 12])
@pytest.mark.parametrize("E,k,with_ingredients", TOPK_SHAPES)
def test_retrieval_on_nonfinite_tables_returns_the_graphs_lists(E, k, with_ingredients, I):
    """m2d_topk_users after one table element became inf (tables_updated after a clean call, so the grouped tables exist): the
    lists of oracle.topk_catalogue -- +inf first, -inf after every finite score, NaN last, each in id order.  The literal
    kernel serves the call whatever kernel the finite tables took, and a listed score is `score_pairs_bydish`'s under "variant" 9
    (m2d_score_pairs_generic) bit for bit.  I = 12: fewer finite dishes than k."""
    import torch
    from foodrec_amd import ScoringEngine
    from oracle import m2d_oracle as oracle
    from test_gpu_catalogue import _explain_mismatches, _tables
    U, C = 40, 4
    k = min(k, I)
    PM, RE, CE, cats = _tables(U, I, C, E, seed=E + k + I, n_nan=1)
    u, d, c, e = 7, 5, 2, 1
    cats[d] = 1                                              # the poisoned dish has every category: +-inf, not NaN
    CE[:, e] = np.abs(CE[:, e]); PM[u, 1:, e] = np.abs(PM[u, 1:, e])
    ing = r = None
    if with_ingredients:
        ING, off, ids_, w, r = _ingredients(I, E, d, seed=E)
        ing = (ING, off, ids_, w)
    pm, re_, ce = _dev(PM), _dev(RE), _dev(CE)
    eng = ScoringEngine(pm, re_, ce)
    eng.set_dish_categories(cats)
    if ing:
        eng.set_ingredients(*ing)
    users = np.arange(U)
    ut = torch.arange(U, dtype=torch.int32, device="cuda")
    s0, i0 = eng.topk_users(ut, k); eng.check()
    assert eng.last_kernel() != "m2d_topk_literal"
    s0, i0 = s0.cpu().numpy(), i0.cpu().numpy()
    poisons = [("U_high +inf", pm, (u, 0, e), np.inf), ("U_high -inf", pm, (u, 0, e), -np.inf), ("U_low", pm, (u, 1 + c, e), np.inf),
               ("RE", re_, (d, e), np.inf), ("CE", ce, (c, e), np.inf)] + ([("ING", None, (r, e), np.inf)] if ing else [])
    failures = []
    for name, tensor, at, value in poisons:
        what = "E%d k%d I%d %s" % (E, k, I, name)
        host = {id(pm): PM, id(re_): RE, id(ce): CE}.get(id(tensor))
        P = {"PM": PM, "RE": RE, "CE": CE}
        ing2 = ing
        if tensor is None:
            ING2 = ing[0].copy(); ING2[at] = value
            ing2 = (ING2,) + ing[1:]
            eng.set_ingredients(*ing2)
        else:
            alt = host.copy(); alt[at] = value
            P = {n: (alt if t is host else t) for n, t in P.items()}
            tensor[at] = float(value)
        eng.tables_updated()
        s1, i1 = eng.topk_users(ut, k); eng.check()
        kernel = eng.last_kernel()
        eng.set_option("variant", 9)                         # the generic pair kernel on the listed (user, dish) pairs
        pu, pi = ut.repeat_interleave(k), i1.reshape(-1).contiguous()
        pair = (eng.score_pairs_ingredients(pu, pi) if ing else eng.score_pairs_bydish(pu, pi)); eng.check()
        pair_kernel = eng.last_kernel()
        eng.set_option("variant", 0)
        if tensor is not None and not ing:                   # the ranking entry points refuse, whichever table it is
            with pytest.raises(ValueError, match="finite"):
                eng.catalogue_rank(ut[:3], torch.zeros(3, dtype=torch.int32, device="cuda"))
            with pytest.raises(ValueError, match="finite"):
                eng.topk_users_excluding(ut[:3], min(k, 16))
        if tensor is None:
            eng.set_ingredients(*ing)
        else:
            tensor[at] = float(host[at])
        same_bits = torch.equal(pair.view(torch.int32), s1.reshape(-1).view(torch.int32))
        s1, i1 = s1.cpu().numpy(), i1.cpu().numpy()
        ref_s, ref_i = oracle.topk_catalogue(P["PM"], P["RE"], P["CE"], cats, users, k, ingredients=ing2)
        seen = set()
        try:                                                 # (every poison is looked at: the message names all that fail)
            for q in range(U):
                if ing2:
                    ref = oracle.inference_ingredients(P["PM"], P["RE"], *ing2, np.full(I, q), np.arange(I), cats)
                else:
                    ref = oracle.inference_f64(P["PM"], P["RE"], P["CE"], np.full(I, q), np.arange(I), cats)
                _assert_list_is_the_graphs(s1[q], i1[q], ref, ref_s[q], ref_i[q], "%s user %d" % (what, q))
                seen |= {"+inf"} if np.isposinf(ref_s[q]).any() else set()
                seen |= {"-inf"} if np.isneginf(ref_s[q]).any() else set()
            # what the case is there for, from the reference alone
            if not (ing and name == "CE"):                   # (with the ingredient table Category_Embedding is not in the formula)
                assert "+inf" in seen or "-inf" in seen, what
            if name.startswith("U_high") and not ing:        # (with the ingredient table the sign is H[d][e]'s, dish by dish)
                assert name[-4:] in seen, (what, seen)        # -inf scores in a list: user u's dishes with every category
            assert kernel == "m2d_topk_literal", (what, kernel)
            assert pair_kernel == "m2d_score_pairs_generic" and same_bits, what + ": not the generic pair kernel's bits"
            if name.startswith("U_"):                        # users the poison does not touch: the clean engine's lists
                keep = users != u
                if not ing:
                    _explain_mismatches(PM, RE, CE, cats, users[keep], s0[keep], i0[keep], s1[keep], i1[keep])
                assert np.mean(i0[keep] == i1[keep]) > 0.98, what
        except AssertionError as err:
            failures.append("%s: %s" % (what, str(err)[:300]))
    assert not failures, "\n".join(failures)
    eng.tables_updated()
    eng.close()
