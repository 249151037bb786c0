"""m2d_catalogue_rank and m2d_topk_users_excluding at every width and at the edges of every launch, on the MI355X.

The inputs are tests/seen_dish_cases.py's exact-arithmetic recipes (tests/test_seen_dish_cases_cpu.py holds their conditions): float32
equals float64 on them, so every comparison with oracle.inference_f64 below is an equality of integers -- and of score bits.
The normal-table cases keep the older files' band checks, tolerances unchanged."""
import functools
import types

import numpy as np
import pytest
import torch

import seen_dish_cases as sd

pytestmark = pytest.mark.gpu

RANK_KERNEL, EXCL_KERNEL = "m2d_rank_count", "m2d_topk_excl_scan"


def _engine(PM, RE, CE, cats, coef=sd.COEF):
    import foodrec_amd
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=coef, device=torch.device("cuda", 0))
    eng.set_dish_categories(cats)
    return eng


@functools.lru_cache(maxsize=None)
def _launch_engine(E):
    r = sd.launch_recipe(E)
    return r, _engine(r.PM, r.RE, r.CE, r.cats)


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def _rank(eng, users, items, exclude=None):
    r, s = eng.catalogue_rank(_i32(users), _i32(items), exclude)
    eng.check()
    assert eng.last_kernel() == RANK_KERNEL
    return r.cpu().numpy(), s.cpu().numpy()


def _topk(eng, users, k, exclude, tier):
    eng.set_option("topk_excl_tier", tier)
    s, i = eng.topk_users_excluding(_i32(users), k, exclude)
    eng.check()
    assert eng.last_kernel() == EXCL_KERNEL
    return s.cpu().numpy(), i.cpu().numpy()


def _device_csr(off, ids):
    return torch.from_numpy(off).cuda(), torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()


def _assert_scores_are_the_oracles(S, users, ids, scores):
    """exact recipes: a listed score IS the float64 score; NaN for an empty-mask dish and for an absent entry (id -1)"""
    ids = np.asarray(ids, np.int64)
    want = np.where(ids >= 0, S[np.asarray(users).reshape((-1,) + (1,) * (ids.ndim - 1)), np.maximum(ids, 0)], np.nan)
    got = np.asarray(scores, np.float64)
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8]


def _assert_lists(S, users, want, got_s, got_i, what=""):
    bad = np.flatnonzero((got_i != want).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:4], got_i[bad[:4]], want[bad[:4]])
    _assert_scores_are_the_oracles(S, users, got_i, got_s)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# ---- 1. widths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", sd.WIDTHS)
def test_width_ranks_equal_host_ranks(E):
    r = sd.width_recipe(E)
    eng = _engine(r.PM, r.RE, r.CE, r.cats)
    r0, s0 = _rank(eng, r.q_users, r.q_items)
    assert eng.get_option("rank_resolved") > 0                # the exact arithmetic, not the bounds alone, did the work
    r1, s1 = _rank(eng, r.q_users, r.q_items, r.q_excl)
    assert eng.get_option("rank_resolved") > 0
    bad = np.flatnonzero(r0 != r.rank0)
    assert bad.size == 0, (bad.size, bad[:8], r0[bad[:8]], r.rank0[bad[:8]])
    bad = np.flatnonzero(r1 != r.rank1)
    assert bad.size == 0, (bad.size, bad[:8], r1[bad[:8]], r.rank1[bad[:8]])
    _assert_scores_are_the_oracles(r.S, r.q_users, r.q_items, s0)
    assert np.array_equal(_bits(s0), _bits(s1))


@pytest.mark.parametrize("E,k", [(E, k) for E in sd.WIDTHS for k in sd.width_ks(E)])
def test_width_lists_equal_host_lists(E, k):
    r = sd.width_recipe(E)
    eng = _engine(r.PM, r.RE, r.CE, r.cats)
    users = np.arange(r.U)
    want = sd.topk_lists(r.S, users, k, r.lists)
    assert (want >= 0).all()
    for tier in (0, 2):
        sc, li = _topk(eng, users, k, r.lists, tier)
        if tier == 2:
            assert eng.get_option("topk_excl_short") == r.U and eng.get_option("topk_excl_tiles_scanned") > 0
        elif (E, k) == (128, 10):
            assert 0 < eng.get_option("topk_excl_short") < r.U      # tier 1 served some users and handed on the others
        _assert_lists(r.S, users, want, sc, li, (E, k, tier))
        _, s = _rank(eng, np.repeat(users, k), li.reshape(-1))       # the same pairs through the rank call: the same bits
        assert np.array_equal(_bits(s).reshape(r.U, k), _bits(sc)), (E, k, tier)


@pytest.mark.parametrize("E", sd.NORMAL_WIDTHS)
def test_width_normal_tables_positions_and_bands(E):
    from test_gpu_topk_excluding import _assert_rank_equals_position, _own_top_plus_random
    rng = np.random.default_rng(800 + E)
    U, I, k, coef = 256, 5000, 10, 0.99
    PM, RE, CE = sd.normal_tables(rng, U, I, E)
    cats = sd.masks(rng, I)
    eng = _engine(PM, RE, CE, cats, coef)
    off, ids = _own_top_plus_random(eng, rng, U, I, 20, 20)
    sc, li = _assert_rank_equals_position(eng, U, I, k, off, ids)
    assert eng.last_kernel() == RANK_KERNEL
    s64 = {}
    score = lambda u: s64.setdefault(u, sd.oracle_scores(PM, RE, CE, cats, u, coef))      # noqa: E731
    for u in range(0, U, 8):
        sd.assert_list_band(score(u), ids[off[u]:off[u + 1]], li[u], sc[u])
    q_users = np.arange(0, U, 8)[rng.integers(0, U // 8, 48)]
    q_items = rng.integers(0, I, 48)
    rr, ss = _rank(eng, q_users, q_items)
    for q in range(48):
        sd.assert_rank_band(score(int(q_users[q])), int(q_items[q]), rr[q], ss[q])


@pytest.mark.parametrize("E", [200, 100])
def test_width_full_protocol_equals_sampled_protocol_and_model_topk(E):
    import foodrec_amd
    rng = np.random.default_rng(70 + E)
    U, I = 40, 600
    PM, RE, CE, cats = sd.exact_tables(rng, U, I, E)
    args = types.SimpleNamespace(num_categories=4, num_users=U, embed_size=E, high_level_score_coefficient=0.5)
    model = foodrec_amd.Model(args, PM, RE, CE, None, device=torch.device("cuda", 0))
    d2c = {str(d): [[float(v)] for v in cats[d]] for d in range(I)}
    testRatings, testNegatives, train = {}, {}, {}
    for u in range(U):
        p = int(rng.integers(0, I - 60))
        negs = sorted(rng.choice(np.arange(p + 1, I), 50, replace=False).tolist())
        testRatings[str(u)] = [p]
        testNegatives[str(u)] = [0] * 50 + negs
        cand = set([p] + negs)
        train[str(u)] = [d for d in range(I) if d not in cand]
    for K in (1, 10):
        h0, n0 = foodrec_amd.evaluate_model(None, model, testRatings, testNegatives, K, d2c)
        h1, n1 = foodrec_amd.evaluate_model_full(None, model, testRatings, train, K, d2c)
        assert h0 == h1 and n0 == n1, K
    assert 0 < sum(h1) < U                                    # K = 10 of 51 candidates: hits and misses both occur
    users = [str(u) for u in range(U)]
    model.set_dish_categories(d2c)
    _, ids = model.topk(users, 10, exclude=train)
    S = sd.score_matrix(PM, RE, CE, cats)
    want = sd.topk_lists(S, range(U), 10, [train[u] for u in users])
    assert np.array_equal(np.asarray(ids), want), np.argwhere(np.asarray(ids) != want)[:8]


# ---- 2. launch edges of catalogue_rank ---------------------------------------------------------------------------------------------------
def _check_ranks(r, eng, users, items, sets=None, what=""):
    """the call against the host table rank[u, p | X_u]; `sets`: (off, ids) of one exclusion set per user"""
    if sets is None:
        want = sd.ranks_excluding(r.pos, users, items)
        got, s = _rank(eng, users, items)
    else:
        qoff, qids = sd.gather_csr(sets[0], sets[1], users)
        want = sd.ranks_excluding(r.pos, users, items, qoff, qids)
        got, s = _rank(eng, users, items, (qoff, qids))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
    _assert_scores_are_the_oracles(r.S, users, items, s)
    return got


@pytest.mark.parametrize("E", [8, 132])
def test_rank_query_counts_around_the_sort_threshold(E):
    r, eng = _launch_engine(E)
    users, items = sd.random_queries(r, 129, 11)
    for sets in (None, sd.user_sets(r, 3)):
        got = {n: _check_ranks(r, eng, users[:n], items[:n], sets, (E, n)) for n in (1, 17, 63, 64, 65, 129)}
        assert np.array_equal(got[65][:64], got[64])          # 64: unsorted; 65: sorted (E <= 128)


@pytest.mark.parametrize("E,ns", [(8, 1), (8, 2), (8, 3), (132, 1), (132, 2), (132, 512)])
def test_rank_share_counts(E, ns):
    r, eng = _launch_engine(E)
    cu = eng.get_option("num_cu")
    n = sd.share_counts(E, cu)[ns]
    assert sd.rank_nsplit(E, n, cu) == ns
    users, items = sd.random_queries(r, n, 12 + ns)
    _check_ranks(r, eng, users, items, None, (E, ns))
    assert eng.get_option("rank_resolved") > 0
    _check_ranks(r, eng, users, items, sd.user_sets(r, 3), (E, ns, "excl"))   # E = 8, ns = 1: n + 1 offsets, 2048 num_cu threads


def test_rank_exclude_ids_past_one_grid():
    r, eng = _launch_engine(32)
    cu = eng.get_option("num_cu")
    rng = np.random.default_rng(13)
    n, per = 700, max(60, 128 * cu // 700 + 8)
    users, items = sd.random_queries(r, n, 14)
    off, ids = sd.lists_csr([rng.choice(r.I, per, replace=False) for _ in range(n)])
    assert off[-1] > 128 * cu                                 # more ids than 16-lane groups in m2d_rank_exclude's grid
    want = sd.ranks_excluding(r.pos, users, items, off, ids)
    got, _ = _rank(eng, users, items, (off, ids))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("E", [132, 48])
def test_rank_user_base_shard(E):
    r, eng = _launch_engine(E)
    users, items = sd.random_queries(r, 200, 15)
    users = users // 2 + r.U // 2                             # the upper half
    sets = sd.user_sets(r, 3)
    full = _check_ranks(r, eng, users, items, sets, E)
    shard = _engine(r.PM[r.U // 2:], r.RE, r.CE, r.cats)
    shard.set_user_base(r.U // 2)
    qoff, qids = sd.gather_csr(sets[0], sets[1], users)
    got, _ = _rank(shard, users, items, (qoff, qids))
    assert np.array_equal(got, full)


# ---- 3. launch edges of topk_users_excluding -------------------------------------------------------------------------------------------
def _variant_call(r, eng, E, n, k, size, seed, tier=2, device=False):
    """n users drawn with repeats, each with one of its VARIANTS exclusion sets -> (users, want, scores, ids)"""
    voff, vids, vwant = sd.variant_lists(E, size, k)
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, r.U * sd.VARIANTS, n)
    users = rows // sd.VARIANTS
    off, ids = sd.gather_csr(voff, vids, rows)
    sc, li = _topk(eng, users, k, _device_csr(off, ids) if device else (off, ids), tier)
    return users, vwant[rows], sc, li


@pytest.mark.parametrize("E", [8, 132])
def test_topk_user_counts_around_one_wave(E):
    r, eng = _launch_engine(E)
    for n in (1, 63, 64, 65):
        users, want, sc, li = _variant_call(r, eng, E, n, 16, 4, 20 + n)
        assert eng.get_option("topk_excl_short") == n
        _assert_lists(r.S, users, want, sc, li, (E, n))


@pytest.mark.parametrize("E", [8, 64])
def test_topk_segments_around_the_lds_limit(E):
    r, eng = _launch_engine(E)
    users, lens, lists = sd.xs_segments(r)
    want = sd.topk_lists(r.S, users, 16, lists)
    sc, li = _topk(eng, users, 16, lists, 2)
    assert eng.get_option("topk_excl_tiles_scanned") > 0
    _assert_lists(r.S, users, want, sc, li, E)


def test_topk_tier1_exact_boundary():
    r, eng = _launch_engine(64)
    users, lists = sd.boundary_sets(r)
    want = sd.topk_lists(r.S, users, 10, lists)
    sc, li = _topk(eng, users, 10, lists, 0)
    assert eng.get_option("topk_excl_short") == users.size // 2      # exactly k survivors: not short; k - 1: short
    _assert_lists(r.S, users, want, sc, li)
    sc2, li2 = _topk(eng, users, 10, lists, 2)
    assert np.array_equal(li2, li) and np.array_equal(_bits(sc2), _bits(sc))


@pytest.mark.parametrize("odd_short", [True, False])
@pytest.mark.parametrize("at", [0, 64])
def test_topk_one_short_user_and_all_but_one(at, odd_short):
    r, eng = _launch_engine(64)
    users, lists = sd.odd_one_sets(r, odd_short, at)
    want = sd.topk_lists(r.S, users, 10, lists)
    sc, li = _topk(eng, users, 10, lists, 0)
    assert eng.get_option("topk_excl_short") == (1 if odd_short else users.size - 1)
    _assert_lists(r.S, users, want, sc, li, (at, odd_short))


@pytest.mark.parametrize("E,tier", [(32, 0), (32, 2), (132, 2)])
def test_topk_too_few_dishes_remain(E, tier):
    r, eng = _launch_engine(E)
    users, lists = sd.too_few_sets(r)
    want = sd.topk_lists(r.S, users, 16, lists)
    sc, li = _topk(eng, users, 16, lists, tier)
    _assert_lists(r.S, users, want, sc, li, (E, tier))
    assert (li[:, 9:] == -1).all() and np.isnan(sc[:, 7:]).all() and not np.isnan(sc[:, :7]).any()


@pytest.mark.parametrize("E,ns", [(8, 1), (8, 2), (8, 3), (132, 1), (132, 2)])
def test_topk_share_counts(E, ns):
    r, eng = _launch_engine(E)
    cu = eng.get_option("num_cu")
    n = sd.share_counts(E, cu)[ns]
    assert sd.excl_nsplit(E, n, cu) == ns
    users, want, sc, li = _variant_call(r, eng, E, n, 3, 4, 30 + ns, device=True)     # (E = 8, ns = 1: 4 n ids > 1024 num_cu threads)
    assert eng.get_option("topk_excl_short") == n and eng.get_option("topk_excl_tiles_scanned") > 0
    _assert_lists(r.S, users, want, sc, li, (E, ns))
    if (E, ns) == (8, 1):
        # scratch regrowth: a 3-user call in between, then the largest again -- the same bits
        _topk(eng, [5, 1, 9], 3, [[1, 2], [], [7]], 2)
        _, _, sc2, li2 = _variant_call(r, eng, E, n, 3, 4, 30 + ns, device=True)
        assert np.array_equal(li2, li) and np.array_equal(_bits(sc2), _bits(sc))
