"""CPU checks of the deep retrieval lists (m2d_topk_users_deep / m2d_topk_users_mlp_deep; DESIGN.md sections 4.11, 8.8): the boundary
(header, ctypes table, option, engine methods, torch ops), the numpy restatement of m2d_select_deep's radix select against a plain
sort by key, float32 = float64 on the exact recipes, the conditions the GPU cases of tests/test_gpu_deep.py rely on, and the
wrong-kernel stand-ins under the same comparisons: each must change the answer of every case aimed at it."""
import inspect
import os
import re

import numpy as np
import pytest

import deep_cases as dc
import seen_dish_cases as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2d_topk_users_deep", "m2d_topk_users_mlp_deep")


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_in_the_header_and_the_ctypes_table():
    import ctypes as c
    from foodrec_amd import _native
    header = _read("include", "m2d.h")
    for name in NEW:
        assert "int %s(m2d_engine *h" % name in header, name
        assert name in _native.SIGNATURES
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_topk_users_deep"][1] == [vp, vp, i64, i32, vp, vp, vp, vp, vp]
    assert _native.SIGNATURES["m2d_topk_users_mlp_deep"][1] == [vp, vp, i64, i32, i32, vp, vp, vp, vp, vp]
    assert _native.ABI_VERSION == 2
    assert "m2d_select.hip" in _read("foodrec_amd", "csrc", "Makefile")
    src = _read("foodrec_amd", "csrc", "m2d_select.hip")
    assert "SD_BITS = %d" % dc.BITS in src and dc.BINS == 1 << dc.BITS
    assert "int m2d_launch_select(" in _read("foodrec_amd", "csrc", "m2d_engine.h") and "int m2d_launch_select(" in src


def test_option_bounds_as_the_source_states_them():
    """deep_chunk_pairs: 256 ... 2^24, default 2^22, set and read like slate_chunk_pairs"""
    abi = _read("foodrec_amd", "csrc", "m2d_abi.hip")
    # one row of the option table serves m2d_set_option (the range, refused with M2D_ERR_INVALID_ARG) and m2d_get_option (the member)
    m = re.search(r'opt\("deep_chunk_pairs", &m2d_engine::opt_deep_chunk_pairs, (\d+), 1 << (\d+), "256 \.\.\. 2\^24"\)', abi)
    assert m and (int(m.group(1)), int(m.group(2))) == (256, 24)
    assert abi.count('"deep_chunk_pairs"') == 1
    assert 'return fail(h, M2D_ERR_INVALID_ARG, std::string("m2d_set_option: ") + name + " takes " + o->takes);' in abi
    eng = _read("foodrec_amd", "csrc", "m2d_engine.h")
    assert "int64_t opt_deep_chunk_pairs = 1 << 22;" in eng and dc.DEFAULT_P == 1 << 22
    assert "deep_chunk_pairs" in _read("include", "m2d.h") and "deep_chunk_pairs" in _read("README.md")
    slate = _read("foodrec_amd", "csrc", "m2d_slate.hip")
    assert "W = W0 < 65536 ? W0 : 65536" in slate and "R = m2d_block_rows(P, W, nU)" in slate
    assert "R0 = P / W > 1 ? P / W : 1" in eng and "return R0 < n ? R0 : n" in eng          # the block rule: m2d_block_rows
    assert dc.ranges(1300, 256) == (256, 1) and dc.ranges(1300, 2048) == (1300, 1) and dc.ranges(100000, 1 << 22) == (65536, 64)


def test_python_surface():
    import torch
    from foodrec_amd import ops, recommender
    assert list(inspect.signature(ops.ScoringEngine.topk_users_deep).parameters) == ["self", "users", "k", "exclude"]
    assert list(inspect.signature(ops.ScoringEngine.topk_users_mlp_deep).parameters) == ["self", "users", "k", "exclude", "candidates"]
    sig = inspect.signature(recommender.Model.topk_deep)
    assert list(sig.parameters) == ["self", "users", "k", "exclude", "head", "candidates"] and sig.parameters["k"].default == 100
    u = torch.empty(7, dtype=torch.int32, device="meta")
    off, ids = torch.empty(8, dtype=torch.int64, device="meta"), torch.empty(3, dtype=torch.int32, device="meta")
    for got in (torch.ops.m2d.topk_users_deep(1, u, 300), torch.ops.m2d.topk_users_deep(1, u, 300, off, ids),
                torch.ops.m2d.topk_users_mlp_deep(1, u, 300), torch.ops.m2d.topk_users_mlp_deep(1, u, 300, 1024, off, ids)):
        s, i = got                                                                  # the fake implementations
        assert s.shape == i.shape == (7, 300) and s.dtype == torch.float32 and i.dtype == torch.int32


def test_k_is_checked_before_the_native_call():
    from foodrec_amd import ops, recommender
    for fn in (ops.ScoringEngine._topk_deep, recommender.Model.topk_deep):
        assert "1 <= k <= 1024" in inspect.getsource(fn)
    import torch
    eng = object.__new__(ops.ScoringEngine)                  # no engine: the check stands in front of everything native
    eng.device = torch.device("cpu")
    for k in (0, 1025, -1, True, 2.5):
        with pytest.raises(ValueError, match="1 <= k <= 1024"):
            eng.topk_users_deep(torch.zeros(3, dtype=torch.int32), k)
        with pytest.raises(ValueError, match="1 <= k <= 1024"):
            eng.topk_users_mlp_deep(torch.zeros(3, dtype=torch.int32), k, None, 0)


# ---- the radix select ------------------------------------------------------------------------------------------------------------------
def test_key_is_the_order():
    """score descending, -0 / +0 tied, bit-equal scores to the lower id, NaN after -inf in id order, no entry last"""
    s = np.asarray([1.0, -np.inf, np.nan, 0.0, -0.0, np.inf, 1.0, np.nan, -1.0], np.float32)
    k = dc.keys(dc.words(s), np.arange(9))
    assert np.argsort(k, kind="stable").tolist() == [5, 0, 6, 3, 4, 8, 1, 2, 7]
    assert (k < dc.NONE).all() and dc.keys(dc.words(np.float32(np.nan)), -1) == dc.NONE


def test_radix_select_equals_a_sort_on_random_rows():
    """10^5 rows: short and long, values from small pools (ties), NaN, infinities, both zeros, TKM_NONE holes, k on both sides of the
    number of real keys"""
    rng = np.random.default_rng(5)
    pool = np.concatenate([rng.standard_normal(40), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, np.nextafter(np.float32(1), 2)]]).astype(np.float32)
    total, seen_passes = 0, set()
    for W, n, k in ((24, 60000, 7), (24, 20000, 30), (100, 15000, 64), (700, 4000, 256), (3000, 1000, 1024)):
        s = pool[rng.integers(0, pool.size, (n, W))] if W < 700 else rng.standard_normal((n, W)).astype(np.float32)
        key = dc.keys(dc.words(s), np.broadcast_to(np.arange(W), (n, W)))
        key[rng.random((n, W)) < 0.1] = dc.NONE
        stats = {}
        got = dc.radix_select(key, k, stats=stats)
        assert np.array_equal(got, dc.sort_select(key, k)), (W, k)
        total += n
        seen_passes |= set(stats["passes"].tolist())
    assert total == 100000
    assert {1, 3, 6} <= seen_passes, seen_passes            # the early exits and the walk into the id word all happened


def test_radix_select_on_the_adversarial_rows():
    for key, k, what in dc.adversarial_rows(np.random.default_rng(6)):
        stats = {}
        got = dc.radix_select(key, k, stats=stats)
        assert np.array_equal(got, dc.sort_select(key, k)), what
        real = int((key != dc.NONE).sum())
        assert (got[0] == dc.NONE).sum() == max(0, k - real), what
        if real > k and "tie" in what or what in ("one value", "all +inf"):
            assert stats["passes"][0] >= 4, what             # equal score words: the id word decides
        if real <= k:
            assert stats["passes"][0] == 1, what             # every real key is listed after one pass
        short = dc.radix_select(key, k, one_short=True)
        assert (real <= k) or not np.array_equal(short, got), what


# ---- the recipes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", dc.EXACT_WIDTHS)
@pytest.mark.parametrize("I", dc.SIZES[:7])
def test_exact_recipes_are_exact(E, I):
    r = dc.exact_recipe(E, I)
    S32 = sd.score_matrix(r.PM, r.RE, r.CE, r.cats, r.coef, np.float32)
    assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), r.S, equal_nan=True)
    assert np.isnan(r.S).all(0).sum() == len(dc.nan_dishes(I))
    assert dc.exact_ks(I)[-1] == min(1024, I)
    w, i = dc.key_lists(r.W32, min(1024, I))
    assert (i[:, -1] >= 0).all() and dc.same(dc.model_lists(r.W32, min(1024, I)), (w, i))


def test_the_other_exact_recipes_are_exact():
    for r in (dc.exact_recipe(64, dc.SIZES[7], U=3), dc.tie_recipe(2), dc.tie_recipe(65), dc.tie_recipe(700), dc.nan40_recipe()):
        S32 = sd.score_matrix(r.PM, r.RE, r.CE, r.cats, r.coef, np.float32)
        assert np.array_equal(S32.astype(np.float64), r.S, equal_nan=True)
    r = dc.neighbour_recipe()
    S32 = sd.score_matrix(r.PM, r.RE, r.CE, r.cats, r.coef, np.float32)
    assert np.array_equal(S32, r.W32)


def test_conditions_the_gpu_cases_rely_on():
    for g in dc.TIE_GROUPS:                                  # a tie group really straddles k, and its survivors are the lowest ids
        r = dc.tie_recipe(g)
        assert len(r.copies) == g
        for j in range(len(r.users)):
            assert dc.straddles(r.W32[j], r.k[j]), (g, j)
            w, i = dc.key_lists(r.W32[j:j + 1], r.k[j])
            tied = i[0][w[0] == w[0, -1]]
            rest = np.setdiff1d(np.flatnonzero(dc.words(r.W32[j]) == w[0, -1]), tied)
            assert rest.size and tied.max() < rest.min(), (g, j)
    r = dc.neighbour_recipe()
    w, i = dc.key_lists(r.W32, r.k + 1)
    assert abs(int(w[0, r.k - 1]) - int(w[0, r.k])) == 1      # neighbouring floats around the k-th
    assert np.array_equal(i[1], np.arange(r.k + 1))           # the all-zero user: ids 0 .. k - 1
    r = dc.nan40_recipe()
    w, i = dc.key_lists(r.W32, r.k)
    assert np.isnan(w.view(np.float32)[:, 10:]).all() and np.array_equal(i[:, 10:], np.broadcast_to(r.nan[:25], (r.U, 25)))
    # too few: the segment of I - 5 ids leaves fewer than k
    lists = dc.segment_lists(1300, 14)
    assert [len(set(x)) for x in lists[:7]] == [0, 1, 63, 64, 65, 300, 1295] and all(x == sorted(x) for x in lists)
    assert any(len(x) != len(set(x)) for x in lists)          # with repeats
    # the ranges: listed and excluded dishes on both sides of every edge
    for case in ("exact1300", "normal5000"):
        r = dc.range_recipe(case)
        assert len(r.edges) == (r.I - 1) // 256 and dc.boundary_condition(dc.key_lists(r.W32, 1024, r.lists)[1], r.lists, r.edges), case
        S32 = sd.score_matrix(r.PM, r.RE, r.CE, r.cats, r.coef, np.float32)
        assert case != "exact1300" or np.array_equal(S32.astype(np.float64), r.S, equal_nan=True)
    # both signs and zeros among the exact scores
    r = dc.exact_recipe(4, 1300)
    assert (r.W32 > 0).any() and (r.W32 < 0).any() and (r.W32 == 0).any()


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
def _aimed_cases():
    """(name, W32, k, lists, range width) -- and the stand-ins aimed at each"""
    r = dc.exact_recipe(64, 1300)
    lists = dc.segment_lists(r.I, len(r.users), best=dc.key_lists(r.W32, 2)[1])
    yield "ranges", r.W32, 300, None, 256, ("forget", "nan_first", "one_short")
    yield "exclusions", r.W32, 300, lists, 256, ("strike_after", "forget", "one_short")
    for g in dc.TIE_GROUPS:
        t = dc.tie_recipe(g)
        yield "ties %d" % g, t.W32[:1], t.k[0], None, 1300, ("higher_id", "one_short")
    n = dc.nan40_recipe()
    yield "nan40", n.W32, n.k, None, 40, ("nan_first", "higher_id", "one_short")
    z = dc.neighbour_recipe()
    yield "equal row", z.W32[1:], z.k, None, 256, ("higher_id", "forget", "one_short")


def test_wrong_kernel_standins_change_every_case_aimed_at_them():
    aimed = set()
    for name, W32, k, lists, W, standins in _aimed_cases():
        want = dc.key_lists(W32, k, lists)
        assert dc.same(dc.model_lists(W32, k, lists, W), want), name
        for s in standins:
            assert not dc.same(dc.model_lists(W32, k, lists, W, standin=s), want), (name, s)
            aimed.add(s)
    assert aimed == set(dc.STANDINS)
