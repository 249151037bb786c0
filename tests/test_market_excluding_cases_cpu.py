"""CPU checks of the excluding market-request tests (tests/test_gpu_market_excluding.py): the new symbol at the boundary, the fake
kernel's shapes, the exactness of the one new recipe, the conditions the GPU cases rely on, and the comparison against stand-ins for
what a subtly wrong kernel would return -- each stand-in must change the answer of every case aimed at it."""
import inspect
import os

import numpy as np
import pytest

import market_cases as mc
import market_excluding_cases as mx
import market_request_cases as mq
import seen_dish_cases as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _squeeze(text):
    return " ".join(text.split())


def test_symbol_is_declared_in_the_header_and_the_ctypes_table():
    import ctypes as c
    from foodrec_amd import _native
    header = _squeeze(open(os.path.join(ROOT, "include", "m2d.h")).read())
    assert "int m2d_topk_markets_excluding(m2d_engine *h, const int32_t *users" in header
    assert "int32_t *out_missing /* device, [nQ, k, max_missing], may be null */, void *stream);" in header
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_topk_markets_excluding"] == (c.c_int, [vp, vp, i64, vp, vp, i64, vp, vp, i32, i32, vp, vp, vp, vp, vp])
    assert _native.ABI_VERSION == 2 and _native.lib().m2d_abi_version() == 2
    assert hasattr(_native.lib(), "m2d_topk_markets_excluding")
    src = _squeeze(open(os.path.join(ROOT, "foodrec_amd", "csrc", "m2d_market_requests.hip")).read())
    assert "template <bool LDS, bool EXCL = false> __global__ __launch_bounds__(256) void m2d_markets_topk(MarketsArgs p)" in src
    assert "m2d_markets_topk<true>" in src and "m2d_markets_topk<false>" in src                 # the two old instantiations, as they were
    assert "template <bool LDS> __global__ __launch_bounds__(256) void m2d_markets_missing(" in src


def test_python_surface_and_the_registered_op():
    import torch
    from foodrec_amd import ops, recommender
    p = inspect.signature(ops.ScoringEngine.topk_markets_excluding).parameters
    assert list(p) == ["self", "users", "markets", "exclude", "k", "max_missing", "return_counts", "return_missing"]
    assert (p["exclude"].default, p["k"].default, p["max_missing"].default, p["return_counts"].default, p["return_missing"].default) == (None, 10, 0, False, False)
    p = inspect.signature(recommender.Model.topk_markets_excluding).parameters
    assert list(p) == ["self", "users", "markets", "exclude", "k", "max_missing", "missing"] and p["missing"].default is False
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        users = torch.empty(5, dtype=torch.int32)
        off, ids = torch.empty(6, dtype=torch.int64), torch.empty(17, dtype=torch.int32)
        xoff, xids = torch.empty(6, dtype=torch.int64), torch.empty(9, dtype=torch.int32)
        for mm, ex in ((0, (None, None)), (3, (xoff, xids))):
            s, i, c, m = torch.ops.m2d.topk_markets_excluding(1, users, off, ids, ex[0], ex[1], 7, mm)
            assert (tuple(s.shape), s.dtype) == ((5, 7), torch.float32)
            assert (tuple(i.shape), i.dtype) == ((5, 7), torch.int32)
            assert (tuple(c.shape), c.dtype) == ((5,), torch.int32)
            assert (tuple(m.shape), m.dtype) == ((5, 7, mm), torch.int32)


def test_float32_equals_float64_on_the_new_recipe():
    c = mx.missing_case()
    s32 = sd.score_matrix(c.PM, c.RE, c.CE, c.cats, c.coef, np.float32)
    assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), c.S, equal_nan=True)


def test_without_exclusions_the_restatement_is_market_requests():
    c = mq.catalogue_case(257)
    for excl in (None, [()] * 8):
        assert mq.same_answer(mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, excl, 1, 10),
                              mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 1, 10))


# ---- the conditions the GPU cases rely on ------------------------------------------------------------------------------------------------
def test_exclusion_kinds_are_what_they_say():
    c = mq.catalogue_case(773)
    base = mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, 10)
    # "best": the first listed dish is excluded in every request that lists one, and the second moves up
    got = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, mx.exclusions(773, "best"), 0, 10)
    listed = base[2] > 0
    assert listed.sum() >= 5 and all(base[1][q, 0] in mx.exclusions(773, "best")[q] for q in np.flatnonzero(listed))
    assert np.array_equal(got[1][listed, 0], base[1][listed, 1]) and np.array_equal(got[2][listed], base[2][listed] - 1)
    # its second id is not cookable: alone it has no effect
    alone = [x[-1:] for x in mx.exclusions(773, "best")]
    assert all(len(x) == 1 for x in alone) and mq.same_answer(mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, alone, 0, 10), base)
    # "all": nothing left, at every tolerance up to 2
    for mm in (0, 1, 2):
        s, i, n = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, mx.exclusions(773, "all"), mm, 10)
        assert (n == 0).all() and (i == -1).all() and np.isnan(s).all()
    assert max(len(x) for x in mx.exclusions(773, "all")) > 300
    # "few": at most three left where there were more than k
    n = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, mx.exclusions(773, "few"), 0, 10)[2]
    assert (n <= 3).all() and (n[base[2] > 10] == 3).all() and (base[2] > 10).sum() >= 3
    # "mixed": the segment lengths, an empty first and an empty last segment
    assert tuple(len(x) for x in mx.exclusions(773, "mixed")) == (0, 1, 63, 64, 65, 300, 40, 0)
    # the C ABI's arrays: ascending, with repeats when asked for
    off, ids = mx.csr(mx.exclusions(773, "mixed"), repeats=True)
    assert off[0] == off[1] == 0 and off[-1] == off[-2] == len(ids) and all(np.all(np.diff(ids[off[q]:off[q + 1]]) >= 0) for q in range(8))
    assert any(np.any(np.diff(ids[off[q]:off[q + 1]]) == 0) for q in range(8))


def test_edge_ids_are_cookable_where_they_are_excluded():
    for n in mq.CATALOGUES:
        c = mx.edge_case(n)
        assert set(c.excl[0].tolist()) == {d for d in mx.EDGE_IDS + (n - 1,) if d < n} and set(c.excl[0].tolist()) <= set(c.excl[1].tolist())
        for q in (0, 1):
            assert len(mc.restate(c.off, c.ids, c.R, c.markets[q], 0)[0]) == n                 # every dish, the edge ids among them
        want = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, c.excl, 0, 64)
        assert want[2][0] == n - len(c.excl[0]) and want[2][1] == n - len(c.excl[1])
        assert not set(want[1][0].tolist()) & set(c.excl[0].tolist())
    s32 = sd.score_matrix(c.PM, c.RE, c.CE, c.cats, c.coef, np.float32)
    assert np.array_equal(s32.astype(np.float64), c.S, equal_nan=True)


def test_share_exclusions_sit_on_both_sides_of_every_boundary():
    c = mq.share_case("773")
    for S in (2, 3, 4):
        for b, e in mq.share_bounds(c.I, S)[:-1]:
            assert all({e - 1, e} <= set(x.tolist()) for x in mx.share_exclusions())
    want = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, mx.share_exclusions(), 0, 10)
    assert not mq.same_answer(want, mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, 10))


def test_the_host_workaround_is_wrong_on_the_history_case():
    c, excl, k = mq.composed_case(64), mx.history_exclusions(), mx.HISTORY_K
    right = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, excl, 0, k)
    ws, wi = mx.host_workaround(c, excl, k)
    wrong = [q for q in range(len(c.users)) if not np.array_equal(wi[q], right[1][q])]
    assert mx.HISTORY > 64 - k and len(wrong) >= 30 and 50 in wrong
    assert (wi[50] >= 0).sum() == 64 - mx.HISTORY and (right[1][50] >= 0).all()
    for q in range(len(c.users)):
        if q not in wrong:                                   # right only where the request has nothing beyond its first 64
            assert c.counts[q] <= 64


def test_missing_layout_is_what_it_says():
    c = mx.missing_case()
    assert c.I > mq.DW
    for d, (n, absent) in mx.LAYOUT.items():
        seg = c.ids[c.off[d]:c.off[d + 1]]
        assert len(seg) == n and [p for p in range(n) if seg[p] % 2] == sorted(absent) and all(seg[p] == v for p, v in absent.items())
    lens = {mx.LAYOUT[d][0] for d in mx.LAYOUT}
    assert {63, 64, 65, 193} <= lens
    pos = {p for d in mx.LAYOUT for p in mx.LAYOUT[d][1]}
    assert {0, 63, 64, 192, 62} <= pos
    # at max_missing = 3 every LAYOUT dish is listed for user 0 at k = 64, rows are shorter than k at the empty market
    s, i, n = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, c.excl, 3, 64)
    assert set(mx.LAYOUT) <= set(i[0].tolist()) and 0 < n[4] < 64 and n[3] == c.I - 2
    m = mx.restate_missing(c.off, c.ids, c.R, c.markets, i, 3)
    row = {int(d): m[0, j] for j, d in enumerate(i[0]) if d >= 0}
    assert row[4].tolist() == [11, 1, 3] and row[5].tolist() == [13, 5, 1] and row[6].tolist() == [21, 21, -1] and row[7].tolist() == [15, 15, -1]
    assert row[8].tolist() == [-1, -1, -1] and (m[3] == -1).all() and (m[4][i[4] >= 0][:, 0] >= 0).all()
    # the count of non-negative entries is market_cases.restate's missing count
    for q in range(len(c.users)):
        miss = mc.restate(c.off, c.ids, c.R, c.markets[q], 3)[1]
        for j, d in enumerate(i[q]):
            assert (m[q, j] >= 0).sum() == (miss[d] if d >= 0 else 0)


# ---- the stand-ins: each changes the answer of every GPU case aimed at it ------------------------------------------------------------------
def _both(c, excl, mm, k, standin, shares=1):
    args = (c.S, c.users, c.off, c.ids, c.R, c.markets, excl, mm, k)
    return mx.restate(*args), mx.restate(*args, standin=standin, shares=shares)


def test_first_for_all_changes_every_case_with_different_lists():
    for n in mq.CATALOGUES[4:]:
        for kind in ("best", "few", "mixed"):
            assert not mq.same_answer(*_both(mq.catalogue_case(n), mx.exclusions(n, kind), 0, 10, "first_for_all")), (n, kind)
    for E in mq.COMPOSED_WIDTHS:
        assert not mq.same_answer(*_both(mq.composed_case(E), mx.composed_exclusions(E), 0, 10, "first_for_all"))
    assert not mq.same_answer(*_both(mq.composed_case(64), mx.history_exclusions(), 0, 10, "first_for_all"))


def test_last_share_unfiltered_changes_the_share_case():
    c = mq.share_case("773")
    for S in (2, 3, 4):
        for k in (10, 64):
            assert not mq.same_answer(*_both(c, mx.share_exclusions(), 0, k, "last_share_unfiltered", S)), (S, k)


def test_excluded_counted_changes_every_case_that_excludes_a_cookable_dish():
    for n in mq.CATALOGUES[4:]:
        for kind in ("best", "all", "few"):
            assert not mq.same_answer(*_both(mq.catalogue_case(n), mx.exclusions(n, kind), 0, 10, "excluded_counted")), (n, kind)
    for n in mq.CATALOGUES:
        assert not mq.same_answer(*_both(mx.edge_case(n), mx.edge_case(n).excl, 0, 10, "excluded_counted")), n
    assert not mq.same_answer(*_both(mq.share_case("773"), mx.share_exclusions(), 0, 10, "excluded_counted"))
    assert not mq.same_answer(*_both(mq.composed_case(64), mx.history_exclusions(), 0, 10, "excluded_counted"))


def test_window_last_missed_changes_every_case_aimed_at_it():
    for n in mq.CATALOGUES[4:]:
        for kind in ("all", "few"):
            assert not mq.same_answer(*_both(mq.catalogue_case(n), mx.exclusions(n, kind), 0, 64, "window_last_missed")), (n, kind)
    for n in mq.CATALOGUES:
        assert not mq.same_answer(*_both(mx.edge_case(n), mx.edge_case(n).excl, 0, 64, "window_last_missed")), n
    assert not mq.same_answer(*_both(mq.share_case("773"), mx.share_exclusions(), 0, 64, "window_last_missed"))
    assert not mq.same_answer(*_both(mq.composed_case(64), mx.history_exclusions(), 0, 10, "window_last_missed"))


@pytest.mark.parametrize("standin", mx.MISSING_STANDINS)
def test_missing_standins_change_the_layout_case(standin):
    c = mx.missing_case()
    for mm in (2, 3):
        i = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, c.excl, mm, 64)[1]
        assert not mx.same_missing(mx.restate_missing(c.off, c.ids, c.R, c.markets, i, mm), mx.restate_missing(c.off, c.ids, c.R, c.markets, i, mm, standin)), mm
