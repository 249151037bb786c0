"""CPU checks of the market-request tests (tests/test_gpu_market_requests.py): the new symbol at the boundary, the kernel's constants
restated in tests/market_request_cases.py against their source lines, the exactness of every exact recipe, the conditions the GPU cases
rely on, and the comparison against stand-ins for what a subtly wrong kernel would return -- each stand-in must change the answer of
every case aimed at it."""
import inspect
import os

import numpy as np
import pytest

import market_cases as mc
import market_request_cases as mq
import seen_dish_cases as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _squeeze(text):
    return " ".join(text.split())


def test_symbol_is_declared_in_the_header_and_the_ctypes_table():
    import ctypes as c
    from foodrec_amd import _native
    header = _squeeze(open(os.path.join(ROOT, "include", "m2d.h")).read())
    assert "int m2d_topk_markets(m2d_engine *h, const int32_t *users" in header
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_topk_markets"] == (c.c_int, [vp, vp, i64, vp, vp, i64, i32, i32, vp, vp, vp, vp])
    assert _native.ABI_VERSION == 2 and _native.lib().m2d_abi_version() == 2
    assert "THE CALL NEVER SYNCHRONISES" in header
    assert "m2d_market_requests.hip" in open(os.path.join(ROOT, "foodrec_amd", "csrc", "Makefile")).read()
    for option in ("market_shares ", "market_shares_used "):
        assert " * " + option in header, option


def test_python_surface_and_the_registered_op():
    import torch
    from foodrec_amd import ops, recommender
    eng, model = ops.ScoringEngine, recommender.Model
    assert list(inspect.signature(eng.topk_markets).parameters) == ["self", "users", "markets", "k", "max_missing", "return_counts"]
    p = inspect.signature(model.topk_markets).parameters
    assert list(p) == ["self", "users", "markets", "k", "max_missing"] and p["k"].default == 10 and p["max_missing"].default == 0
    assert list(inspect.signature(model.topk).parameters)[:8] == ["self", "users", "k", "exclude", "head", "candidates", "among", "market"]
    assert hasattr(torch.ops.m2d, "topk_markets") and "fake kernel" in inspect.getsource(ops).split('"m2d::topk_markets"')[1]
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        users = torch.empty(5, dtype=torch.int32)
        off, ids = torch.empty(6, dtype=torch.int64), torch.empty(17, dtype=torch.int32)
        s, i, c = torch.ops.m2d.topk_markets(1, users, off, ids, 7, 0)
    assert (tuple(s.shape), s.dtype) == ((5, 7), torch.float32)
    assert (tuple(i.shape), i.dtype) == ((5, 7), torch.int32)
    assert (tuple(c.shape), c.dtype) == ((5,), torch.int32)


def test_restated_constants_match_their_source_lines():
    src = _squeeze(open(os.path.join(ROOT, "foodrec_amd", "csrc", "m2d_market_requests.hip")).read())
    for line in ("constexpr int MQ_DW = %d;" % mq.DW,
                 "constexpr int MQ_WAVES = %d;" % mq.WAVES,
                 "constexpr int MQ_DB = MQ_DW * MQ_WAVES;",
                 "constexpr int MQ_EB = %d;" % mq.EB,
                 "constexpr int MQ_BF = %d;" % mq.BF,
                 "constexpr int MQ_LDS_BITS = 1 << 16;",
                 "constexpr int MQ_KMAX = %d;" % mq.KMAX,
                 "constexpr int MQ_MAX_SHARES = %d;" % mq.MAX_SHARES,
                 "const bool lds = R <= MQ_LDS_BITS;",
                 'h->last_kernel = lds ? "%s" : "%s";' % (mq.TOPK_LDS, mq.TOPK_L2),
                 "int64_t S = h->opt_market_shares > 0 ? h->opt_market_shares : 4 * (int64_t)h->num_cu / nQ;",
                 "const int64_t smax = nb < MQ_MAX_SHARES ? nb : MQ_MAX_SHARES;",
                 "const int64_t b0 = (int64_t)s * nb / S, b1 = (int64_t)(s + 1) * nb / S;"):
        assert line in src, line
    assert (mq.DW, mq.WAVES, mq.DB, mq.EB, mq.LB) == (mc.DW, mc.WAVES, mc.DB, mc.EB, mc.LB)      # the walk is m2d_market_flag's
    engine = _squeeze(open(os.path.join(ROOT, "foodrec_amd", "csrc", "m2d_engine.h")).read())
    assert "constexpr uint64_t TKM_NONE = ~0ull;" in engine and "uint64_t tkm_key(const float s, const int32_t id)" in engine
    for name in ("m2d_topk_mlp.hip", "m2d_select.hip", "m2d_select.h"):                              # one definition
        select = _squeeze(open(os.path.join(ROOT, "foodrec_amd", "csrc", name)).read())
        assert "constexpr uint64_t TKM_NONE" not in select and "uint64_t tkm_key(" not in select, name


def test_share_rule():
    assert mq.shares_used(0, 1, 256, 773) == 4 and mq.shares_used(0, 1, 256, 10 ** 6) == 64 and mq.shares_used(0, 1025, 256, 10 ** 6) == 1
    assert mq.shares_used(0, 16, 256, 10 ** 6) == 64 and mq.shares_used(0, 100, 256, 10 ** 6) == 10 and mq.shares_used(64, 7, 256, 600) == 3
    assert mq.share_bounds(773, 4) == [(0, 256), (256, 512), (512, 768), (768, 773)]
    assert mq.share_bounds(773, 3) == [(0, 256), (256, 512), (512, 773)]
    assert mq.share_bounds(773, 64) == mq.share_bounds(773, 4) and mq.share_bounds(600, 2) == [(0, 256), (256, 600)]
    for n in (1, 255, 256, 257, 600, 773, 5000):
        for S in mq.SHARES:
            b = mq.share_bounds(n, S)
            assert b[0][0] == 0 and b[-1][1] == n and all(x[1] == y[0] for x, y in zip(b, b[1:])) and all(e > s for s, e in b)


# ---- exactness: float32 equals float64 on every exact recipe the GPU file uses ---------------------------------------------------------
def _exact_cases():
    return ([("catalogue %d" % n, mq.catalogue_case(n)) for n in mq.CATALOGUES] + [("bitmap %d" % R, mq.bitmap_case(R)) for R in mc.BITMAP_ROWS]
            + [("composed %d" % E, mq.composed_case(E)) for E in mq.COMPOSED_WIDTHS] + [("share " + w, mq.share_case(w)) for w in ("773", "600", "hollow", "last wave")]
            + [("other shape", mq.other_shape_case())])


def test_float32_equals_float64_on_every_exact_recipe():
    for name, c in _exact_cases():
        users = np.unique(c.users)
        s32 = sd.score_matrix(c.PM, c.RE, c.CE, c.cats, c.coef, np.float32, users=users)
        s64 = c.S[users]
        assert s32.dtype == np.float32 and np.array_equal(s32.astype(np.float64), s64, equal_nan=True), name


def test_the_two_statements_of_the_order_agree():
    c = mq.composed_case(64)
    for k in mq.COMPOSED_KS:
        a = mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, k)
        assert mq.same_answer(a, mq.restate_with_exact_lists(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, k))


# ---- the conditions the GPU cases rely on ------------------------------------------------------------------------------------------------
def test_catalogue_cases_exceed_every_k_and_fall_short_of_it():
    for n, want in ((257, (98, 131, 167, 189)), (773, (356, 499, 612, 705))):
        c = mq.catalogue_case(n)
        got = tuple(len(mc.restate(c.off, c.ids, c.R, c.markets[0], mm)[0]) for mm in c.tolerances)
        assert got == want, (n, got)
    c = mq.catalogue_case(773)
    short = [len(mc.restate(c.off, c.ids, c.R, m, 0)[0]) for m in c.markets[2:5]]
    assert short[0] == 0 and max(short) <= 3, short


def test_composed_counts():
    c = mq.composed_case(64)
    assert tuple(c.counts[:10]) == (0, 0, 3, 7, 7, 7, 11, 13, 18, 25) and c.counts[50] == 590 and np.all(np.diff(c.counts[:51]) >= 0)
    assert 56 in c.counts and 65 in c.counts
    assert [m for m in range(51) if c.counts[m] == 7] == [3, 4, 5]                              # count = k at k = 7
    assert any(c.counts[m] == k + 1 for m in range(51) for k in mq.COMPOSED_KS)
    # cookable empty-mask dishes are listed last in id order wherever the list reaches them
    s, i, n = mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, 64)
    seen = 0
    for m in range(51):
        if c.counts[m] <= 64:
            empty = sorted(set(sd.LAUNCH_EMPTY) & set(i[m][:c.counts[m]].tolist()))
            seen = max(seen, len(empty))
            assert i[m][c.counts[m] - len(empty):c.counts[m]].tolist() == empty and np.isnan(s[m][c.counts[m] - len(empty):c.counts[m]]).all()
            assert not np.isnan(s[m][:c.counts[m] - len(empty)]).any()
    assert seen >= 1 and set(sd.LAUNCH_EMPTY) <= set(mc.restate(c.off, c.ids, c.R, c.markets[50], 0)[0].tolist())
    # the same user under two markets, one market under two users
    assert c.users[51] == c.users[3] and len(c.markets[51]) != len(c.markets[3])
    assert len(c.markets[52]) == len(c.markets[3]) and c.users[52] != c.users[3]


@pytest.mark.parametrize("which", ("773", "600"))
def test_equal_keys_straddle_every_share_boundary(which):
    c = mq.share_case(which)
    for S in (2, 3, 4):
        if len(mq.share_bounds(c.I, S)) < 2:
            continue
        for q, u in enumerate(c.users):
            cook = mc.restate(c.off, c.ids, c.R, c.markets[q], c.max_missing)[0]
            assert mq.straddling_ties(c.S, u, cook, 64, S, c.I), "%s: no straddling tie for user %d at %d shares" % (which, u, S)


def test_hollow_and_last_wave_shares():
    c = mq.share_case("hollow")
    cook = mc.restate(c.off, c.ids, c.R, c.markets[0], 0)[0]
    b = mq.share_bounds(c.I, 3)
    assert len(b) == 3 and not ((cook >= b[1][0]) & (cook < b[1][1])).any() and (cook < b[0][1]).any() and (cook >= b[2][0]).any()
    c = mq.share_case("last wave")
    cook = mc.restate(c.off, c.ids, c.R, c.markets[0], 0)[0]
    assert len(cook) and cook.min() >= mq.share_bounds(c.I, 2)[1][0]


# ---- the stand-ins: each changes the answer of every GPU case aimed at it ------------------------------------------------------------------
def _answers(c, mm, k, standin, shares=1):
    users = c.users
    return (mq.restate(c.S, users, c.off, c.ids, c.R, c.markets, mm, k), mq.restate(c.S, users, c.off, c.ids, c.R, c.markets, mm, k, standin, shares))


def test_shared_bitmap_changes_every_multi_market_case():
    for n in mq.CATALOGUES:
        if n == 1:                                                # one empty dish: every market answers alike (the case checks counts of 0)
            continue
        c = mq.catalogue_case(n)
        for mm in c.tolerances[:3]:
            assert not mq.same_answer(*_answers(c, mm, 10, "shared_bitmap")), (n, mm)
    for R in mc.BITMAP_ROWS:
        assert not mq.same_answer(*_answers(mq.bitmap_case(R), 0, 10, "shared_bitmap")), R
    for E in mq.COMPOSED_WIDTHS:
        assert not mq.same_answer(*_answers(mq.composed_case(E), 0, 10, "shared_bitmap"))
    assert not mq.same_answer(*_answers(mq.other_shape_case(), 0, 10, "shared_bitmap"))


def test_count_listed_changes_every_case_with_more_than_k():
    for n in mq.CATALOGUES[4:]:
        c = mq.catalogue_case(n)
        for k in mq.KS:
            assert not mq.same_answer(*_answers(c, 0, k, "count_listed")), (n, k)
    for k in mq.COMPOSED_KS:
        assert not mq.same_answer(*_answers(mq.composed_case(64), 0, k, "count_listed"))


@pytest.mark.parametrize("which", ("773", "600"))
def test_share_standins_change_the_share_cases(which):
    c = mq.share_case(which)
    for S in (2, 3, 4):
        if len(mq.share_bounds(c.I, S)) < S:
            continue
        for standin in ("tie_to_higher_share", "drop_last_share"):
            a, b = _answers(c, c.max_missing, 64, standin, S)
            assert not mq.same_answer(a, b), (which, S, standin)
            if standin == "tie_to_higher_share":                 # every row of the call holds such a tie
                assert all(not np.array_equal(a[1][q], b[1][q]) for q in range(len(c.users))), (which, S, standin)


def test_drop_last_share_changes_the_last_wave_case_and_nan_first_the_composed_ones():
    c = mq.share_case("last wave")
    assert not mq.same_answer(*_answers(c, 0, 10, "drop_last_share", 2))
    for E in mq.COMPOSED_WIDTHS:
        assert not mq.same_answer(*_answers(mq.composed_case(E), 0, 64, "nan_ranked_first"))
    n = mq.normal_case()
    assert len(n.markets) == 64 and all(len(m) for m in n.markets)
