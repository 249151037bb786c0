"""GPU tests of the deep retrieval lists (m2d_topk_users_deep, m2d_topk_users_mlp_deep; DESIGN.md sections 4.11, 8.8): against the
calls that exist for k <= 64, against the float64 restatement on exact tables up to k = 1 024, against the key rule over the engine's
own score words on normal tables, ties and digits, dish ranges, exclusions, the two-stage form, errors and refusals, and what stands
around the calls.  No comparison has a tolerance: ids as integers, scores as 32-bit words.  The calls go through the C ABI into
poisoned [nU, k] buffers with a guard row on either side.  Inputs and restatements: tests/deep_cases.py."""
import ctypes

import numpy as np
import pytest

import deep_cases as dc
import seen_dish_cases as sd
import slate_cases as sc
from helpers import mlp_head

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN no kernel computes; as an id: no dish


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(r, head=None, user_base=0, masks=True, tables=None):
    from foodrec_amd import ScoringEngine
    PM, RE, CE = tables if tables is not None else (r.PM, r.RE, r.CE)
    eng = ScoringEngine(PM, RE, CE, coef=r.coef, user_base=user_base)
    if masks:
        eng.set_dish_categories(r.cats)
    if head is not None:
        eng.set_mlp_head(*head)
    return eng


def _abi(eng, users, k, off=None, ids=None, candidates=None, null=()):
    """one call through the C ABI -> (status, score words uint32 [nU, k], ids int64 [nU, k]); the guard rows checked"""
    import torch
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    users = _dev(np.asarray(users, np.int32))
    nU, kk = users.numel(), max(int(k), 1)
    bs = torch.full(((nU + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    bi = torch.full(((nU + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    xo = _dev(np.asarray(off, np.int64)) if off is not None else None
    xi = _dev(np.asarray(ids, np.int32)) if ids is not None else None
    ptr = lambda t, name, shift=0: None if t is None or name in null else t.data_ptr() + shift      # noqa: E731
    args = [eng._h, ptr(users, "users"), nU, int(k)] + ([] if candidates is None else [int(candidates)])
    args += [ptr(xo, "off"), ptr(xi, "ids"), ptr(bs, "scores", 4 * kk), ptr(bi, "out_ids", 4 * kk), _stream_ptr()]
    fn = _native.lib().m2d_topk_users_deep if candidates is None else _native.lib().m2d_topk_users_mlp_deep
    rc = fn(*args)
    torch.cuda.synchronize()
    s, i = bs.cpu().numpy().view(np.uint32).reshape(nU + 2, kk), bi.cpu().numpy().reshape(nU + 2, kk)
    assert (s[[0, -1]] == POISON).all() and (i[[0, -1]] == POISON).all(), "a guard row was written"
    return rc, s[1:-1], i[1:-1].astype(np.int64)


def _deep(eng, users, k, lists=None, candidates=None):
    """the lists of a call that must succeed: every element written, the id latch clear"""
    off, ids = dc.csr(lists) if lists is not None else (None, None)
    rc, s, i = _abi(eng, users, k, off, ids, candidates)
    assert rc == 0, eng_error(eng)
    eng.check()
    assert (i != POISON).all() and (s != POISON).all(), "%d elements not written" % int((i == POISON).sum())
    return s, i


def eng_error(eng):
    from foodrec_amd import _native
    return (_native.lib().m2d_last_error(eng._h) or b"").decode()


def _latched(eng):
    """(code, value, index) of m2d_check"""
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    bv, bi = ctypes.c_int64(), ctypes.c_int64()
    rc = _native.lib().m2d_check(eng._h, _stream_ptr(), ctypes.byref(bv), ctypes.byref(bi))
    return rc, bv.value, bi.value


def _slate_matrix(eng, users, I):
    out = eng.score_slate(_dev(np.asarray(users, np.int32)), _dev(np.arange(I, dtype=np.int32)))
    eng.check()
    return out.cpu().numpy()


def _head_matrix(eng, users, I):
    users = np.asarray(users, np.int32)
    out = eng.score_pairs_mlp(_dev(np.repeat(users, I)), _dev(np.tile(np.arange(I, dtype=np.int32), users.size)))
    eng.check()
    return out.cpu().numpy().reshape(users.size, I)


def _assert_same(got, want, what=""):
    gs, gi = got
    ws, wi = want
    assert np.array_equal(np.asarray(gi, np.int64), np.asarray(wi, np.int64)), "%s: ids of %d rows differ" % (
        what, int((np.asarray(gi) != np.asarray(wi)).any(1).sum()))
    assert np.array_equal(np.asarray(gs, np.uint32), np.asarray(ws, np.uint32)), "%s: score words differ" % what


def _t(x):
    s, i = x
    return dc.words(s.cpu().numpy()), i.cpu().numpy().astype(np.int64)


# ---- 1. against the calls that exist, k <= 64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ("exact", "normal"))
def test_up_to_64_the_lists_are_the_existing_calls(tables):
    r = sd.launch_recipe(64) if tables == "exact" else dc.normal_recipe(64)
    rng = np.random.default_rng(3)
    users = rng.integers(0, r.U, 40).astype(np.int32)
    head = mlp_head(5 * r.E, 256, 64, rng, scale=4.0)
    eng = _engine(r)
    slate = _dev(np.arange(r.I, dtype=np.int32))
    for k in (1, 10, 64):
        want = _t(eng.topk_slate(_dev(users), slate, k))
        _assert_same(_deep(eng, users, k), want, "%s, k = %d" % (tables, k))
    eng.set_mlp_head(*head)
    lists = dc.segment_lists(r.I, len(users), best=dc.key_lists(_head_matrix(eng, users, r.I), 2)[1])
    for k in (1, 10, 64):
        for x in (None, lists):
            want = _t(eng.topk_users_mlp_excluding(_dev(users), k, None if x is None else tuple(map(_dev, dc.csr(x))), 0))
            eng.check()
            _assert_same(_deep(eng, users, k, x, candidates=0), want, "%s, head, k = %d, exclusions %s" % (tables, k, x is not None))
    eng.close()


# ---- 2. beyond 64, exact tables --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", dc.EXACT_WIDTHS)
@pytest.mark.parametrize("I", dc.SIZES)
def test_exact_tables_equal_the_float64_restatement(E, I):
    r = dc.exact_recipe(E, I, U=3 if I > 2000 else 6)
    eng = _engine(r)
    matrix = _slate_matrix(eng, r.users, I)
    assert np.isnan(matrix).all(0).sum() == len(dc.nan_dishes(I))
    for k in dc.exact_ks(I):
        s, i = _deep(eng, r.users, k)
        ws, wi = sc.exact_lists(r.S[r.users], np.arange(I), k)
        assert np.array_equal(i, wi), "E = %d, I = %d, k = %d: ids of %d rows differ" % (E, I, k, int((i != wi).any(1).sum()))
        nan = np.isnan(ws)                                   # (a NaN's payload is the engine's own: the matrix comparison below)
        assert np.array_equal(np.isnan(s.view(np.float32)), nan), (E, I, k)
        assert np.array_equal(sc.bits(np.where(nan, 0, s.view(np.float32))), sc.bits(np.where(nan, 0, ws))), (E, I, k)
        assert np.array_equal(s, dc.words(np.take_along_axis(matrix, i, 1))), "a listed word is not score_slate's"
    eng.close()


# ---- 3. beyond 64, normal tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", (64, 200))
def test_normal_tables_equal_the_key_rule_over_the_engines_words(E):
    r = dc.normal_recipe(E)
    eng = _engine(r)
    matrix = _slate_matrix(eng, r.users, r.I)
    lists = dc.segment_lists(r.I, len(r.users), best=dc.key_lists(matrix, 2)[1])
    for k in (65, 300, 1024):
        _assert_same(_deep(eng, r.users, k), dc.key_lists(matrix, k), "E = %d, k = %d" % (E, k))
        _assert_same(_deep(eng, r.users, k, lists), dc.key_lists(matrix, k, lists), "E = %d, k = %d, exclusions" % (E, k))
    eng.set_mlp_head(*r.head)
    hm = _head_matrix(eng, r.users, r.I)
    assert np.unique(dc.words(hm)).size > hm.size // 2
    for k in (65, 1024):
        _assert_same(_deep(eng, r.users, k, candidates=0), dc.key_lists(hm, k), "E = %d, head, k = %d" % (E, k))
        _assert_same(_deep(eng, r.users, k, lists, candidates=0), dc.key_lists(hm, k, lists), "E = %d, head, k = %d, exclusions" % (E, k))
    _assert_same(_deep(eng, r.users, 300), dc.key_lists(matrix, 300), "the catalogue call ignores the head")
    eng.close()


# ---- 4. ties and digits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", dc.TIE_GROUPS)
def test_a_tie_group_across_position_k_keeps_its_lowest_ids(group):
    r = dc.tie_recipe(group)
    eng = _engine(r)
    for P in (256, dc.DEFAULT_P):                            # the copies in several ranges, and in one
        eng.set_option("deep_chunk_pairs", P)
        for j, u in enumerate(r.users):
            k = r.k[j]
            s, i = _deep(eng, [u], k)
            _assert_same((s, i), dc.key_lists(r.W32[j:j + 1], k), "group of %d, user %d, k = %d" % (group, u, k))
            kept = np.isin(r.copies, i[0])                   # the group straddles k: part of it is listed, and that part is its lowest ids
            assert 0 < kept.sum() < group and kept[:kept.sum()].all(), (group, u, k)
    eng.close()


def test_equal_rows_neighbouring_floats_and_nan_rows():
    r = dc.neighbour_recipe()
    eng = _engine(r)
    for P in (256, dc.DEFAULT_P):
        eng.set_option("deep_chunk_pairs", P)
        for k in (1, r.k, r.I):
            s, i = _deep(eng, r.users, k)
            _assert_same((s, i), dc.key_lists(r.W32, k), "neighbouring floats / the all-zero user, k = %d" % k)
            assert np.array_equal(i[1], np.arange(k))        # every score equal: ids 0 .. k - 1
    # a head whose last bias is +inf: every score +inf
    h = list(mlp_head(5 * r.E, 256, 64, np.random.default_rng(1)))
    h[5] = float("inf")
    eng.set_mlp_head(*h)
    hm = _head_matrix(eng, r.users, r.I)
    assert np.isposinf(hm).all()
    for k in (70, r.I):
        s, i = _deep(eng, r.users, k, candidates=0)
        assert np.array_equal(i, np.broadcast_to(np.arange(k), i.shape)) and (s == 0x7F800000).all()
    eng.close()
    n = dc.nan40_recipe()
    eng = _engine(n)
    s, i = _deep(eng, n.users, n.k)
    ws, wi = dc.key_lists(n.W32, n.k)
    _assert_same((s[:, :10], i), (ws[:, :10], wi), "30 of 40 NaN")
    assert np.isnan(s.view(np.float32)[:, 10:]).all() and np.array_equal(i[:, 10:], np.broadcast_to(n.nan[:25], (n.U, 25)))
    eng.close()


def test_both_signs_and_zeros_on_exact_tables():
    r = dc.exact_recipe(4, 1300)                              # E = 4: many equal scores, zeros among them
    assert (r.W32 > 0).any() and (r.W32 < 0).any() and (r.W32 == 0).any()
    eng = _engine(r)
    matrix = _slate_matrix(eng, r.users, r.I)
    for k in (300, 1024):
        _assert_same(_deep(eng, r.users, k), dc.key_lists(matrix, k), "k = %d" % k)
    eng.close()


# ---- 5. ranges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("exact1300", "normal5000"))
def test_lists_do_not_depend_on_the_ranges(case):
    r = dc.range_recipe(case)                                # best dishes and excluded ids on both sides of every edge
    k = 1024
    eng = _engine(r, head=dc.normal_recipe(64).head)
    matrix = _slate_matrix_headless(eng, r)
    hm = _head_matrix(eng, r.users, r.I)
    want = wanth = None
    lists, edges = r.lists, r.edges
    for P in (dc.DEFAULT_P, 2048, 256):
        W, _ = dc.ranges(r.I, P)
        eng.set_option("deep_chunk_pairs", P)
        eng.set_option("topk_mlp_chunk_pairs", P)
        assert eng.get_option("deep_chunk_pairs") == P
        got = _deep(eng, r.users, k, lists)
        goth = _deep(eng, r.users, k, lists, candidates=0)
        if want is None:
            want, wanth = got, goth
            _assert_same(got, dc.key_lists(matrix, k, lists), "%s, default ranges" % case)
            _assert_same(goth, dc.key_lists(hm, k, lists), "%s, head, default ranges" % case)
            assert dc.boundary_condition(got[1], lists, edges)
        _assert_same(got, want, "%s, deep_chunk_pairs = %d (W = %d, k = %d)" % (case, P, W, k))
        _assert_same(goth, wanth, "%s, head, topk_mlp_chunk_pairs = %d" % (case, P))
    for bad in (255, (1 << 24) + 1, 0, -1):
        with pytest.raises(ValueError):
            eng.set_option("deep_chunk_pairs", bad)
    assert eng.get_option("deep_chunk_pairs") == 256
    eng.close()


def _slate_matrix_headless(eng, r):
    """score_slate refuses under a head: the matrix from an engine without one"""
    e2 = _engine(r)
    m = _slate_matrix(e2, r.users, r.I)
    e2.close()
    return m


# ---- 6. exclusions -------------------------------------------------------------------------------------------------------------------------
def test_exclusion_segments_of_every_size_repeated_users_and_a_shard():
    r = dc.normal_recipe(64)
    base = 9000
    eng = _engine(r, user_base=base)
    users = np.asarray([2, 2, 2, 2, 2, 2, 2, 5, 5, 5, 5, 5, 5, 5] + list(range(7)), np.int32)     # repeated users, different segments
    matrix = _slate_matrix(eng, users + base, r.I)
    lists = dc.segment_lists(r.I, len(users), seed=1, best=dc.key_lists(matrix, 2)[1])
    assert [len(set(x)) for x in lists[:7]] == [0, 1, 63, 64, 65, 300, r.I - 5]
    for k in (10, 300, 1024):
        s, i = _deep(eng, users + base, k, lists)
        _assert_same((s, i), dc.key_lists(matrix, k, lists), "k = %d" % k)
        if k > 5:                                            # fewer than k left: -1 / NaN from column 5 on
            for j in (6, 13, 20):
                assert (i[j, :5] >= 0).all() and (i[j, 5:] == -1).all() and (s[j, 5:] == dc.NAN_WORD).all()
    eng.close()


# ---- 7. two-stage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K1", (65, 256, 1024))
def test_two_stage_reranks_the_deep_candidates(K1):
    r = dc.normal_recipe(64)
    eng = _engine(r, head=r.head)
    users = r.users
    hm = _head_matrix(eng, users, r.I)
    lists = dc.segment_lists(r.I, len(users), seed=2)
    for P in (dc.DEFAULT_P, 256):
        eng.set_option("deep_chunk_pairs", P)
        eng.set_option("topk_mlp_chunk_pairs", P)
        for x in (None, lists):
            _, cand = _deep(eng, users, K1, x)               # stage 1: the deep catalogue lists for that user and segment
            for k in sorted({10, 65, K1}):
                want_w = np.full((len(users), k), dc.NAN_WORD, np.uint32)
                want_i = np.full((len(users), k), -1, np.int64)
                for j in range(len(users)):
                    c = cand[j][cand[j] >= 0]                # a slot stage 1 left empty is dropped
                    w, i = dc.key_lists(hm[j:j + 1, c], min(k, c.size), ids=c) if c.size else (np.zeros((1, 0), np.uint32), np.zeros((1, 0), np.int64))
                    want_w[j, :w.shape[1]], want_i[j, :i.shape[1]] = w[0], i[0]
                _assert_same(_deep(eng, users, k, x, candidates=K1), (want_w, want_i), "K1 = %d, k = %d, P = %d" % (K1, k, P))
    assert (want_i[6] == -1).sum() == K1 - 5                 # the segment of I - 5 ids: five candidates
    eng.close()


# ---- 8. errors and refusals --------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, I=300, U=8, seed=1)
    eng = _engine(r, head=r.head)
    users = np.arange(4, dtype=np.int32)
    off, ids = dc.csr([[1], [2, 3], [], [7]])
    for cand in (None, 0):
        for k in (0, 1025, r.I + 1, -3):
            assert _abi(eng, users, k, candidates=cand)[0] == _native.M2D_ERR_INVALID_ARG
            assert "1 <= k <= min(1024, I)" in eng_error(eng)
        for null in ("users", "scores", "out_ids"):
            assert _abi(eng, users, 5, candidates=cand, null=(null,))[0] == _native.M2D_ERR_INVALID_ARG
            assert "null buffer" in eng_error(eng)
        assert _abi(eng, users, 5, off, ids, candidates=cand, null=("ids",))[0] == _native.M2D_ERR_INVALID_ARG     # excl_off without excl_ids
        assert _abi(eng, np.zeros(0, np.int32), 5, candidates=cand)[0] == 0          # nU == 0
    for cand in (-1, 4, 301, 1025):                          # k = 5: below k, above I, above 1024
        assert _abi(eng, users, 5, candidates=cand)[0] == _native.M2D_ERR_INVALID_ARG, cand
        assert "candidates must be 0 (exact) or k <= candidates <= min(1024, I)" in eng_error(eng)
    assert _abi(eng, users, 5, candidates=300)[0] == 0
    assert _native.lib().m2d_topk_users_mlp(eng._h, None, 4, 5, 65, None, None, None) == _native.M2D_ERR_INVALID_ARG     # its range is what it was
    with pytest.raises(ValueError, match="1 <= k <= 1024"):
        eng.topk_users_deep(_dev(users), 1025)
    eng.close()
    bare = _engine(r, masks=False)
    assert _abi(bare, users, 5)[0] == _native.M2D_ERR_NOT_CONFIGURED
    bare.set_dish_categories(r.cats)
    for cand in (0, 10):
        assert _abi(bare, users, 5, candidates=cand)[0] == _native.M2D_ERR_NOT_CONFIGURED and "m2d_set_mlp_head" in eng_error(bare)
    bare.close()


def test_refusals_name_the_condition():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, I=300, U=8, seed=1)
    rng = np.random.default_rng(2)
    eng = _engine(r, head=r.head)
    users = np.arange(6, dtype=np.int32)
    want = _deep(eng, users, 100)
    wanth = _deep(eng, users, 100, candidates=0)
    nnz = 3 * r.I
    eng.set_ingredients((rng.standard_normal((50, r.E)) / 8).astype(np.float32), np.arange(0, nnz + 1, 3, dtype=np.int32),
                        rng.integers(0, 50, nnz).astype(np.int32))
    assert _abi(eng, users, 100)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng) == "m2d_topk_users_deep: the ingredient table is set (not supported)"
    assert _abi(eng, users, 100, candidates=100)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng) == "m2d_topk_users_mlp_deep: the ingredient table is set (not supported)"
    s, i = _deep(eng, users, 100, candidates=0)               # the exact head form serves the ingredient table
    _assert_same((s, i), dc.key_lists(_head_matrix(eng, users, r.I), 100), "exact head form, ingredient table")
    eng.clear_ingredients()
    _assert_same(_deep(eng, users, 100), want, "after clear_ingredients")
    keep = eng.re[7, 3].item()
    eng.re[7, 3] = float("inf")
    eng.tables_updated()
    for cand, name in ((None, "m2d_topk_users_deep"), (100, "m2d_topk_users_mlp_deep")):
        assert _abi(eng, users, 100, candidates=cand)[0] == _native.M2D_ERR_UNSUPPORTED
        assert eng_error(eng) == name + ": needs finite tables (a table value is not finite)"
    eng.re[7, 3] = keep
    eng.tables_updated()
    _assert_same(_deep(eng, users, 100), want, "after the value was put back")
    _assert_same(_deep(eng, users, 100, candidates=0), wanth, "head, after the value was put back")
    eng.close()


def test_bad_ids_are_latched_with_value_and_position():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, I=300, U=8, seed=1)
    eng = _engine(r, head=r.head, user_base=100)
    users = (np.arange(12) % r.U + 100).astype(np.int32)
    good = [[1, 5], [], [0, 2, 299], [7]] * 3
    off, ids = dc.csr(good)
    want = {c: _deep(eng, users, 70, good, candidates=c) for c in (None, 0, 70)}

    def latched(users_, off_, ids_, cand, code, value, index, P):
        eng.set_option("deep_chunk_pairs", P)
        eng.set_option("topk_mlp_chunk_pairs", P)
        assert _abi(eng, users_, 70, off_, ids_, candidates=cand)[0] == 0
        assert _latched(eng) == (code, value, index), (cand, P, eng_error(eng))
        assert _latched(eng)[0] == 0                         # cleared; the engine is usable and the next call right
        _assert_same(_deep(eng, users, 70, good, candidates=cand), want[cand], "after a latched error")

    for P in (dc.DEFAULT_P, 256):                            # 256: user blocks of one row -- the position is the caller's
        for cand in (None, 70):
            bad_u = users.copy(); bad_u[9] = 100 + r.U
            latched(bad_u, off, ids, cand, _native.M2D_ERR_BAD_USER_ID, 100 + r.U, 9, P)
            bad_u[9] = 99
            latched(bad_u, off, ids, cand, _native.M2D_ERR_BAD_USER_ID, 99, 9, P)
        for cand in (None, 0, 70):
            x = ids.copy(); x[4] = r.I                       # position 4 of the id array: [0, 2, 299] -> 300
            latched(users, off, x, cand, _native.M2D_ERR_BAD_ITEM_ID, r.I, 4, P)
            x = ids.copy(); x[2], x[3] = 9, 2                # [9, 2, 299]: the id at position 3 is below its predecessor
            latched(users, off, x, cand, _native.M2D_ERR_INVALID_ARG, 2, 3, P)
            o = off.copy(); o[0] = 1
            latched(users, o, ids, cand, _native.M2D_ERR_INVALID_ARG, 1, 0, P)
    eng.close()


# ---- 9. around the calls ---------------------------------------------------------------------------------------------------------------------
def test_lists_follow_writers_and_a_new_head():
    import torch
    r = dc.normal_recipe(64, I=500, U=16, seed=2)
    rng = np.random.default_rng(8)
    eng = _engine(r, head=r.head, tables=(r.PM.copy(), r.RE.copy(), r.CE.copy()))
    users = np.arange(r.U, dtype=np.int32)
    t = lambda a: torch.as_tensor(a, device="cuda")         # noqa: E731

    def snapshot(e):
        return _deep(e, users, 200), _deep(e, users, 200, candidates=0), _deep(e, users, 100, candidates=200)

    def fresh(head):
        f = _engine(r, head=head, tables=(eng.pm.cpu().numpy(), eng.re.cpu().numpy(), eng.ce.cpu().numpy()))
        out = snapshot(f)
        f.close()
        return out

    def check(before, head, what):
        now = snapshot(eng)
        assert any(not dc.same(a, b) for a, b in zip(before, now)), what + " changed nothing"
        for a, b in zip(now, fresh(head)):
            _assert_same(a, b, what)
        return now

    state = snapshot(eng)
    B, L = 400, 7
    wu = (np.arange(B) % r.U).astype(np.int32)
    wi = rng.choice(np.flatnonzero(r.cats.sum(1) > 0), B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, r.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(r.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    state = check(state, r.head, "write_memory")
    eng.re[:50] *= 1.5
    eng.tables_updated()
    state = check(state, r.head, "tables_updated")
    head2 = mlp_head(5 * r.E, 256, 64, rng, scale=4.0)
    eng.set_mlp_head(*head2)
    now = snapshot(eng)
    _assert_same(now[0], state[0], "a new head leaves the catalogue lists alone")
    assert not dc.same(now[1], state[1])
    for a, b in zip(now, fresh(head2)):
        _assert_same(a, b, "a new head")
    eng.close()


def test_existing_calls_are_what_they_were_around_deep_calls():
    from foodrec_amd import _native
    r = dc.normal_recipe(64)
    users = _dev(r.users)
    slate = _dev(np.arange(0, r.I, 3, dtype=np.int32))
    pu, pi = _dev(np.repeat(r.users, 20)), _dev(np.tile(np.arange(20, dtype=np.int32) * 7, len(r.users)))

    def existing(e, head):
        out = [_t(e.topk_users(users, 10)), (dc.words(e.score_pairs_bydish(pu, pi).cpu().numpy()), np.zeros(1))]
        out.append(_t(e.topk_users_mlp(users, 10, 0)) if head else _t(e.topk_slate(users, slate, 10)))
        e.check()
        return out

    for head in (False, True):
        eng = _engine(r, head=r.head if head else None)
        before = existing(eng, head)
        _deep(eng, r.users, 1024)
        _deep(eng, r.users, 300, dc.segment_lists(r.I, len(r.users)))
        if head:
            _deep(eng, r.users, 300, candidates=0)
            _deep(eng, r.users, 64, candidates=1024)
        assert _abi(eng, r.users, 1025)[0] == _native.M2D_ERR_INVALID_ARG                  # a refused call
        for a, b in zip(before, existing(eng, head)):
            _assert_same(a, b, "an existing call moved (head = %s)" % head)
        eng.close()


def test_torch_ops_and_the_model():
    import types
    import torch
    import foodrec_amd
    r = dc.normal_recipe(64)
    eng = _engine(r, head=r.head)
    users = r.users[:9]
    lists = dc.segment_lists(r.I, len(users))
    off, ids = map(_dev, dc.csr(lists))
    want = _deep(eng, users, 300, lists)
    _assert_same(_t(torch.ops.m2d.topk_users_deep(eng.id, _dev(users), 300, off, ids)), want, "torch.ops.m2d.topk_users_deep")
    _assert_same(_t(eng.topk_users_deep(_dev(users), 300, [sorted(set(x)) for x in lists])), want, "lists of id lists")
    _assert_same(_t(torch.ops.m2d.topk_users_deep(eng.id, _dev(users), 300)), _deep(eng, users, 300), "no exclusions")
    _assert_same(_t(torch.ops.m2d.topk_users_mlp_deep(eng.id, _dev(users), 100, 256, off, ids)), _deep(eng, users, 100, lists, candidates=256),
                 "torch.ops.m2d.topk_users_mlp_deep")
    eng.check()
    eng.close()
    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    model.set_mlp_head(*r.head)
    excl = {int(u): sorted(set(x)) for u, x in zip(users[:7], lists[:7])}
    per_user = [excl.get(int(u), []) for u in users]
    s, i = model.topk_deep(users.tolist(), exclude=excl)
    assert s.shape == i.shape == (9, 100) and s.dtype == np.float32 and i.dtype == np.int32
    _assert_same((dc.words(s), i), _deep(model.engine, users, 100, per_user), "Model.topk_deep")
    s, i = model.topk_deep(users.tolist(), 50, exclude=excl, head=True, candidates=200)
    _assert_same((dc.words(s), i), _deep(model.engine, users, 50, per_user, candidates=200), "Model.topk_deep(head=True)")
    for k in (0, 1025):
        with pytest.raises(ValueError, match="1 <= k <= 1024"):
            model.topk_deep(users.tolist(), k)
    with pytest.raises(ValueError, match="candidates"):
        model.topk_deep(users.tolist(), 10, candidates=20)
