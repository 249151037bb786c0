"""GPU tests of filtered menu retrieval (m2d_topk_menu_filtered; build-defined, no reference counterpart): the
lists against the restatement (tests/menu_filtered_cases.py) applied to the engine's OWN m2d_score_slate words over arange(I), the
equalities with m2d_topk_menu, m2d_topk_users_deep and m2d_topk_slate, independence from the launcher's cut and from the selection
form, errors and refusals, state changes, the neighbouring calls, the Python surface.  No comparison has a tolerance: ids as
integers, scores as 32-bit words.  The calls go through the C ABI into poisoned buffers with a guard row on either side.  The
conditions the cases rely on are asserted in tests/test_menu_filtered_cases_cpu.py on host scores and again here, where a case depends
on them, on the engine's words."""
import ctypes

import numpy as np
import pytest

import deep_cases as dc
import menu_cases as mc
import menu_filtered_cases as mf

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN no kernel computes; as an id: no dish
NAME = "m2d_topk_menu_filtered"


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(r, user_base=0, masks=True, tables=None):
    from foodrec_amd import ScoringEngine
    PM, RE, CE = tables if tables is not None else (r.PM, r.RE, r.CE)
    eng = ScoringEngine(PM, RE, CE, coef=r.coef, user_base=user_base)
    if masks:
        eng.set_dish_categories(r.cats)
    return eng


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


def _abi(eng, users, caps, k, lists=None, slate=None, null=(), raw=None, nD=None, plain=False):
    """One call through the C ABI -> (status, score words uint32 [nU, k], ids int64 [nU, k]); the guard rows are checked.  lists: one id
    list per user (ascending, repeats allowed) -> CSR; raw: an (offsets, ids) pair as it is; plain: m2d_topk_menu instead."""
    import torch
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    users = np.asarray(users, np.int32)
    nU = len(users)
    caps = np.ascontiguousarray(np.broadcast_to(np.asarray(caps, np.int32), (nU, eng.C)))
    ut = _dev(users if nU else np.zeros(1, np.int32))
    ct = _dev(caps.reshape(-1) if nU else np.zeros(1, np.int32))
    off = ids = st = None
    if raw is not None or lists is not None:
        o, x = raw if raw is not None else mf.csr(lists)
        off, ids = _dev(np.asarray(o, np.int64)), _dev(np.asarray(x, np.int32) if len(x) else np.zeros(1, np.int32))
    if slate is not None:
        st = _dev(np.asarray(slate, np.int32))
        nD = len(slate) if nD is None else nD
    kk = max(int(k), 1)
    bs = torch.full(((nU + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    bi = torch.full(((nU + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    ptr = lambda t, name, shift=0: None if name in null or t is None else t.data_ptr() + shift      # noqa: E731
    if plain:
        rc = _native.lib().m2d_topk_menu(eng._h, ptr(ut, "users"), nU, int(k), ptr(ct, "caps"), ptr(bs, "scores", 4 * kk),
                                         ptr(bi, "out_ids", 4 * kk), _stream_ptr())
    else:
        rc = _native.lib().m2d_topk_menu_filtered(eng._h, ptr(ut, "users"), nU, int(k), ptr(ct, "caps"), ptr(off, "excl_off"),
                                                  ptr(ids, "excl_ids"), ptr(st, "slate"), int(nD or 0), ptr(bs, "scores", 4 * kk),
                                                  ptr(bi, "out_ids", 4 * kk), _stream_ptr())
    torch.cuda.synchronize()
    s, i = bs.cpu().numpy().view(np.uint32).reshape(nU + 2, kk), bi.cpu().numpy().reshape(nU + 2, kk)
    assert (s[[0, -1]] == POISON).all() and (i[[0, -1]] == POISON).all(), "a guard row was written"
    return rc, s[1:-1], i[1:-1].astype(np.int64)


def _menu(eng, users, caps, k, lists=None, slate=None, plain=False):
    """the lists of a call that must succeed: every element written, the id latch clear"""
    rc, s, i = _abi(eng, users, caps, k, lists, slate, plain=plain)
    assert rc == 0, eng_error(eng)
    eng.check()
    assert (i != POISON).all() and (s != POISON).all(), "%d elements not written" % int((i == POISON).sum())
    return s, i


def _matrix(eng, U, user_base=0):
    """the engine's own m2d_score_slate words of every user for every dish: float32 [U, I]"""
    out = eng.score_slate(_dev(np.arange(U, dtype=np.int32) + user_base), _dev(np.arange(eng.I, dtype=np.int32)))
    eng.check()
    return out.cpu().numpy()


def _same(got, want, what=""):
    assert np.array_equal(np.asarray(got[1], np.int64), np.asarray(want[1], np.int64)), "%s: ids of %d rows differ" % (
        what, int((np.asarray(got[1]) != np.asarray(want[1])).any(1).sum()))
    assert np.array_equal(np.asarray(got[0], np.uint32), np.asarray(want[0], np.uint32)), "%s: score words differ" % what


def _t(x):
    s, i = x
    return dc.words(s.cpu().numpy()), i.cpu().numpy().astype(np.int64)


def _both_selections(eng, users, caps, k, lists, slate, want, what):
    for select in (0, 1):
        eng.set_option("menu_select", select)
        _same(_menu(eng, users, caps, k, lists, slate), want, "%s, menu_select = %d" % (what, select))
    eng.set_option("menu_select", 0)


# ---- 1. the equalities ----------------------------------------------------------------------------------------------------------------
def test_null_filters_are_topk_menu_words_and_launches():
    from foodrec_amd import _native
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    n = len(r.users)
    for caps, k in ((mc.caps_all(n, 6, 2), 10), (mc.caps_mixed(n, 6), 64)):
        for P in (256, dc.DEFAULT_P):
            eng.set_option("deep_chunk_pairs", P)
            want = _menu(eng, r.users, caps, k, plain=True)
            kernel = eng.last_kernel()
            _same(_menu(eng, r.users, caps, k), want, "null filters, P = %d" % P)
            assert eng.last_kernel() == kernel == "m2d_menu_merge"
    _same(_menu(eng, r.users, caps, k, slate=np.arange(r.I)), want, "slate = arange(I)")
    lists = mf.own_menu_lists(_matrix(eng, r.U)[r.users], r.cats, caps, k)
    _same(_menu(eng, r.users, caps, k, lists, np.arange(r.I)), _menu(eng, r.users, caps, k, lists), "slate = arange(I), exclusions")
    assert _native.lib().m2d_topk_menu_filtered is not None
    eng.close()


@pytest.mark.parametrize("recipe", ("exact4", "normal6"))
def test_caps_of_k_give_the_deep_lists_and_topk_slates_lists(recipe):
    r = mc.exact_recipe(4, 64, 1300) if recipe == "exact4" else mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    users, n = r.users, len(r.users)
    for k in (1, 10, 64):
        caps = mc.caps_uncapped(n, r.C, k)
        lists = mf.own_menu_lists(S[users], r.cats, caps, k, seed=k)
        off, ids = mf.csr(lists)
        deep = _t(eng.topk_users_deep(_dev(users), k, (_dev(off), _dev(ids))))
        eng.check()
        _same(deep, dc.key_lists(S[users], k, lists), "topk_users_deep against the key rule")
        _same(_menu(eng, users, caps, k, lists), deep, "caps >= k with exclusions, k = %d" % k)
        for nD in (64, 257, 1299):
            slate = mf.slate_of(r.I, nD, seed=k)
            top = _t(eng.topk_slate(_dev(users), _dev(slate), k))
            eng.check()
            _same(_menu(eng, users, caps, k, None, slate), top, "caps >= k over a slate of %d, k = %d" % (nD, k))
    eng.close()


def test_one_users_menu_over_slate_less_x_is_the_menu_over_the_slate_with_x_excluded():
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    slate = mf.slate_of(r.I, 700)
    for j, u in enumerate(r.users[:4]):
        caps = mc.caps_mixed(1, 6, seed=j, hi=4)
        x = mf.own_menu_lists(S[u:u + 1], r.cats, caps, 10, slate, sizes=(65,), seed=j)
        less = np.setdiff1d(slate, x[0]).astype(np.int32)
        a, b = _menu(eng, [u], caps, 10, x, slate), _menu(eng, [u], caps, 10, None, less)
        _same(a, b, "user %d" % u)
        _same(a, mf.filtered_lists(S[u:u + 1], r.cats, caps, 10, x, slate))
        assert mf.differs(a, _menu(eng, [u], caps, 10, None, slate)).all()
    eng.close()


# ---- 2. the strike form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", (False, True))
@pytest.mark.parametrize("n", mf.SEGMENT_NS + (16385,))
def test_segments_of_every_size_under_exclusion_lists_of_every_size(n, multi):
    """a segment of n dishes -- one wave, four waves, sixteen waves of a selection block, a wave's second step -- alone in the catalogue
    and among the dishes of other signatures; exclusion segments of 0 / 1 / 63 / 64 / 65 / 300 ids with repeats, ids of other
    signatures interleaved, each starting with the row's own best menu dishes; both selections; ranges of 256 where there are several"""
    r = mf.segment_recipe_n(n, multi=multi)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, users, rows = S[r.users], r.users, len(r.users)
    for caps, k in ((mc.caps_all(rows, 4, 2), min(10, r.I)), (mc.caps_uncapped(rows, 4, 64), min(64, r.I))):
        lists = mf.own_menu_lists(W32, r.cats, caps, k)
        want = mf.filtered_lists(W32, r.cats, caps, k, lists)
        free = mc.menu_lists(W32, r.cats, caps, k)
        assert (mf.differs(want, free) == np.asarray([len(x) > 0 for x in lists])).all()
        _both_selections(eng, users, caps, k, lists, None, want, "n = %d, k = %d" % (n, k))
        if n in (257, 1025):                                  # ranges of 256: the last one is a single dish, narrower than k
            eng.set_option("deep_chunk_pairs", 256)
            _both_selections(eng, users, caps, k, lists, None, want, "n = %d, k = %d, ranges of 256" % (n, k))
            eng.set_option("deep_chunk_pairs", dc.DEFAULT_P)
    if n >= 63:                                               # the whole segment excluded, and all of it but its last dish
        caps = mc.caps_uncapped(rows, 4, 64)
        for x in (r.segment, r.segment[:-1]):
            lists = [x] * rows
            want = mf.filtered_lists(W32, r.cats, caps, min(64, r.I), lists)
            assert not np.isin(want[1], x).any()
            _same(_menu(eng, users, caps, min(64, r.I), lists), want, "a whole segment excluded")
    eng.close()


@pytest.mark.parametrize("n,multi", ((1025, True), (1025, False), (257, True)))
def test_excluded_dishes_on_both_sides_of_every_slice_and_step_edge(n, multi):
    """best dishes planted at a segment's first and last dish and on both sides of every 64-slice edge (every fourth: a 256-step edge);
    one side excluded, the other listed"""
    r = mf.slice_edge_recipe(n, multi)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, rows = S[r.users], len(r.users)
    lists, kept = mf.edge_lists(r, r.users)
    for caps, k in ((mc.caps_uncapped(rows, 4, 64), 64), (mc.caps_all(rows, 4, 9), 64)):
        want = mf.filtered_lists(W32, r.cats, caps, k, lists)
        if caps[0, 0] == 64:
            free = mc.menu_lists(W32, r.cats, caps, k)
            for j in range(rows):
                assert np.isin(lists[j], free[1][j]).all() and np.isin(kept[j], want[1][j]).all()
        for P in (256, 2048, dc.DEFAULT_P):
            eng.set_option("deep_chunk_pairs", P)
            _both_selections(eng, r.users, caps, k, lists, None, want, "P = %d" % P)
    eng.close()


def test_excluded_dishes_on_both_sides_of_every_range_and_segment_edge():
    r = mc.edge_recipe()
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, rows = S[r.users], len(r.users)
    lists, pairs = mf.range_edge_lists(r, r.users)
    more = [np.sort(np.concatenate([x, y])) for x, y in zip(lists, mf.own_menu_lists(W32, r.cats, mc.caps_all(rows, 4, 2), 10, seed=1))]
    for ls in (lists, more):
        for caps, k in ((mc.caps_uncapped(rows, 4, 64), 64), (mc.caps_all(rows, 4, 2), 10), (mc.caps_mixed(rows, 4, hi=9), 64)):
            want = mf.filtered_lists(W32, r.cats, caps, k, ls)
            for P in (256, 2048, dc.DEFAULT_P):
                eng.set_option("deep_chunk_pairs", P)
                _both_selections(eng, r.users, caps, k, ls, None, want, "P = %d, k = %d" % (P, k))
            for j in (0, rows - 1):                           # nU = 1 and the row's position
                _same(_menu(eng, r.users[j:j + 1], caps[j:j + 1], k, ls[j:j + 1]), (want[0][j:j + 1], want[1][j:j + 1]), "nU = 1")
    eng.close()


@pytest.mark.parametrize("C,E,I", ((3, 64, 1300), (4, 64, 1300), (5, 64, 1300), (6, 64, 1300), (4, 4, 257), (4, 200, 257), (6, 200, 1300)))
def test_every_category_count_and_width(C, E, I):
    r = mc.normal_recipe(C, E, I) if C == 6 else mc.exact_recipe(C, E, I)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, rows = S[r.users], len(r.users)
    slate = mf.slate_of(I, I // 2)
    for name in ("one", "two", "mixed"):
        caps = mc.cap_set(name, rows, C, 10)
        for sl in (None, slate):
            lists = mf.own_menu_lists(W32, r.cats, caps, 10, sl)
            want = mf.filtered_lists(W32, r.cats, caps, 10, lists, sl)
            _both_selections(eng, r.users, caps, 10, lists, sl, want, "C %d E %d caps %s slate %s" % (C, E, name, sl is not None))
    eng.close()


@pytest.mark.parametrize("group", mc.TIE_GROUPS)
def test_tied_copies_across_segments_with_one_of_a_pair_excluded(group):
    r = mc.tie_recipe(group)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    w = dc.words(S)
    assert (w[:, r.copies] == w[:, r.copies[:1]]).all() and sorted(set(r.sig[r.copies])) == [1, 2]
    slate = mf.slate_of(r.I, 900, keep=r.copies)
    for j, u in enumerate(r.users):
        k = r.k[j]
        for x in (r.copies[0::2], r.copies[1::2], r.copies[:1]):
            for caps in (mc.caps_uncapped(1, 4, k), np.asarray([[k, 1, k, k]], np.int32)):
                for sl in (None, slate):
                    want = mf.filtered_lists(S[u:u + 1], r.cats, caps, k, [x], sl)
                    _same(_menu(eng, [u], caps, k, [x], sl), want, "group %d, user %d" % (group, u))
        if j < len(r.users) - 1:                              # (the last user is the all-zero user: its ties go to the lowest ids)
            free = mf.filtered_lists(S[u:u + 1], r.cats, mc.caps_uncapped(1, 4, k), k, None, slate)
            assert np.isin(free[1], r.copies).any()           # without exclusions copies are listed
    eng.close()


# ---- 3. the slate form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", (1300, 16385))
def test_slates_of_every_size(I):
    r = mc.normal_recipe(6, 64, I)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, rows = S[r.users], len(r.users)
    caps = mc.caps_all(rows, 6, 2)
    free = mc.menu_lists(W32, r.cats, caps, 10)
    for nD in mf.SLATE_NDS:
        slate = mf.slate_of(I, nD, seed=nD)
        want = mf.filtered_lists(W32, r.cats, caps, 10, None, slate)           # nD = 1, 63 under caps: k > what the slate can give
        if nD < I:
            after = [[d for d in row if d in set(slate.tolist())] for row in free[1]]
            assert any(want[1][j][want[1][j] >= 0].tolist() != after[j] for j in range(rows))
        _both_selections(eng, r.users, caps, 10, None, slate, want, "nD = %d" % nD)
        lists = mf.own_menu_lists(W32, r.cats, caps, 10, slate, seed=nD)
        want = mf.filtered_lists(W32, r.cats, caps, 10, lists, slate)
        _both_selections(eng, r.users, caps, 10, lists, slate, want, "nD = %d with exclusions" % nD)
        if nD <= 63:                                          # k > nD, uncapped: the whole slate in order, then -1 / NaN
            want = mf.filtered_lists(W32, r.cats, mc.caps_uncapped(rows, 6, 64), 64, None, slate)
            assert ((want[1] >= 0).sum(1) == nD).all()
            _same(_menu(eng, r.users, mc.caps_uncapped(rows, 6, 64), 64, None, slate), want, "k > nD = %d" % nD)
    for keep in ((1, 2, 5, 40), (3,)):                       # a slate that leaves whole signatures empty; a slate of one signature
        slate = np.flatnonzero(np.isin(r.sig, keep)).astype(np.int32)
        assert len(slate) >= 1
        for P in (256, dc.DEFAULT_P):
            eng.set_option("deep_chunk_pairs", P)
            lists = mf.own_menu_lists(W32, r.cats, caps, 10, slate)
            _same(_menu(eng, r.users, caps, 10, lists, slate), mf.filtered_lists(W32, r.cats, caps, 10, lists, slate), "signatures %s" % (keep,))
    eng.close()


# ---- 4. errors and refusals ------------------------------------------------------------------------------------------------------------------
def test_bad_lists_slates_users_and_caps_are_latched_with_value_and_position():
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    r = mc.normal_recipe(6, 64, 1300)
    base = 100
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, user_base=base)
    users, n = r.users + base, len(r.users)
    caps = mc.caps_mixed(n, 6, seed=2)
    slate = mf.slate_of(r.I, 257)
    lists = mf.own_menu_lists(S[r.users], r.cats, caps, 10, slate)
    want = mf.filtered_lists(S[r.users], r.cats, caps, 10, lists, slate)
    _same(_menu(eng, users, caps, 10, lists, slate), want)
    off, ids = mf.csr(lists)

    def deep_reports(o, x):                                  # what m2d_topk_users_deep latches for the same lists
        import torch
        out_s, out_i = torch.empty((n, 10), device="cuda"), torch.empty((n, 10), dtype=torch.int32, device="cuda")
        ot, xt, ut = _dev(np.asarray(o, np.int64)), _dev(np.asarray(x, np.int32)), _dev(users)
        assert _native.lib().m2d_topk_users_deep(eng._h, ut.data_ptr(), n, 10, ot.data_ptr(), xt.data_ptr(), out_s.data_ptr(),
                                                 out_i.data_ptr(), _stream_ptr()) == 0
        return _latched(eng)

    at = int(off[4]) - 1                                     # the last id of row 3's segment: no id of the segment behind it
    assert off[4] - off[3] > 64 and ids[at - 1] > 0
    for pos, value in ((at, r.I), (at, -1), (at, int(ids[at - 1]) - 1), (len(ids) - 1, 2 ** 31 - 1)):
        x = ids.copy(); x[pos] = value
        code = _native.M2D_ERR_BAD_ITEM_ID if not 0 <= value < r.I else _native.M2D_ERR_INVALID_ARG
        for sl in (None, slate):
            assert _abi(eng, users, caps, 10, raw=(off, x), slate=sl)[0] == 0
            got = _latched(eng)
            assert got == (code, value, pos) == deep_reports(off, x), (pos, value, got)
    for q, value in ((0, 1), (4, int(off[3]) - 1), (n, int(off[n - 1]) - 1)):
        o = off.copy(); o[q] = value
        assert _abi(eng, users, caps, 10, raw=(o, ids), slate=slate)[0] == 0
        got = _latched(eng)
        assert got[0] != 0 and got == deep_reports(o, ids), (q, value, got)
    for pos, value in ((0, -1), (100, r.I), (256, 2 ** 31 - 1), (17, -(2 ** 31))):
        sl = slate.copy(); sl[pos] = value
        assert _abi(eng, users, caps, 10, lists, sl)[0] == 0
        assert _latched(eng) == (_native.M2D_ERR_BAD_ITEM_ID, value, pos), (pos, value)
    for pos in (1, 64, 256):
        for value in (int(slate[pos - 1]), int(slate[pos - 1]) - 1):          # equal to its predecessor, below it
            sl = slate.copy(); sl[pos] = value
            assert _abi(eng, users, caps, 10, lists, sl)[0] == 0
            assert _latched(eng) == (_native.M2D_ERR_INVALID_ARG, value, pos), (pos, value)
    for P in (dc.DEFAULT_P, 256):
        eng.set_option("deep_chunk_pairs", P)
        for row in (0, n // 2, n - 1):
            ok = np.setdiff1d(np.arange(n), [row])
            u = users.copy(); u[row] = base + r.U
            rc, s, i = _abi(eng, u, caps, 10, lists, slate)
            assert rc == 0 and _latched(eng) == (_native.M2D_ERR_BAD_USER_ID, base + r.U, row)
            _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), "the other users' rows")
            bad = caps.copy(); bad[row, 4] = -3
            rc, s, i = _abi(eng, users, bad, 10, lists, slate)
            assert rc == 0 and _latched(eng) == (_native.M2D_ERR_INVALID_ARG, -3, row * 6 + 4)
            _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), "the other users' rows")
    _same(_menu(eng, users, caps, 10, lists, slate), want, "after the latched errors")
    eng.close()


def test_argument_errors():
    from foodrec_amd import _native
    r = mc.exact_recipe(4, 64, 257)
    eng = _engine(r)
    caps = mc.caps_all(len(r.users), 4, 2)
    lists = [np.asarray([1, 2], np.int64)] * len(r.users)
    slate = mf.slate_of(r.I, 100)
    bad = _native.M2D_ERR_INVALID_ARG
    for k in (0, 65, -3, 1024):
        assert _abi(eng, r.users, caps, k, lists, slate)[0] == bad and NAME + ": need nU >= 0 and 1 <= k <= min(64, I)" in eng_error(eng)
    for nD in (0, -1, r.I + 1):
        assert _abi(eng, r.users, caps, 5, lists, slate, nD=nD)[0] == bad and eng_error(eng) == NAME + ": with a slate need 1 <= nD <= I"
    assert _abi(eng, r.users, caps, 5, lists, slate, null=("excl_ids",))[0] == bad and eng_error(eng) == NAME + ": excl_off without excl_ids"
    for null in ("users", "caps", "scores", "out_ids"):
        assert _abi(eng, r.users, caps, 5, lists, slate, null=(null,))[0] == bad and eng_error(eng) == NAME + ": null buffer"
    assert _abi(eng, np.zeros(0, np.int32), caps[:0], 5, [], slate)[0] == 0 and _latched(eng)[0] == 0      # nU == 0: nothing is launched
    S = _matrix(eng, r.U)
    want = mf.filtered_lists(S[r.users], r.cats, caps, 64, lists, slate)     # k = 64 > what a slate of 100 gives under caps of 2
    _same(_menu(eng, r.users, caps, 64, lists, slate), want, "k = 64")
    eng.close()
    bare = _engine(r, masks=False)
    assert _abi(bare, r.users, caps, 5, lists, slate)[0] == _native.M2D_ERR_NOT_CONFIGURED
    bare.close()


def test_refusals_name_the_call():
    from foodrec_amd import _native
    rng = np.random.default_rng(2)
    r7 = mc.normal_recipe(7, 64, 300)
    eng = _engine(r7)
    assert _abi(eng, r7.users, mc.caps_all(len(r7.users), 7, 2), 5, slate=np.arange(10))[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng).startswith(NAME + ": more than 6 categories")
    eng.close()
    r = dc.normal_recipe(64, I=300, U=8, seed=1, head=False)
    eng = _engine(r)
    users = np.arange(r.U, dtype=np.int32)
    caps = mc.caps_all(r.U, 4, 2)
    slate, lists = mf.slate_of(r.I, 100), [np.asarray([3, 9], np.int64)] * r.U
    want = _menu(eng, users, caps, 10, lists, slate)
    nnz = 3 * r.I
    eng.set_ingredients((rng.standard_normal((50, r.E)) / 8).astype(np.float32), np.arange(0, nnz + 1, 3, dtype=np.int32),
                        rng.integers(0, 50, nnz).astype(np.int32))
    for kw in (dict(), dict(lists=lists), dict(slate=slate)):
        assert _abi(eng, users, caps, 10, **kw)[0] == _native.M2D_ERR_UNSUPPORTED
        assert eng_error(eng) == NAME + ": the ingredient table is set (not supported)"
    eng.clear_ingredients()
    keep = eng.re[7, 3].item()
    eng.re[7, 3] = float("inf")
    eng.tables_updated()
    assert _abi(eng, users, caps, 10, lists, slate)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng) == NAME + ": needs finite tables (a table value is not finite)"
    eng.re[7, 3] = keep
    eng.tables_updated()
    _same(_menu(eng, users, caps, 10, lists, slate), want, "after the value was put back")
    eng.close()


# ---- 5. engine state ---------------------------------------------------------------------------------------------------------------------------
def test_lists_follow_write_memory_tables_updated_and_new_masks():
    import torch
    b = dc.normal_recipe(64, I=500, U=16, seed=2, head=False)
    rng = np.random.default_rng(8)
    eng = _engine(b, tables=(b.PM.copy(), b.RE.copy(), b.CE.copy()))
    users = np.arange(b.U, dtype=np.int32)
    caps = mc.caps_all(b.U, 4, 2)
    slate = mf.slate_of(b.I, 300)
    t = lambda a: torch.as_tensor(a, device="cuda")         # noqa: E731
    cats = [b.cats]

    def check(before, what):
        S = _matrix(eng, b.U)
        lists = mf.own_menu_lists(S, cats[0], caps, 10, slate)
        now = _menu(eng, users, caps, 10, lists, slate)
        _same(now, mf.filtered_lists(S, cats[0], caps, 10, lists, slate), what)
        plain = _menu(eng, users, caps, 10, None, slate)
        assert before is None or not dc.same(before, plain), what + " changed nothing"
        return plain

    state = check(None, "at the start")
    B, L = 400, 7
    wu = (np.arange(B) % b.U).astype(np.int32)
    wi = rng.choice(np.flatnonzero(b.cats.sum(1) > 0), B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, b.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(b.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    state = check(state, "write_memory")
    eng.re[:50] *= 1.5
    eng.tables_updated()
    state = check(state, "tables_updated")
    cats[0] = np.roll(b.cats, 1, axis=1)                     # other signatures for the same dishes: the slate's partition follows
    assert (mc.signatures(cats[0]) != mc.signatures(b.cats)).mean() > 0.5
    eng.set_dish_categories(cats[0])
    state = check(state, "a second set_dish_categories")     # (the first call after it is the slate form: it builds the catalogue index)
    cats[0] = b.cats
    eng.set_dish_categories(cats[0])
    check(state, "the first masks again")
    eng.close()


def test_a_user_base_shard():
    r = mc.normal_recipe(6, 64, 1300)
    base = 1000
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, user_base=base)
    users = np.asarray([3, 3, 3, 0, 7, 3, 0], np.int32)
    caps = mc.caps_mixed(len(users), 6, seed=4)
    slate = mf.slate_of(r.I, 700)
    lists = mf.own_menu_lists(S[users], r.cats, caps, 10, slate)
    _same(_menu(eng, users + base, caps, 10, lists, slate), mf.filtered_lists(S[users], r.cats, caps, 10, lists, slate), "a shard")
    eng.close()


def test_filters_that_arrive_late_on_a_side_stream():
    """Stream order: on a side stream a blocker (matrix products), then the copies that put the real exclusion lists and the real slate
    where decoys stood, then the call -- entered while the blocker runs (the slate form then waits for that stream).  The lists are the
    real request's, on an engine whose first menu call this is and again on the warmed engine."""
    import torch
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    n = len(r.users)
    caps = mc.caps_mixed(n, 6, seed=5)
    twin = _engine(r)
    S = _matrix(twin, r.U)
    slates = (mf.slate_of(r.I, 700, seed=1), mf.slate_of(r.I, 700, seed=2))
    lists = [mf.own_menu_lists(S[r.users], r.cats, caps, 10, sl, sizes=(65,), seed=j) for j, sl in enumerate(slates)]
    want, other = (_menu(twin, r.users, caps, 10, ls, sl) for ls, sl in zip(lists, slates))
    twin.close()
    assert mf.differs(want, other).mean() >= 0.9             # the decoy's answer is another one
    (off, ids), (doff, dids) = mf.csr(lists[0]), mf.csr(lists[1])
    assert len(ids) == len(dids)
    a = torch.randn((8192, 8192), device="cuda")
    side = torch.cuda.Stream()
    src = [_dev(x) for x in (off, ids, slates[0])]
    ut, ct = _dev(r.users), _dev(caps)
    for episode in ("first use", "warmed"):
        bufs = [_dev(x) for x in (doff, dids, slates[1])]
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(6):
                a @ a
            for b, s in zip(bufs, src):
                b.copy_(s, non_blocking=True)
            arrived = torch.cuda.Event()
            arrived.record(side)
            late = not arrived.query()                        # the copies had not landed when the call was made
            got = torch.ops.m2d.topk_menu_filtered(eng.id, ut, ct, 10, bufs[0], bufs[1], bufs[2])
            side.synchronize()
            eng.check()
        assert late, "the blocker was too short to show anything"
        _same(_t(got), want, "side stream, " + episode)
    eng.close()


def test_existing_calls_are_what_they_were_around_the_new_call():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, head=False)
    users = _dev(r.users)
    n = len(r.users)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    caps = mc.caps_all(n, 4, 2)
    slate = mf.slate_of(r.I, 300)
    lists = mf.own_menu_lists(S[r.users], r.cats, caps, 10, sizes=(65, 300))
    off, ids = (_dev(x) for x in mf.csr(lists))

    def existing():
        out = [_menu(eng, r.users, caps, 10, plain=True), _t(eng.topk_users_deep(users, 300, (off, ids))),
               _t(eng.topk_slate(users, _dev(slate), 10)), _t(eng.topk_users(users, 10))]
        eng.check()
        return out

    before = existing()
    for sl in (None, slate):
        _menu(eng, r.users, caps, 10, lists, sl)
        _menu(eng, r.users, mc.caps_mixed(n, 4), 64, lists, sl)
    assert _abi(eng, r.users, caps, 65, lists, slate)[0] == _native.M2D_ERR_INVALID_ARG            # a refused call
    bad = slate.copy(); bad[5] = r.I                                                                # three failed ones
    assert _abi(eng, r.users, caps, 10, lists, bad)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_ITEM_ID
    x = [np.asarray([5, 4], np.int64)] * n
    assert _abi(eng, r.users, caps, 10, x, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_INVALID_ARG
    u = r.users.copy(); u[3] = r.U
    assert _abi(eng, u, caps, 10, lists, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_USER_ID
    for a, b in zip(before, existing()):
        _same(a, b, "an existing call moved")
    eng.close()


# ---- 6. the Python surface ----------------------------------------------------------------------------------------------------------------------
def test_torch_op_and_the_model():
    import types
    import torch
    import foodrec_amd
    r = dc.normal_recipe(64, head=False)
    eng = _engine(r)
    n = len(r.users)
    caps = mc.caps_mixed(n, 4)
    S = _matrix(eng, r.U)
    slate = mf.slate_of(r.I, 300)
    lists = mf.own_menu_lists(S[r.users], r.cats, caps, 10, slate)
    off, ids = (_dev(x) for x in mf.csr(lists))
    want = _menu(eng, r.users, caps, 10, lists, slate)
    op = torch.ops.m2d.topk_menu_filtered
    _same(_t(op(eng.id, _dev(r.users), _dev(caps), 10, off, ids, _dev(slate))), want, "torch.ops.m2d.topk_menu_filtered")
    _same(_t(op(eng.id, _dev(r.users), _dev(caps), 10)), _menu(eng, r.users, caps, 10, plain=True), "the op without filters")
    one = np.asarray([2, 0, 1, 3], np.int32)                  # a single row is broadcast
    _same(_t(op(eng.id, _dev(r.users), _dev(one), 12, among=_dev(slate))), _menu(eng, r.users, np.tile(one, (n, 1)), 12, None, slate), "caps [C]")
    _same(_t(eng._topk_menu_filtered(_dev(r.users), 10, _dev(caps), [x.tolist() for x in lists], _dev(slate))), want, "host lists")
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        eng._topk_menu_filtered(_dev(r.users), 65, _dev(one))
    with pytest.raises(TypeError):
        eng._topk_menu_filtered(_dev(r.users), 5, _dev(one), among=_dev(slate.astype(np.int64)))
    with pytest.raises(ValueError, match="at least one dish"):
        eng._topk_menu_filtered(_dev(r.users), 5, _dev(one), among=_dev(slate[:0]))
    eng.close()

    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    who = [str(u) for u in r.users]                          # ids as the reference feeds them: str
    had = {who[j]: [str(d) for d in lists[j][::-1]] for j in range(n) if j % 2 == 0}           # a dict: any order, repeats, missing keys
    by_row = [np.unique(np.asarray(had.get(u, []), np.int64)) for u in who]       # (a user who repeats has one list)
    cap2 = np.tile(np.asarray([10, 2, 10, 0], np.int32), (n, 1))
    s, i = model.topk_menu_filtered(who, 10, {1: 2, 3: 0}, exclude=had, among=[str(d) for d in slate[::-1]] + [str(slate[0])])
    assert s.dtype == np.float32 and i.dtype == np.int32
    _same((dc.words(s), i), _menu(model.engine, r.users, cap2, 10, by_row, slate), "Model.topk_menu_filtered, a dict and among")
    s, i = model.topk_menu_filtered(who, 10, {1: 2, 3: 0}, exclude=by_row)
    _same((dc.words(s), i), _menu(model.engine, r.users, cap2, 10, by_row), "Model.topk_menu_filtered, a list, no slate")
    s, i = model.topk_menu_filtered(who)
    _same((dc.words(s), i), _t(model.engine.topk_users_deep(_dev(r.users), 10)), "Model.topk_menu_filtered, nothing given")
    model.set_recipes({str(d): [d % 50, (7 * d) % 50] for d in range(r.I)}, 50)
    market = list(range(0, 50, 2)) + [1, 3]
    for miss in (0, 1):
        cook = model.cookable(market, miss)
        assert 0 < len(cook) < r.I
        s, i = model.topk_menu_filtered(who, 10, {1: 2, 3: 0}, exclude=had, market=market, max_missing=miss)
        _same((dc.words(s), i), _menu(model.engine, r.users, cap2, 10, by_row, cook), "Model.topk_menu_filtered, a market")
    s, i = model.topk_menu_filtered(who, 5, market=[49])
    assert len(model.cookable([49])) == 0 and (i == -1).all() and np.isnan(s).all()
    with pytest.raises(ValueError, match="among together with market"):
        model.topk_menu_filtered(who, among=[1], market=market)
