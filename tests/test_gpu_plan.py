"""GPU tests of meal plans (m2d_plan_menus; build-defined, no reference counterpart): the plans against the
engine's OWN composition -- D calls of m2d_topk_menu_filtered, the host growing the exclusion lists and lowering the caps -- and against
the restatement (tests/plan_cases.py) applied to the engine's own m2d_score_slate words; list edges, the launcher's cuts, ties across a
day boundary, the equalities with the filtered call, errors and refusals, the neighbouring calls, the Python surface.  No comparison
has a tolerance: ids as integers, scores as 32-bit words.  The calls go through the C ABI into poisoned [nU, days, k] buffers with a
guard row on either side.  The conditions the cases rely on are asserted in tests/test_plan_cases_cpu.py on host scores and again
here, where a case depends on them, on the engine's words."""
import ctypes

import numpy as np
import pytest

import deep_cases as dc
import menu_cases as mc
import menu_filtered_cases as mf
import plan_cases as pc

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN no kernel computes; as an id: no dish
NAME = "m2d_plan_menus"


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


def _abi(eng, users, caps, days, k, plan=None, lists=None, slate=None, null=(), raw=None, nD=None, filtered=False):
    """One call through the C ABI -> (status, score words uint32 [nU, days, k], ids int64 [nU, days, k]); the guard rows are checked.
    plan: the plan caps (None: a null pointer); lists: one id list per user -> CSR; raw: an (offsets, ids) pair as it is; filtered:
    m2d_topk_menu_filtered instead (days = 1, no plan caps)."""
    import torch
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    users = np.asarray(users, np.int32)
    nU = len(users)
    table = lambda t: _dev(np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.int32), (nU, eng.C))).reshape(-1) if nU else np.zeros(1, np.int32))  # noqa: E731
    ut = _dev(users if nU else np.zeros(1, np.int32))
    ct = table(caps)
    pt = table(plan) if plan is not None else None
    off = ids = st = None
    if raw is not None or lists is not None:
        o, x = raw if raw is not None else mf.csr(lists)
        off, ids = _dev(np.asarray(o, np.int64)), _dev(np.asarray(x, np.int32) if len(x) else np.zeros(1, np.int32))
    if slate is not None:
        st = _dev(np.asarray(slate, np.int32))
        nD = len(slate) if nD is None else nD
    nd = max(int(days), 1)
    row = nd * max(int(k), 1)
    if row > 4 * pc.MAX_LIST:                                # (a refused call: nothing is written, the buffers need not hold a plan)
        nd = row = 1
    bs = torch.full(((nU + 2) * row,), POISON, dtype=torch.int32, device="cuda")
    bi = torch.full(((nU + 2) * row,), POISON, dtype=torch.int32, device="cuda")
    ptr = lambda t, name, shift=0: None if name in null or t is None else t.data_ptr() + shift      # noqa: E731
    if filtered:
        assert days == 1 and plan is None
        rc = _native.lib().m2d_topk_menu_filtered(eng._h, ptr(ut, "users"), nU, int(k), ptr(ct, "caps"), ptr(off, "excl_off"),
                                                  ptr(ids, "excl_ids"), ptr(st, "slate"), int(nD or 0), ptr(bs, "scores", 4 * row),
                                                  ptr(bi, "out_ids", 4 * row), _stream_ptr())
    else:
        rc = _native.lib().m2d_plan_menus(eng._h, ptr(ut, "users"), nU, int(days), int(k), ptr(ct, "caps"), ptr(pt, "plan_caps"),
                                          ptr(off, "excl_off"), ptr(ids, "excl_ids"), ptr(st, "slate"), int(nD or 0),
                                          ptr(bs, "scores", 4 * row), ptr(bi, "out_ids", 4 * row), _stream_ptr())
    torch.cuda.synchronize()
    s, i = bs.cpu().numpy().view(np.uint32).reshape(nU + 2, row), bi.cpu().numpy().reshape(nU + 2, row)
    assert (s[[0, -1]] == POISON).all() and (i[[0, -1]] == POISON).all(), "a guard row was written"
    shape = (nU, nd, row // nd)
    return rc, s[1:-1].reshape(shape), i[1:-1].astype(np.int64).reshape(shape)


def _plan(eng, users, caps, days, k, plan=None, lists=None, slate=None):
    """the plans of a call that must succeed: every element written, the id latch clear"""
    rc, s, i = _abi(eng, users, caps, days, k, plan, lists, slate)
    assert rc == 0, eng_error(eng)
    eng.check()
    assert (i != POISON).all() and (s != POISON).all(), "%d elements not written" % int((i == POISON).sum())
    return s, i


def _filtered(eng, users, caps, k, lists=None, slate=None):
    rc, s, i = _abi(eng, users, caps, 1, k, None, lists, slate, filtered=True)
    assert rc == 0, eng_error(eng)
    eng.check()
    return s[:, 0], i[:, 0]


def _compose(eng, sig, users, caps, days, k, plan=None, lists=None, slate=None):
    """THE COMPOSITION the call replaces, on the same engine: D calls of m2d_topk_menu_filtered; between them the host appends the
    day's dishes to every user's exclusion list, sorts it, and lowers the caps to min(cap, plan cap - used) floored at 0.  (Once a day
    is empty for every user the later calls would repeat it: they are not made.)"""
    n, C = len(users), eng.C
    caps = np.broadcast_to(np.asarray(caps, np.int64), (n, C))
    had = [np.asarray(x, np.int64) for x in (lists if lists is not None else [np.zeros(0, np.int64)] * n)]
    used = np.zeros((n, C), np.int64)
    out_w = np.full((n, days, k), pc.NAN_WORD, np.uint32)
    out_i = np.full((n, days, k), -1, np.int64)
    for d in range(days):
        today = np.stack([pc.day_caps(caps[j], None if plan is None else np.broadcast_to(plan, (n, C))[j], used[j]) for j in range(n)])
        w, i = _filtered(eng, users, today, k, [np.sort(x) for x in had], slate)
        out_w[:, d], out_i[:, d] = w, i
        if (i < 0).all():
            break
        for j in range(n):
            took = i[j][i[j] >= 0]
            used[j] += pc.used_by(sig, took, C)
            had[j] = np.concatenate([had[j], took])
    return out_w, out_i


def _matrix(eng, U, user_base=0):
    """the engine's own m2d_score_slate words of every user for every dish: float32 [U, I]"""
    out = eng.score_slate(_dev(np.arange(U, dtype=np.int32) + user_base), _dev(np.arange(eng.I, dtype=np.int32)))
    eng.check()
    return out.cpu().numpy()


def _same(got, want, what=""):
    a, b = np.asarray(got[1], np.int64), np.asarray(want[1], np.int64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: ids of %d rows differ" % (what, int((a != b).reshape(len(a), -1).any(1).sum()))
    assert np.array_equal(np.asarray(got[0], np.uint32), np.asarray(want[0], np.uint32)), "%s: score words differ" % what


def _t(x):
    s, i = x
    return dc.words(s.cpu().numpy()), i.cpu().numpy().astype(np.int64)


def _recipe(name):
    kind, C, E, I = name
    return mc.exact_recipe(C, E, I) if kind == "exact" else mc.normal_recipe(C, E, I)


def _day_cap(k):
    return max(1, (k + 1) // 2)


# ---- 1. and 2. against the engine's own composition, and against the restatement -------------------------------------------------------
RECIPES = (("exact", 3, 64, 1300), ("exact", 4, 4, 257), ("exact", 4, 200, 257), ("exact", 4, 64, 255), ("normal", 6, 64, 1300),
           ("normal", 6, 200, 1300), ("normal", 6, 64, 16385))


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("recipe", RECIPES, ids=lambda n: "%s-C%d-E%d-I%d" % n)
def test_plans_are_the_composition_of_filtered_menus_and_the_restatement(recipe, shape):
    """without filters and plan caps (uncapped days and capped ones); with plan caps and exclusion segments of 0 / 1 / 65 / 300 ids;
    with both over a slate"""
    r = _recipe(recipe)
    days, k = shape
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, users, n = S[r.users], r.users, len(r.users)
    slate = mf.slate_of(r.I, max(r.I // 2, 1))
    plan = pc.plan_caps_of(n, r.C, days, k)
    caps = mc.caps_all(n, r.C, _day_cap(k))
    lists = mf.own_menu_lists(W32, r.cats, caps, k, sizes=(0, 1, 65, 300))
    long = days * k > 256 and r.I > 1300                     # (the composition is D calls: the longest plans once per recipe)
    for cp, pl, ls, sl in ((mc.caps_uncapped(n, r.C, k), None, None, None), (caps, None, None, None), (caps, plan, lists, None),
                           (caps, plan, lists, slate))[1 if long else 0:]:
        got = _plan(eng, users, cp, days, k, pl, ls, sl)
        what = "%s %dx%d plan %s lists %s slate %s" % (recipe, days, k, pl is not None, ls is not None, sl is not None)
        _same(got, _compose(eng, r.sig, users, cp, days, k, pl, ls, sl), what + ": the composition")
        want = pc.plan_lists(W32, r.cats, cp, pl, days, k, ls, sl)
        _same(got, want, what + ": the restatement")
        if days * k <= 192:
            _same(got, pc.merged_plan(W32, r.cats, cp, pl, days, k, ls, sl, W=mf.RANGE_W), what + ": the merged form")
        took = got[1][got[1] >= 0]
        assert days == 1 or (got[1][:, 1:] >= 0).any()       # the later days hold dishes
        for j in range(n):                                   # no dish twice in a plan, none of the excluded
            row = got[1][j][got[1][j] >= 0]
            assert len(np.unique(row)) == len(row) and (ls is None or not np.isin(row, ls[j]).any())
        if pl is not None and days > 1:
            assert pc.differs(want, pc.plan_lists(W32, r.cats, cp, None, days, k, ls, sl)).any(), what + ": the plan caps bind nothing"
        assert len(took)
    eng.close()


@pytest.mark.parametrize("nD", (1, 63, 65, 1300))
def test_plans_over_slates_of_every_size(nD):
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, users, n = S[r.users], r.users, len(r.users)
    slate = mf.slate_of(r.I, nD, seed=nD)
    for days, k in ((7, 3), (13, 5), (3, 64)):
        caps, plan = mc.caps_all(n, 6, _day_cap(k)), pc.plan_caps_of(n, 6, days, k)
        lists = mf.own_menu_lists(W32, r.cats, caps, k, slate, sizes=(0, 1, 65, 300), seed=nD)
        for pl, ls in ((None, None), (plan, lists)):
            got = _plan(eng, users, caps, days, k, pl, ls, slate)
            _same(got, _compose(eng, r.sig, users, caps, days, k, pl, ls, slate), "nD = %d, %dx%d: the composition" % (nD, days, k))
            _same(got, pc.plan_lists(W32, r.cats, caps, pl, days, k, ls, slate), "nD = %d, %dx%d: the restatement" % (nD, days, k))
    eng.close()


# ---- 3. list edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((8, 8), (13, 5), (65, 1)), ids=lambda s: "%dx%d" % s)
def test_segments_of_0_1_63_64_65_dishes_under_lists_of_64_and_65(shape):
    """a cursor runs off a short list; a list ends in -1 before L; a list of exactly L; a segment one dish longer than L"""
    r = mc.segment_recipe()
    days, k = shape
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, users, n = S[r.users], r.users, len(r.users)
    only = np.flatnonzero(np.isin(r.sig, list(mc.SEGMENT_SIZES))).astype(np.int32)      # the planted segments alone: every list is read to its end
    assert len(only) == 1 + 63 + 64 + 65
    for caps in (mc.caps_uncapped(n, 4, k), mc.caps_all(n, 4, _day_cap(k))):
        for sl in (None, only):
            want = pc.plan_lists(W32, r.cats, caps, None, days, k, None, sl)
            for select in ((0, 1) if days * k <= 64 else (0,)):
                eng.set_option("menu_select", select)
                _same(_plan(eng, users, caps, days, k, None, None, sl), want, "%dx%d select %d" % (days, k, select))
            eng.set_option("menu_select", 0)
        if caps[0, 0] == k:                                  # uncapped over the planted segments: all 193 dishes, then nothing
            assert ((want[1] >= 0).sum((1, 2)) == min(days * k, len(only))).all()
    eng.close()


def test_fewer_admissible_dishes_than_the_plan_asks_for():
    """a short day followed by empty days; days k above I and above nD"""
    r = mc.exact_recipe(4, 64, 255)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    W32, users, n = S[r.users], r.users, len(r.users)
    for days, k, caps, sl in ((16, 64, mc.caps_uncapped(n, 4, 64), None), (1024, 1, mc.caps_uncapped(n, 4, 1), None),
                              (7, 3, mc.caps_uncapped(n, 4, 3), mf.slate_of(r.I, 17)), (5, 10, mc.caps_zero_on(n, 4, 10, 0), mf.slate_of(r.I, 40)),
                              (9, 7, mc.caps_all(n, 4, 0), None)):
        nD = r.I if sl is None else len(sl)
        got = _plan(eng, users, caps, days, k, None, None, sl)
        assert ((got[1] >= 0).sum((1, 2)) < days * k).all()   # no user's plan is full
        _same(got, pc.plan_lists(W32, r.cats, caps, None, days, k, None, sl), "%dx%d over %d dishes" % (days, k, nD))
        took = (got[1] >= 0).sum(2)
        if caps.min() > 0:
            assert (took.sum(1) == nD).all()                 # uncapped: every dish once, the NaN dishes included
        for j in range(n):
            first_short = int(np.argmax(took[j] < k))
            assert took[j][first_short] < k and (took[j][first_short + 1:] == 0).all()
        if k > 1 and caps.min() > 0:
            assert (took % k != 0).any()                     # a day that is short but not empty
    plan = np.full((n, 4), 2, np.int32)                      # the plan caps end the plan: at most 2 per category, then only the empty masks
    got = _plan(eng, users, mc.caps_all(n, 4, 2), 6, 4, plan)
    _same(got, pc.plan_lists(W32, r.cats, mc.caps_all(n, 4, 2), plan, 6, 4), "plan caps of 2")
    for j in range(n):
        row = got[1][j][got[1][j] >= 0]
        assert (pc.used_by(r.sig, row, 4) <= 2).all() and (got[1][j][-1] == -1).all()
    eng.close()


# ---- 4. the launcher's cuts ----------------------------------------------------------------------------------------------------------------
def _block_rows(P, sig, L):
    """the launcher's user block for a catalogue-wide call"""
    sizes = np.bincount(np.asarray(sig, np.int64), minlength=64)
    sizes = sizes[sizes > 0]
    Wmax = int(np.minimum(np.minimum(sizes, P), 65536).max())
    return max(1, P // max(Wmax, len(sizes) * L))


@pytest.mark.parametrize("shape", ((7, 3), (8, 8), (13, 5), (16, 64)), ids=lambda s: "%dx%d" % s)
def test_the_plans_do_not_depend_on_the_launchers_cut_or_the_selection(shape):
    """deep_chunk_pairs 256 (ranges narrower than L, P < S' L: blocks of one user), 2 048 and the default; menu_select 0 / 1 at
    L <= 64; nU = 1 / 5 / 4 blocks + 1; repeated users"""
    r = mc.edge_recipe()
    days, k = shape
    L = days * k
    eng = _engine(r)
    S = _matrix(eng, r.U)
    blocks = _block_rows(2048, r.sig, L)
    assert _block_rows(256, r.sig, L) == 1 and 256 < len(set(r.sig.tolist())) * L or L <= 21
    users = np.resize(r.users, 4 * blocks + 1).astype(np.int32)      # 4 full blocks at P = 2 048 and a block of one row; users repeat
    n = len(users)
    W32 = S[users]
    caps, plan = mc.caps_mixed(n, 4, hi=_day_cap(k) + 1), pc.plan_caps_of(n, 4, days, k, seed=1)
    lists = mf.own_menu_lists(W32, r.cats, caps, k, sizes=(0, 1, 65, 300))
    want = pc.plan_lists(W32, r.cats, caps, plan, days, k, lists)
    assert pc.differs(want, pc.plan_lists(W32, r.cats, caps, None, days, k, lists)).any()
    for P in (256, 2048, dc.DEFAULT_P):
        eng.set_option("deep_chunk_pairs", P)
        for select in ((0, 1) if L <= 64 else (0,)):
            eng.set_option("menu_select", select)
            _same(_plan(eng, users, caps, days, k, plan, lists), want, "P = %d, menu_select = %d" % (P, select))
        eng.set_option("menu_select", 0)
        for rows in ([0], [n - 1], [3, 3, 3, 0, 7 % n], list(range(5))):
            sub = (want[0][rows], want[1][rows])
            _same(_plan(eng, users[rows], caps[rows], days, k, plan[rows], [lists[j] for j in rows]), sub, "P = %d, rows %s" % (P, rows))
    eng.close()


def test_a_user_base_shard():
    r = mc.normal_recipe(6, 64, 1300)
    base = 1000
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, user_base=base)
    users = np.asarray([3, 3, 3, 0, 7, 3, 0], np.int32)
    n = len(users)
    caps, plan = mc.caps_mixed(n, 6, seed=4), pc.plan_caps_of(n, 6, 7, 3, seed=4)
    slate = mf.slate_of(r.I, 700)
    lists = mf.own_menu_lists(S[users], r.cats, caps, 3, slate)
    _same(_plan(eng, users + base, caps, 7, 3, plan, lists, slate), pc.plan_lists(S[users], r.cats, caps, plan, 7, 3, lists, slate), "a shard")
    eng.close()


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", mc.TIE_GROUPS)
def test_tied_copies_in_two_segments_straddle_a_day_boundary(group):
    """menu_cases' twin-category recipe: bit-equal words under the masks {0} and {1}.  Day 1 ends inside the tie group: the lower ids
    go to the earlier day.  The all-zero user: one tie group over every segment."""
    r = mc.tie_recipe(group)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    w = dc.words(S)
    assert (w[:, r.copies] == w[:, r.copies[:1]]).all() and sorted(set(r.sig[r.copies])) == [1, 2]
    for j, u in enumerate(r.users):
        k = r.k[j]
        for days in (2, 3):
            for caps, plan in ((mc.caps_uncapped(1, 4, k), None), (np.asarray([[k, max(k // 2, 1), k, k]], np.int32), None),
                               (mc.caps_uncapped(1, 4, k), np.asarray([[days * k, k + 1, days * k, days * k]], np.int32))):
                want = pc.plan_lists(S[u:u + 1], r.cats, caps, plan, days, k)
                _same(_plan(eng, [u], caps, days, k, plan), want, "group %d, user %d, %d days" % (group, u, days))
                _same(_compose(eng, r.sig, [u], caps, days, k, plan), want, "the composition")
        if j < len(r.users) - 1:
            free = pc.plan_lists(S[u:u + 1], r.cats, mc.caps_uncapped(1, 4, k), None, 2, k)[1][0]
            a, b = free[0][np.isin(free[0], r.copies)], free[1][np.isin(free[1], r.copies)]
            assert len(a) and len(b) and a.max() < b.min()   # copies on both days, the lower ids on the first
        else:
            free = pc.plan_lists(S[u:u + 1], r.cats, mc.caps_uncapped(1, 4, k), None, 2, k)[1][0]
            real = np.flatnonzero(r.sig != 0)
            assert free.ravel().tolist() == real[:2 * k].tolist()      # the all-zero user: the lowest ids, in id order over the days
    eng.close()


def test_a_tie_group_across_position_L_of_a_list():
    """65 bit-equal copies, half in segment {0} and half in {1}: L = days k is chosen so that position L of segment {0}'s own list lies
    inside its run of copies -- the list of L holds the lower ids of the run -- and the plan reads that list to its end"""
    r = mc.tie_recipe(65)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    hit = 0
    for u in r.users[:-1]:
        seg = np.flatnonzero(r.sig == 1)
        order = mc.order_of(dc.words(S[u])[seg], seg)
        run = np.flatnonzero(np.isin(order, r.copies))
        lo, hi = int(run[0]), int(run[-1])
        for days, k in ((2, 32), (3, 16), (5, 8), (13, 5), (4, 4), (7, 3), (2, 8), (5, 2)):
            L = days * k
            if not lo < L <= hi:
                continue
            hit += 1
            # only segment {0} may be taken from: every other category is closed, so the plan is that segment's list of L, day by day
            caps = np.asarray([[k, 0, 0, 0]], np.int32)
            want = pc.plan_lists(S[u:u + 1], r.cats, caps, None, days, k)
            assert want[1].ravel().tolist() == order[:L].tolist()
            for P in (256, dc.DEFAULT_P):
                eng.set_option("deep_chunk_pairs", P)
                _same(_plan(eng, [u], caps, days, k), want, "user %d, L = %d, P = %d" % (u, L, P))
    assert hit >= 3
    eng.close()


# ---- 6. equality with the filtered call -------------------------------------------------------------------------------------------------------
def test_one_day_without_plan_caps_is_the_filtered_call_and_plan_caps_of_days_k_bind_nothing():
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    n = len(r.users)
    slate = mf.slate_of(r.I, 700)
    for caps, k in ((mc.caps_all(n, 6, 2), 10), (mc.caps_mixed(n, 6), 64)):
        lists = mf.own_menu_lists(S[r.users], r.cats, caps, k, slate)
        for P in (256, dc.DEFAULT_P):
            eng.set_option("deep_chunk_pairs", P)
            for ls, sl in ((None, None), (lists, None), (lists, slate)):
                w, i = _filtered(eng, r.users, caps, k, ls, sl)
                kernel = eng.last_kernel()
                _same(_plan(eng, r.users, caps, 1, k, None, ls, sl), (w[:, None], i[:, None]), "days = 1, P = %d" % P)
                assert eng.last_kernel() == kernel == "m2d_menu_merge"
                _same(_plan(eng, r.users, caps, 1, k, np.full((n, 6), k), ls, sl), (w[:, None], i[:, None]), "days = 1, plan caps of k")
                assert eng.last_kernel() == "m2d_plan_merge"
    for days, k in ((7, 3), (13, 5), (16, 64)):
        caps = mc.caps_all(n, 6, _day_cap(k))
        free = _plan(eng, r.users, caps, days, k, None, lists, slate)
        _same(_plan(eng, r.users, caps, days, k, np.full((n, 6), days * k), lists, slate), free, "plan caps of days k, %dx%d" % (days, k))
        assert eng.last_kernel() == "m2d_plan_merge"
    eng.close()


# ---- 7. errors and refusals -----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from foodrec_amd import _native
    r = mc.exact_recipe(4, 64, 257)
    eng = _engine(r)
    n = len(r.users)
    caps = mc.caps_all(n, 4, 2)
    lists = [np.asarray([1, 2], np.int64)] * n
    slate = mf.slate_of(r.I, 100)
    bad = _native.M2D_ERR_INVALID_ARG
    for k in (0, 65, -3, 1024):
        assert _abi(eng, r.users, caps, 1, k, None, lists, slate)[0] == bad and NAME + ": need nU >= 0 and 1 <= k <= min(64, I)" in eng_error(eng)
    for days, k in ((0, 5), (-1, 5), (205, 5), (1025, 1), (17, 64), (2 ** 31 - 1, 64)):
        assert _abi(eng, r.users, caps, days, k, None, lists, slate)[0] == bad
        assert eng_error(eng) == NAME + ": need days >= 1 and days * k <= M2D_PLAN_MAX_LIST = 1024", (days, k)
    for nD in (0, -1, r.I + 1):
        assert _abi(eng, r.users, caps, 2, 5, None, lists, slate, nD=nD)[0] == bad and eng_error(eng) == NAME + ": with a slate need 1 <= nD <= I"
    assert _abi(eng, r.users, caps, 2, 5, None, lists, slate, null=("excl_ids",))[0] == bad and eng_error(eng) == NAME + ": excl_off without excl_ids"
    for null in ("users", "caps", "scores", "out_ids"):
        assert _abi(eng, r.users, caps, 2, 5, caps, lists, slate, null=(null,))[0] == bad and eng_error(eng) == NAME + ": null buffer"
    assert _abi(eng, np.zeros(0, np.int32), caps[:0], 3, 5, None, [], slate)[0] == 0 and _latched(eng)[0] == 0       # nU == 0: nothing is launched
    S = _matrix(eng, r.U)
    for days, k in ((1024, 1), (16, 64), (204, 5)):          # the largest plans are in range
        _same(_plan(eng, r.users, caps, days, k, None, lists, slate), pc.plan_lists(S[r.users], r.cats, caps, None, days, k, lists, slate))
    eng.close()
    bare = _engine(r, masks=False)
    assert _abi(bare, r.users, caps, 2, 5, None, lists, slate)[0] == _native.M2D_ERR_NOT_CONFIGURED
    bare.close()


def test_bad_caps_plan_caps_users_lists_and_slates_are_latched_with_value_and_position():
    from foodrec_amd import _native
    r = mc.normal_recipe(6, 64, 1300)
    base = 100
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, user_base=base)
    users, n = r.users + base, len(r.users)
    days, k = 7, 3
    caps, plan = mc.caps_mixed(n, 6, seed=2), pc.plan_caps_of(n, 6, days, k, seed=2)
    slate = mf.slate_of(r.I, 257)
    lists = mf.own_menu_lists(S[r.users], r.cats, caps, k, slate)
    want = pc.plan_lists(S[r.users], r.cats, caps, plan, days, k, lists, slate)
    _same(_plan(eng, users, caps, days, k, plan, lists, slate), want)
    off, ids = mf.csr(lists)

    def filtered_reports(**kw):                              # what m2d_topk_menu_filtered latches for the same inputs
        assert _abi(eng, users, caps, 1, k, None, filtered=True, **kw)[0] == 0
        return _latched(eng)

    for P in (dc.DEFAULT_P, 256):
        eng.set_option("deep_chunk_pairs", P)
        for row in (0, n // 2, n - 1):
            ok = np.setdiff1d(np.arange(n), [row])
            for which, position in (("caps", row * 6 + 4), ("plan", n * 6 + row * 6 + 4)):
                c, p = caps.copy(), plan.copy()
                (c if which == "caps" else p)[row, 4] = -3
                rc, s, i = _abi(eng, users, c, days, k, p, lists, slate)
                assert rc == 0 and _latched(eng) == (_native.M2D_ERR_INVALID_ARG, -3, position), (which, row)
                _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), "the other users' rows")
                (c if which == "caps" else p)[row, 4] = 0    # a latched cap counts as 0
                _same((s, i), _plan(eng, users, c, days, k, p, lists, slate), "a cap below 0 counts as 0")
            u = users.copy(); u[row] = base + r.U
            rc, s, i = _abi(eng, u, caps, days, k, plan, lists, slate)
            assert rc == 0 and _latched(eng) == (_native.M2D_ERR_BAD_USER_ID, base + r.U, row)
            _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), "the other users' rows")
    at = int(off[4]) - 1
    for pos, value in ((at, r.I), (at, -1), (at, int(ids[at - 1]) - 1), (len(ids) - 1, 2 ** 31 - 1)):
        x = ids.copy(); x[pos] = value
        for sl in (None, slate):
            assert _abi(eng, users, caps, days, k, plan, raw=(off, x), slate=sl)[0] == 0
            got = _latched(eng)
            assert got[0] != 0 and got == filtered_reports(raw=(off, x), slate=sl), (pos, value, got)
    for q, value in ((0, 1), (4, int(off[3]) - 1), (n, int(off[n - 1]) - 1)):
        o = off.copy(); o[q] = value
        assert _abi(eng, users, caps, days, k, plan, raw=(o, ids), slate=slate)[0] == 0
        got = _latched(eng)
        assert got[0] != 0 and got == filtered_reports(raw=(o, ids), slate=slate), (q, value, got)
    for pos, value in ((0, -1), (100, r.I), (256, 2 ** 31 - 1), (64, int(slate[63])), (256, int(slate[255]) - 1)):
        sl = slate.copy(); sl[pos] = value
        assert _abi(eng, users, caps, days, k, plan, lists, sl)[0] == 0
        got = _latched(eng)
        code = _native.M2D_ERR_BAD_ITEM_ID if not 0 <= value < r.I else _native.M2D_ERR_INVALID_ARG
        assert got == (code, value, pos) == filtered_reports(lists=lists, slate=sl), (pos, value, got)
    _same(_plan(eng, users, caps, days, k, plan, lists, slate), want, "after the latched errors")
    eng.close()


def test_refusals_name_the_call():
    from foodrec_amd import _native
    rng = np.random.default_rng(2)
    r7 = mc.normal_recipe(7, 64, 300)
    eng = _engine(r7)
    assert _abi(eng, r7.users, mc.caps_all(len(r7.users), 7, 2), 3, 5, slate=np.arange(10))[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng).startswith(NAME + ": more than 6 categories")
    eng.close()
    r = dc.normal_recipe(64, I=300, U=8, seed=1, head=False)
    eng = _engine(r)
    users = np.arange(r.U, dtype=np.int32)
    caps = mc.caps_all(r.U, 4, 2)
    slate, lists = mf.slate_of(r.I, 100), [np.asarray([3, 9], np.int64)] * r.U
    want = _plan(eng, users, caps, 7, 3, caps, lists, slate)
    nnz = 3 * r.I
    eng.set_ingredients((rng.standard_normal((50, r.E)) / 8).astype(np.float32), np.arange(0, nnz + 1, 3, dtype=np.int32),
                        rng.integers(0, 50, nnz).astype(np.int32))
    for kw in (dict(), dict(lists=lists), dict(slate=slate), dict(plan=caps)):
        for days in (1, 7):
            assert _abi(eng, users, caps, days, 3, **kw)[0] == _native.M2D_ERR_UNSUPPORTED
            assert eng_error(eng) == NAME + ": the ingredient table is set (not supported)"
    eng.clear_ingredients()
    keep = eng.re[7, 3].item()
    eng.re[7, 3] = float("inf")
    eng.tables_updated()
    assert _abi(eng, users, caps, 7, 3, caps, lists, slate)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng) == NAME + ": needs finite tables (a table value is not finite)"
    eng.re[7, 3] = keep
    eng.tables_updated()
    _same(_plan(eng, users, caps, 7, 3, caps, lists, slate), want, "after the value was put back")
    eng.close()


# ---- 8. surroundings ---------------------------------------------------------------------------------------------------------------------------
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
        out = [_t(eng._topk_menu(users, 10, _dev(caps))), _filtered(eng, r.users, caps, 10, lists, slate),
               _t(eng.topk_users_deep(users, 300, (off, ids))), _t(eng.topk_users(users, 10))]
        eng.check()
        return out

    before = existing()
    for sl in (None, slate):
        _plan(eng, r.users, caps, 7, 3, None, lists, sl)
        _plan(eng, r.users, mc.caps_mixed(n, 4), 16, 64, caps, lists, sl)
    assert _abi(eng, r.users, caps, 17, 64, None, lists, slate)[0] == _native.M2D_ERR_INVALID_ARG       # a refused call
    bad = slate.copy(); bad[5] = r.I                                                                     # four failed ones
    assert _abi(eng, r.users, caps, 7, 3, None, lists, bad)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_ITEM_ID
    x = [np.asarray([5, 4], np.int64)] * n
    assert _abi(eng, r.users, caps, 7, 3, None, x, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_INVALID_ARG
    u = r.users.copy(); u[3] = r.U
    assert _abi(eng, u, caps, 7, 3, None, lists, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_USER_ID
    assert _abi(eng, r.users, caps, 7, 3, -caps, lists, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_INVALID_ARG
    for a, b in zip(before, existing()):
        _same(a, b, "an existing call moved")
    eng.close()


def test_plans_follow_write_memory_tables_updated_and_new_masks():
    import torch
    b = dc.normal_recipe(64, I=500, U=16, seed=2, head=False)
    rng = np.random.default_rng(8)
    eng = _engine(b, tables=(b.PM.copy(), b.RE.copy(), b.CE.copy()))
    users = np.arange(b.U, dtype=np.int32)
    caps, plan = mc.caps_all(b.U, 4, 2), pc.plan_caps_of(b.U, 4, 7, 3)
    slate = mf.slate_of(b.I, 300)
    t = lambda a: torch.as_tensor(a, device="cuda")         # noqa: E731
    cats = [b.cats]

    def check(before, what):
        S = _matrix(eng, b.U)
        lists = mf.own_menu_lists(S, cats[0], caps, 3, slate)
        _same(_plan(eng, users, caps, 7, 3, plan, lists, slate), pc.plan_lists(S, cats[0], caps, plan, 7, 3, lists, slate), what)
        free = _plan(eng, users, caps, 7, 3, plan)
        _same(free, pc.plan_lists(S, cats[0], caps, plan, 7, 3), what + ", the catalogue")
        assert before is None or not pc.same(before, free), what + " changed nothing"
        return free

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
    cats[0] = np.roll(b.cats, 1, axis=1)                     # other signatures for the same dishes: the index is rebuilt
    assert (mc.signatures(cats[0]) != mc.signatures(b.cats)).mean() > 0.5
    eng.dish_cats.copy_(t(cats[0]))                          # the masks change in place: tables_updated names them
    eng.tables_updated()
    state = check(state, "tables_updated with changed masks")
    cats[0] = b.cats
    eng.set_dish_categories(cats[0])
    check(state, "the first masks again")
    eng.close()


def test_inputs_that_arrive_late_on_a_side_stream():
    """Stream order: on a side stream a blocker (matrix products), then the copies that put the real caps, plan caps, exclusion lists
    and slate where decoys stood, then the call -- entered while the blocker runs.  The plans are the real request's, on an engine
    whose first menu call this is and again on the warmed engine."""
    import torch
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    n = len(r.users)
    days, k = 7, 3
    twin = _engine(r)
    S = _matrix(twin, r.U)
    caps = (mc.caps_all(n, 6, 2), mc.caps_all(n, 6, 1))
    plans = (pc.plan_caps_of(n, 6, days, k, seed=1), pc.plan_caps_of(n, 6, days, k, seed=2))
    slates = (mf.slate_of(r.I, 700, seed=1), mf.slate_of(r.I, 700, seed=2))
    lists = [mf.own_menu_lists(S[r.users], r.cats, caps[j], k, sl, sizes=(65,), seed=j) for j, sl in enumerate(slates)]
    want, other = (_plan(twin, r.users, caps[j], days, k, plans[j], lists[j], slates[j]) for j in (0, 1))
    twin.close()
    assert pc.differs(want, other).mean() >= 0.9             # the decoy's answer is another one
    (off, ids), (doff, dids) = mf.csr(lists[0]), mf.csr(lists[1])
    assert len(ids) == len(dids)
    a = torch.randn((8192, 8192), device="cuda")
    side = torch.cuda.Stream()
    src = [_dev(x) for x in (off, ids, slates[0], caps[0], plans[0])]
    ut = _dev(r.users)
    for episode in ("first use", "warmed"):
        bufs = [_dev(x) for x in (doff, dids, slates[1], caps[1], plans[1])]
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(6):
                a @ a
            for b, s in zip(bufs, src):
                b.copy_(s, non_blocking=True)
            arrived = torch.cuda.Event()
            arrived.record(side)
            late = not arrived.query()                        # the copies had not landed when the call was made
            got = torch.ops.m2d.plan_menus(eng.id, ut, bufs[3], days, k, bufs[4], bufs[0], bufs[1], bufs[2])
            side.synchronize()
            eng.check()
        assert late, "the blocker was too short to show anything"
        _same(_t(got), want, "side stream, " + episode)
    eng.close()


def test_torch_op_and_the_model():
    import types
    import torch
    import foodrec_amd
    r = dc.normal_recipe(64, head=False)
    eng = _engine(r)
    n = len(r.users)
    days, k = 7, 3
    caps, plan = mc.caps_mixed(n, 4), pc.plan_caps_of(n, 4, days, k)
    S = _matrix(eng, r.U)
    slate = mf.slate_of(r.I, 300)
    lists = mf.own_menu_lists(S[r.users], r.cats, caps, k, slate)
    off, ids = (_dev(x) for x in mf.csr(lists))
    want = _plan(eng, r.users, caps, days, k, plan, lists, slate)
    op = torch.ops.m2d.plan_menus
    got = op(eng.id, _dev(r.users), _dev(caps), days, k, _dev(plan), off, ids, _dev(slate))
    assert tuple(got[0].shape) == tuple(got[1].shape) == (n, days, k) and got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    _same(_t(got), want, "torch.ops.m2d.plan_menus")
    _same(_t(op(eng.id, _dev(r.users), _dev(caps), days, k)), _plan(eng, r.users, caps, days, k), "the op without filters or plan caps")
    one = np.asarray([2, 0, 1, 3], np.int32)                  # a single row is broadcast, in either table
    _same(_t(op(eng.id, _dev(r.users), _dev(one), 5, 4, _dev(one + 3), among=_dev(slate))),
          _plan(eng, r.users, np.tile(one, (n, 1)), 5, 4, np.tile(one + 3, (n, 1)), None, slate), "tables [C]")
    _same(_t(eng._plan_menus(_dev(r.users), days, k, _dev(caps), _dev(plan), [x.tolist() for x in lists], _dev(slate))), want, "host lists")
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        eng._plan_menus(_dev(r.users), 2, 65, _dev(one))
    with pytest.raises(ValueError, match="days >= 1 and days \\* k <= 1024"):
        eng._plan_menus(_dev(r.users), 17, 64, _dev(one))
    with pytest.raises(TypeError):
        eng._plan_menus(_dev(r.users), 2, 5, _dev(one), _dev(one.astype(np.int64)))
    with pytest.raises(ValueError, match="at least one dish"):
        eng._plan_menus(_dev(r.users), 2, 5, _dev(one), among=_dev(slate[:0]))
    eng.close()

    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    who = [str(u) for u in r.users]                          # ids as the reference feeds them: str
    had = {who[j]: [str(d) for d in lists[j][::-1]] for j in range(n) if j % 2 == 0}           # a dict: any order, repeats, missing keys
    by_row = [np.unique(np.asarray(had.get(u, []), np.int64)) for u in who]
    cap2 = np.tile(np.asarray([k, 2, k, 0], np.int32), (n, 1))
    plan2 = np.tile(np.asarray([4, days * k, days * k, days * k], np.int32), (n, 1))
    s, i = model.plan_menus(who, days, k, {1: 2, 3: 0}, {0: 4}, exclude=had, among=[str(d) for d in slate[::-1]] + [str(slate[0])])
    assert s.dtype == np.float32 and i.dtype == np.int32 and s.shape == i.shape == (n, days, k)
    _same((dc.words(s), i), _plan(model.engine, r.users, cap2, days, k, plan2, by_row, slate), "Model.plan_menus, dicts and among")
    s, i = model.plan_menus(who, days, k, {1: 2, 3: 0}, exclude=by_row)
    _same((dc.words(s), i), _plan(model.engine, r.users, cap2, days, k, None, by_row), "Model.plan_menus, a list, no slate, no plan caps")
    s, i = model.plan_menus(who)                             # nothing given: 7 days of 3, the first 21 of the order
    deep = _t(model.engine.topk_users_deep(_dev(r.users), 21))
    _same((dc.words(s).reshape(n, 21), i.reshape(n, 21)), deep, "Model.plan_menus, nothing given")
    model.set_recipes({str(d): [d % 50, (7 * d) % 50] for d in range(r.I)}, 50)
    market = list(range(0, 50, 2)) + [1, 3]
    for miss in (0, 1):
        cook = model.cookable(market, miss)
        assert 0 < len(cook) < r.I
        s, i = model.plan_menus(who, days, k, {1: 2, 3: 0}, {0: 4}, exclude=had, market=market, max_missing=miss)
        _same((dc.words(s), i), _plan(model.engine, r.users, cap2, days, k, plan2, by_row, cook), "Model.plan_menus, a market")
    s, i = model.plan_menus(who, 4, 5, market=[49])
    assert len(model.cookable([49])) == 0 and (i == -1).all() and np.isnan(s).all() and i.shape == (n, 4, 5)
    with pytest.raises(ValueError, match="among together with market"):
        model.plan_menus(who, among=[1], market=market)
