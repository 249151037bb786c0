"""GPU tests of household meal plans (m2d_plan_groups; build-defined, no reference counterpart).  Oracles that
do not run the new code: (a) the restatement plan_cases.plan_lists applied to the engine's OWN m2d_score_groups_slate words over the slate
"all ids ascending", under caps folded on the host; (b) m2d_plan_menus for groups of one; (c) m2d_topk_groups / m2d_topk_groups_slate
where no cap binds.  No comparison has a tolerance: ids as integers, scores as 32-bit words (under the mean a NaN is compared as a NaN,
as tests/test_gpu_groups.py does).  The calls go through the C ABI into poisoned [nG, days, k] buffers with a guard row on either side.
The conditions the cases rely on are asserted in tests/test_plan_group_cases_cpu.py on host scores and again here, where a case
depends on them, on the engine's words."""
import ctypes

import numpy as np
import pytest

import deep_cases as dc
import group_cases as gc
import menu_cases as mc
import plan_cases as pc
import plan_group_cases as pg

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN no kernel computes; as an id: no dish
NAME = "m2d_plan_groups"
ALL_MODES = (gc.LEAST, gc.MEAN, gc.MOST)
MODE_NAMES = {v: n for n, v in gc.MODES.items()}


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


def _abi(eng, members, mode, caps, days, k, plan=None, per_member=False, lists=None, slate=None, null=(), raw=None, nD=None, M=None, flag=None):
    """One call through the C ABI -> (status, score words uint32 [nG, days, k], ids int64 [nG, days, k]); the guard rows are checked.
    caps / plan: [nG, C] or [C], with per_member [nG, M, C]; plan None: a null pointer; lists: one id list per group -> CSR; raw: an
    (offsets, ids) pair as it is; flag: caps_per_member as passed (None: per_member)."""
    import torch
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    members = np.asarray(members, np.int32)
    nG, M = members.shape[0], members.shape[1] if M is None else M
    shape = (nG, members.shape[1], eng.C) if per_member else (nG, eng.C)
    table = lambda t: _dev(np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.int32), shape)).reshape(-1) if nG else np.zeros(1, np.int32))  # noqa: E731
    mt = _dev(members.reshape(-1) if members.size else np.zeros(1, np.int32))
    ct = table(caps)
    pt = table(plan) if plan is not None else None
    off = ids = st = None
    if raw is not None or lists is not None:
        o, x = raw if raw is not None else pg.csr(lists)
        off, ids = _dev(np.asarray(o, np.int64)), _dev(np.asarray(x, np.int32) if len(x) else np.zeros(1, np.int32))
    if slate is not None:
        st = _dev(np.asarray(slate, np.int32))
        nD = len(slate) if nD is None else nD
    nd = max(int(days), 1)
    row = nd * max(int(k), 1)
    if row > 4 * pc.MAX_LIST:                                # (a refused call: nothing is written, the buffers need not hold a plan)
        nd = row = 1
    bs = torch.full(((nG + 2) * row,), POISON, dtype=torch.int32, device="cuda")
    bi = torch.full(((nG + 2) * row,), POISON, dtype=torch.int32, device="cuda")
    ptr = lambda t, name, shift=0: None if name in null or t is None else t.data_ptr() + shift      # noqa: E731
    rc = _native.lib().m2d_plan_groups(eng._h, ptr(mt, "members"), nG, M, int(mode), int(days), int(k), ptr(ct, "caps"), ptr(pt, "plan_caps"),
                                       int(per_member) if flag is None else flag, ptr(off, "excl_off"), ptr(ids, "excl_ids"),
                                       ptr(st, "slate"), int(nD or 0), ptr(bs, "scores", 4 * row), ptr(bi, "out_ids", 4 * row), _stream_ptr())
    torch.cuda.synchronize()
    s, i = bs.cpu().numpy().view(np.uint32).reshape(nG + 2, row), bi.cpu().numpy().reshape(nG + 2, row)
    assert (s[[0, -1]] == POISON).all() and (i[[0, -1]] == POISON).all(), "a guard row was written"
    out = (nG, nd, row // nd)
    return rc, s[1:-1].reshape(out), i[1:-1].astype(np.int64).reshape(out)


def _plan(eng, members, mode, caps, days, k, plan=None, per_member=False, lists=None, slate=None):
    """the plans of a call that must succeed: every element written, the id latch clear"""
    rc, s, i = _abi(eng, members, mode, caps, days, k, plan, per_member, lists, slate)
    assert rc == 0, eng_error(eng)
    eng.check()
    assert (i != POISON).all() and (s != POISON).all(), "%d elements not written" % int((i == POISON).sum())
    return s, i


def _words(eng, members, mode):
    """ORACLE (a)'s input: the engine's own m2d_score_groups_slate words over all ids ascending, float32 [nG, I]"""
    out = eng.score_groups(_dev(np.asarray(members, np.int32)), _dev(np.arange(eng.I, dtype=np.int32)), MODE_NAMES[mode])
    eng.check()
    return out.cpu().numpy()


def _want(eng, members, mode, cats, caps, days, k, plan=None, per_member=False, lists=None, slate=None, W=None):
    """ORACLE (a): plan_lists over the engine's group words, the caps folded on the host"""
    W = _words(eng, members, mode) if W is None else W
    if per_member:
        caps = pg.fold_caps(caps, members)
        plan = None if plan is None else pg.fold_caps(plan, members)
    return pc.plan_lists(W, cats, caps, plan, days, k, lists, slate)


def _same(got, want, mode=None, what=""):
    a, b = np.asarray(got[1], np.int64), np.asarray(want[1], np.int64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: ids of %d rows differ" % (what, int((a != b).reshape(len(a), -1).any(1).sum()))
    assert gc.same_words(got[0], want[0], gc.MEAN if mode == gc.MEAN else gc.LEAST), "%s: score words differ" % what


def _t(x):
    s, i = x
    return dc.words(s.cpu().numpy()), i.cpu().numpy().astype(np.int64)


def _day_cap(k):
    return max(1, (k + 1) // 2)


def _plan_menus(eng, users, caps, days, k, plan=None, lists=None, slate=None):
    """ORACLE (b): m2d_plan_menus through the engine method (tests/test_gpu_plan.py checks it)"""
    n = len(users)
    table = lambda t: _dev(np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.int32), (n, eng.C))))      # noqa: E731
    out = eng._plan_menus(_dev(np.asarray(users, np.int32)), days, k, table(caps), None if plan is None else table(plan),
                          None if lists is None else [np.asarray(x).tolist() for x in lists], None if slate is None else _dev(np.asarray(slate, np.int32)))
    eng.check()
    return _t(out)


# ---- 1. shapes against oracle (a) -------------------------------------------------------------------------------------------------------
RECIPES = ((3, 64, 1300), (4, 4, 257), (4, 200, 256), (6, 64, 255), (4, 64, 16385))


@pytest.mark.parametrize("shape", pg.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("recipe", RECIPES, ids=lambda n: "C%d-E%d-I%d" % n)
def test_plans_are_the_walk_over_the_engines_own_group_words(recipe, shape):
    """M = 1 / 2 / 3 / 8 / 64 with every count from 1 to M in one call; the caps per member (the binding row in the first, a middle or
    the last used slot, filler rows of 0 or a negative cap) with plan caps; every mode at M = 3, the modes in turn elsewhere"""
    C, E, I = recipe
    days, k = shape
    r = mc.exact_recipe(C, E, I)
    eng = _engine(r)
    turn = RECIPES.index(recipe) + pg.SHAPES.index(shape)
    bound = crossed = 0
    for q, M in enumerate(pg.MEMBER_COUNTS):
        members = gc.member_matrix(r.U, gc.words_groups(M), M, seed=turn)
        nG = len(members)
        assert set(gc.counts(members).tolist()) == set(range(1, M + 1))
        gcaps = mc.caps_mixed(nG, C, seed=turn, hi=_day_cap(k) + 1)
        gplan = pc.plan_caps_of(nG, C, days, k, seed=turn)
        slot, filler = ("first", "middle", "last")[(q + turn) % 3], (0, -7)[(q + turn) % 2]
        caps, plan = pg.spread_caps(gcaps, members, slot, filler, seed=q), pg.spread_caps(gplan, members, slot, filler, seed=q + 9)
        for mode in (ALL_MODES if M == 3 else (ALL_MODES[(q + turn) % 3],)):
            what = "C%d E%d I%d %dx%d M = %d %s" % (C, E, I, days, k, M, MODE_NAMES[mode])
            W = _words(eng, members, mode)
            got = _plan(eng, members, mode, caps, days, k, plan, True)
            want = pc.plan_lists(W, r.cats, gcaps, gplan, days, k)
            _same(got, want, mode, what)
            for g in range(nG):                              # no dish twice in a plan
                row = got[1][g][got[1][g] >= 0]
                assert len(np.unique(row)) == len(row)
            head = slice(0, 4)                               # (the conditions on a few rows: the restatement is the cost of this test)
            bound += int(pc.differs((want[0][head], want[1][head]), pc.plan_lists(W[head], r.cats, np.full(C, days * k), None, days, k)).sum())
            crossed += int(pg.crosses_a_day(want[1]).sum())
    assert bound and (days == 1 or crossed)
    eng.close()


# ---- 2. caps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES, ids=lambda m: MODE_NAMES[m])
def test_caps_per_member_give_the_rows_of_the_host_minimum(mode):
    r = mc.exact_recipe(4, 64, 1300)
    eng = _engine(r)
    members = gc.member_matrix(r.U, 13, 8)
    nG = len(members)
    cnt = gc.counts(members)
    W = _words(eng, members, mode)
    for days, k in ((1, 10), (7, 3)):
        gcaps, gplan = mc.caps_all(nG, 4, _day_cap(k)), pc.plan_caps_of(nG, 4, days, k)
        free = _plan(eng, members, mode, np.full(4, days * k), days, k)
        for gp in (None, gplan):
            per_group = _plan(eng, members, mode, gcaps, days, k, gp)
            kernel = eng.last_kernel()
            assert kernel == ("m2d_menu_merge" if days == 1 and gp is None else "m2d_plan_merge")
            _same(per_group, pc.plan_lists(W, r.cats, gcaps, gp, days, k), mode, "caps per group")
            assert pc.differs(per_group, free).any()          # a cap binds
            for slot in ("first", "middle", "last"):
                for filler in (0, -1):                       # a filler slot's row must not bind and must not latch
                    caps = pg.spread_caps(gcaps, members, slot, filler)
                    plan = None if gp is None else pg.spread_caps(gp, members, slot, filler, seed=3)
                    assert np.array_equal(pg.fold_caps(caps, members), gcaps) and (cnt < 8).any()
                    _same(_plan(eng, members, mode, caps, days, k, plan, True), per_group, mode, "the binding row in the %s slot, filler %d" % (slot, filler))
                    assert eng.last_kernel() == kernel
    # only the plan caps per member bind; a member row of "uncapped" everywhere folds to uncapped
    loose = np.full((nG, 8, 4), 21, np.int32)
    plan = pg.spread_caps(pc.plan_caps_of(nG, 4, 7, 3, seed=5), members, "last", 0)
    _same(_plan(eng, members, mode, loose, 7, 3, plan, True), pc.plan_lists(W, r.cats, np.full(4, 21), pg.fold_caps(plan, members), 7, 3), mode)
    _same(_plan(eng, members, mode, loose, 7, 3, None, True), pc.plan_lists(W, r.cats, np.full(4, 21), None, 7, 3), mode)
    eng.close()


def test_caps_below_zero_are_latched_with_value_and_position_in_both_tables_and_both_forms():
    from foodrec_amd import _native
    r = mc.exact_recipe(4, 64, 257)
    eng = _engine(r)
    M, days, k = 3, 7, 3
    members = gc.member_matrix(r.U, 7, M)
    nG = len(members)
    cnt = gc.counts(members)
    gcaps, gplan = mc.caps_mixed(nG, 4, seed=1) + 1, pc.plan_caps_of(nG, 4, days, k, seed=1)
    caps, plan = pg.spread_caps(gcaps, members, "middle", -9), pg.spread_caps(gplan, members, "last", -9)
    bad = _native.M2D_ERR_INVALID_ARG
    for mode in (gc.LEAST, gc.MEAN):
        want = _want(eng, members, mode, r.cats, caps, days, k, plan, True)
        _same(_plan(eng, members, mode, caps, days, k, plan, True), want, mode)          # negative filler rows: nothing latched
        for P in (dc.DEFAULT_P, 256):
            eng.set_option("deep_chunk_pairs", P)
            for g in (0, nG // 2, nG - 1):
                ok = np.setdiff1d(np.arange(nG), [g])
                j = int(cnt[g]) - 1
                for which, position in (("caps", (g * M + j) * 4 + 2), ("plan", nG * M * 4 + (g * M + j) * 4 + 2)):
                    c, p = caps.copy(), plan.copy()
                    (c if which == "caps" else p)[g, j, 2] = -3
                    assert pg.negative_caps(c, members) + pg.negative_caps(p, members, nG * M * 4) == [(-3, position)]
                    rc, s, i = _abi(eng, members, mode, c, days, k, p, True)
                    assert rc == 0 and _latched(eng) == (bad, -3, position), (which, g)
                    _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), mode, "the other groups' rows")
                    (c if which == "caps" else p)[g, j, 2] = 0                           # a latched cap counts as 0
                    _same((s, i), _plan(eng, members, mode, c, days, k, p, True), mode, "a cap below 0 counts as 0")
                for which, position in (("caps", g * 4 + 1), ("plan", nG * 4 + g * 4 + 1)):   # per group: the merge's latch, nG in place of nU
                    c, p = gcaps.copy(), gplan.copy()
                    (c if which == "caps" else p)[g, 1] = -2
                    rc, s, i = _abi(eng, members, mode, c, days, k, p)
                    assert rc == 0 and _latched(eng) == (bad, -2, position), (which, g)
                    _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), mode, "the other groups' rows, caps per group")
        eng.set_option("deep_chunk_pairs", dc.DEFAULT_P)
    eng.close()


# ---- 3. the launcher's cuts -------------------------------------------------------------------------------------------------------------
def _block_groups(P, sig, L, M):
    sizes = np.bincount(np.asarray(sig, np.int64), minlength=64)
    sizes = sizes[sizes > 0]
    Wmax = int(np.minimum(np.minimum(sizes, P), 65536).max())
    return max(1, P // max(M * Wmax, len(sizes) * L))


@pytest.mark.parametrize("shape", ((7, 3), (8, 8), (13, 5)), ids=lambda s: "%dx%d" % s)
def test_rows_do_not_depend_on_the_cut_the_selection_the_call_or_the_padding(shape):
    """deep_chunk_pairs 256 / 2 048 (blocks of one group) / 4 096 (three blocks and a group) / default x menu_select 0 / 1; nG = 1, 5
    and all; the groups permuted; M padded from 3 to 64"""
    r = mc.edge_recipe()
    days, k = shape
    L, M = days * k, 3
    eng = _engine(r)
    blocks = _block_groups(4096, r.sig, L, M)
    assert _block_groups(256, r.sig, L, M) == 1 and _block_groups(2048, r.sig, L, M) == 1 and blocks >= 2
    members = gc.member_matrix(r.U, 3 * blocks + 1, M, seed=2)
    nG = len(members)
    rng = np.random.default_rng(L)
    mode = ALL_MODES[L % 3]
    W = _words(eng, members, mode)
    gcaps, gplan = mc.caps_mixed(nG, 4, hi=_day_cap(k) + 1), pc.plan_caps_of(nG, 4, days, k, seed=1)
    caps, plan = pg.spread_caps(gcaps, members, "last", 0), pg.spread_caps(gplan, members, "first", -1)
    lists = pg.group_exclusions(W, r.cats, gcaps, k)
    want = pc.plan_lists(W, r.cats, gcaps, gplan, days, k, lists)
    assert pc.differs(want, pc.plan_lists(W, r.cats, np.full(4, L), None, days, k, lists)).any()
    perm = rng.permutation(nG)
    assert nG >= 7
    for P in (256, 2048, 4096, dc.DEFAULT_P):
        eng.set_option("deep_chunk_pairs", P)
        for select in ((0, 1) if L <= 64 else (0,)):
            eng.set_option("menu_select", select)
            what = "P = %d, menu_select = %d" % (P, select)
            _same(_plan(eng, members, mode, caps, days, k, plan, True, lists), want, mode, what)
            for rows in ([0], [nG - 1], list(range(5)), perm.tolist()):
                sub = (want[0][rows], want[1][rows])
                _same(_plan(eng, members[rows], mode, caps[rows], days, k, plan[rows], True, [lists[g] for g in rows]), sub, mode, what + ", rows")
        eng.set_option("menu_select", 0)
        wide = lambda t: np.concatenate([t, np.full((nG, 61, 4), -4, np.int32)], 1)      # noqa: E731
        _same(_plan(eng, pg.padded(members, 64), mode, wide(caps), days, k, wide(plan), True, lists), want, mode, "P = %d, M = 64" % P)
    eng.close()


def test_member_order_does_not_show_where_no_words_tie_and_the_sums_are_exact():
    r = mc.exact_recipe(4, 64, 1300)
    eng = _engine(r)
    members = gc.member_matrix(r.U, 11, 8, seed=3)
    other = pg.permuted_members(members)
    assert (members != other).any()
    caps = mc.caps_all(len(members), 4, 2)
    for mode in ALL_MODES:
        _same(_plan(eng, other, mode, caps, 7, 3), _plan(eng, members, mode, caps, 7, 3), mode, MODE_NAMES[mode])
    eng.close()


# ---- 4. segments and ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((8, 8), (13, 5)), ids=lambda s: "%dx%d" % s)
def test_segments_of_0_1_63_64_65_dishes_and_fewer_dishes_than_the_plan_asks_for(shape):
    r = mc.segment_recipe()
    days, k = shape
    eng = _engine(r)
    members = gc.member_matrix(r.U, 7, 3)
    nG = len(members)
    only = np.flatnonzero(np.isin(r.sig, list(mc.SEGMENT_SIZES))).astype(np.int32)
    assert len(only) == 1 + 63 + 64 + 65
    few = pg.slate_of(r.I, 17)
    for mode in ALL_MODES:
        W = _words(eng, members, mode)
        for caps in (mc.caps_uncapped(nG, 4, k), mc.caps_all(nG, 4, _day_cap(k))):
            for sl in (None, only, few):
                want = pc.plan_lists(W, r.cats, caps, None, days, k, None, sl)
                for select in ((0, 1) if days * k <= 64 else (0,)):
                    eng.set_option("menu_select", select)
                    _same(_plan(eng, members, mode, caps, days, k, None, False, None, sl), want, mode, "%dx%d select %d" % (days, k, select))
                eng.set_option("menu_select", 0)
            if caps[0, 0] == k:
                assert ((want[1] >= 0).sum((1, 2)) == 17).all()          # the last slate, uncapped: every dish once, then nothing
                took = (want[1] >= 0).sum(2)
                assert (took[:, -1] == 0).all() and (took % k != 0).any()
    none = _plan(eng, members, gc.LEAST, mc.caps_all(nG, 4, 0), 5, 4, None, False, None, only)      # nothing admissible: every row is written
    assert (none[1] == -1).all() and (none[0] == pc.NAN_WORD).all()
    eng.close()


@pytest.mark.parametrize("group", mc.TIE_GROUPS)
def test_tied_copies_in_two_segments_across_a_day_boundary_and_across_position_L(group):
    """menu_cases' twin-category recipe; a household of the same user twice scores that user's words in every mode ((x + x) / 2 is
    exact), so the tie groups are where tie_recipe put them"""
    r = mc.tie_recipe(group)
    eng = _engine(r)
    hit = 0
    for j, u in enumerate(r.users):
        k = r.k[j]
        members = np.asarray([[u, u, -1], [u, -1, -1]], np.int32)
        for mode in ALL_MODES:
            W = _words(eng, members, mode)
            w = dc.words(W)
            assert (w[:, r.copies] == w[:, r.copies[:1]]).all() and gc.same_words(w[0], w[1], gc.MEAN)
            for days in (2, 3):
                for caps, plan in ((mc.caps_uncapped(2, 4, k), None), (np.asarray([[k, max(k // 2, 1), k, k]] * 2, np.int32), None),
                                   (mc.caps_uncapped(2, 4, k), np.asarray([[days * k, k + 1, days * k, days * k]] * 2, np.int32))):
                    want = pc.plan_lists(W, r.cats, caps, plan, days, k)
                    _same(_plan(eng, members, mode, caps, days, k, plan), want, mode, "group %d, user %d, %d days" % (group, u, days))
            if j < len(r.users) - 1:
                free = pc.plan_lists(W, r.cats, mc.caps_uncapped(2, 4, k), None, 2, k)[1][0]
                a, b = free[0][np.isin(free[0], r.copies)], free[1][np.isin(free[1], r.copies)]
                assert len(a) and len(b) and a.max() < b.min()           # copies on both days, the lower ids on the first
        if group == 65 and j < len(r.users) - 1:              # position L of segment {0}'s own list inside its run of copies
            seg = np.flatnonzero(r.sig == 1)
            W = _words(eng, members, gc.LEAST)
            order = mc.order_of(dc.words(W[0])[seg], seg)
            run = np.flatnonzero(np.isin(order, r.copies))
            for days, kk in ((2, 32), (3, 16), (5, 8), (13, 5), (4, 4), (7, 3), (2, 8), (5, 2)):
                L = days * kk
                if not int(run[0]) < L <= int(run[-1]):
                    continue
                hit += 1
                caps = np.asarray([[kk, 0, 0, 0]] * 2, np.int32)
                want = pc.plan_lists(W, r.cats, caps, None, days, kk)
                assert want[1][0].ravel().tolist() == order[:L].tolist()
                for P in (256, dc.DEFAULT_P):
                    eng.set_option("deep_chunk_pairs", P)
                    _same(_plan(eng, members, gc.LEAST, caps, days, kk), want, None, "user %d, L = %d, P = %d" % (u, L, P))
    assert group != 65 or hit >= 3
    eng.close()


@pytest.mark.parametrize("recipe", ("sign", "nan"))
def test_zeros_of_both_signs_infinities_and_a_nan_in_one_member_alone(recipe):
    """group_cases' recipes: -0 against +0 in both member orders (the first-member rule shows in the listed WORD), +-inf words, a NaN
    in one member only -- the listed words are the engine's own group words, the order is theirs"""
    r, members = (gc.sign_recipe(), gc.sign_members()) if recipe == "sign" else (gc.nan_recipe(), gc.nan_members())
    eng = _engine(r)
    nG = len(members)
    seen = set()
    for mode in ALL_MODES:
        W = _words(eng, members, mode)
        seen |= set(dc.words(W).ravel().tolist())
        for days, k, caps in ((1, 8, mc.caps_uncapped(nG, 4, 8)), (4, 2, mc.caps_all(nG, 4, 1)), (3, 3, mc.caps_all(nG, 4, 2))):
            want = pc.plan_lists(W, r.cats, caps, None, days, k)
            got = _plan(eng, members, mode, caps, days, k)
            assert np.array_equal(got[1], want[1]), (recipe, mode, days, k)
            listed = got[1] >= 0
            rows = np.nonzero(listed)[0]
            assert np.array_equal(got[0][listed], dc.words(W)[rows, got[1][listed]])       # words, NaN payloads included: the engine's own
    if recipe == "sign":
        assert {0x80000000, 0x00000000, 0x7F800000, 0xFF800000} <= seen
    else:
        assert any(np.isnan(np.uint32(w).view(np.float32)) for w in seen) and {0x7F800000, 0xFF800000} <= seen
    eng.close()


# ---- 5. exclusions, slates, a shard -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nD", (1, 64, 65, 1300))
def test_exclusion_segments_of_0_1_65_300_ids_over_slates_of_every_size(nD):
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    members = gc.member_matrix(r.U, 9, 4, seed=nD)
    nG = len(members)
    slate = pg.slate_of(r.I, nD, seed=nD)
    for q, (days, k) in enumerate(((7, 3), (13, 5))):
        mode = ALL_MODES[(q + nD) % 3]
        W = _words(eng, members, mode)
        gcaps, gplan = mc.caps_all(nG, 6, _day_cap(k)), pc.plan_caps_of(nG, 6, days, k)
        caps = pg.spread_caps(gcaps, members, "middle", 0)
        lists = pg.group_exclusions(W, r.cats, gcaps, k, slate, seed=nD)
        assert sorted({len(x) for x in lists}) == [0, 1, 65, 300]
        for ls, sl in ((lists, None), (lists, slate), (None, slate)):
            got = _plan(eng, members, mode, gcaps, days, k, gplan, False, ls, sl)
            want = pc.plan_lists(W, r.cats, gcaps, gplan, days, k, ls, sl)
            _same(got, want, mode, "nD = %d, %dx%d" % (nD, days, k))
            _same(_plan(eng, members, mode, caps, days, k, None, True, ls, sl), pc.plan_lists(W, r.cats, gcaps, None, days, k, ls, sl), mode,
                  "caps per member, nD = %d" % nD)
            for g in range(nG):
                row = got[1][g][got[1][g] >= 0]
                assert ls is None or not np.isin(row, ls[g]).any()
                assert sl is None or np.isin(row, sl).all()
    eng.close()


def test_a_user_base_shard():
    r = mc.normal_recipe(6, 64, 1300)
    base = 1000
    eng = _engine(r, user_base=base)
    members = gc.member_matrix(r.U, 7, 3, user_base=base)
    gcaps, gplan = mc.caps_mixed(7, 6, seed=4), pc.plan_caps_of(7, 6, 7, 3, seed=4)
    slate = pg.slate_of(r.I, 700)
    for mode in ALL_MODES:
        W = _words(eng, members, mode)
        lists = pg.group_exclusions(W, r.cats, gcaps, 3, slate)
        _same(_plan(eng, members, mode, pg.spread_caps(gcaps, members, "last"), 7, 3, pg.spread_caps(gplan, members, "first"), True, lists, slate),
              pc.plan_lists(W, r.cats, gcaps, gplan, 7, 3, lists, slate), mode, "a shard")
    eng.close()


# ---- 6. equalities (b) and (c) --------------------------------------------------------------------------------------------------------------
def test_a_group_of_one_is_plan_menus_row_for_that_user_in_every_mode():
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    users = r.users
    n = len(users)
    slate = pg.slate_of(r.I, 700)
    for M in (1, 5):
        members = pg.padded(users[:, None], M)
        for days, k, plan in ((1, 10, None), (7, 3, None), (7, 3, pc.plan_caps_of(n, 6, 7, 3)), (16, 64, pc.plan_caps_of(n, 6, 16, 64))):
            caps = mc.caps_mixed(n, 6, hi=_day_cap(k) + 1)
            base = _plan_menus(eng, users, caps, days, k, plan)
            lists = [np.asarray(sorted(set(base[1][j].ravel()[:3].tolist()) - {-1}), np.int64) for j in range(n)]    # each user's best three
            for ls, sl in ((None, None), (lists, slate)):
                want = _plan_menus(eng, users, caps, days, k, plan, ls, sl)
                kernel = eng.last_kernel()
                assert kernel == ("m2d_menu_merge" if days == 1 and plan is None else "m2d_plan_merge")
                for mode in ALL_MODES:
                    _same(_plan(eng, members, mode, caps, days, k, plan, False, ls, sl), want, None, "M = %d, %dx%d, %s" % (M, days, k, MODE_NAMES[mode]))
                    assert eng.last_kernel() == kernel
                    wide = lambda t: None if t is None else np.repeat(t[:, None, :], M, 1) * np.where(np.arange(M) == 0, 1, -1)[None, :, None]      # noqa: E731
                    _same(_plan(eng, members, mode, wide(caps), days, k, wide(plan), True, ls, sl), want, None, "caps per member")
    eng.close()


def test_where_no_cap_binds_one_day_is_the_group_list_of_k():
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    members = gc.member_matrix(r.U, 9, 4)
    nG = len(members)
    slate = pg.slate_of(r.I, 300)
    for mode in ALL_MODES:
        for k in (1, 10, 64):
            W = _words(eng, members, mode)
            lists = pg.group_exclusions(W, r.cats, mc.caps_uncapped(nG, 6, k), k)
            for more in (0, 5):
                caps = mc.caps_uncapped(nG, 6, k, more)
                for ls, sl in ((None, None), (lists, None), (None, slate)):
                    s, i = eng.topk_groups(_dev(members), k, MODE_NAMES[mode], None if ls is None else [x.tolist() for x in ls],
                                           None if sl is None else _dev(sl))
                    eng.check()
                    want = _t((s, i))
                    got = _plan(eng, members, mode, caps, 1, k, None, False, ls, sl)
                    assert eng.last_kernel() == "m2d_menu_merge"
                    _same((got[0][:, 0], got[1][:, 0]), want, mode, "%s k = %d" % (MODE_NAMES[mode], k))
                    per = _plan(eng, members, mode, np.repeat(caps[:, None, :], 4, 1), 1, k, np.repeat(caps[:, None, :], 4, 1), True, ls, sl)
                    _same((per[0][:, 0], per[1][:, 0]), want, mode, "caps and plan caps per member that bind nothing")
    eng.close()


# ---- 7. errors and refusals ------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from foodrec_amd import _native
    r = mc.exact_recipe(4, 64, 257)
    eng = _engine(r)
    members = gc.member_matrix(r.U, 5, 3)
    caps = mc.caps_all(5, 4, 2)
    lists = [np.asarray([1, 2], np.int64)] * 5
    slate = pg.slate_of(r.I, 100)
    bad = _native.M2D_ERR_INVALID_ARG
    for M in (0, -1, 65):
        assert _abi(eng, members, 0, caps, 2, 5, M=M)[0] == bad and eng_error(eng) == NAME + ": need 1 <= M <= 64"
    for mode in (-1, 3):
        assert _abi(eng, members, mode, caps, 2, 5)[0] == bad and eng_error(eng) == NAME + ": mode must be M2D_GROUP_LEAST, _MEAN or _MOST"
    for k in (0, 65, -3, 1024):
        assert _abi(eng, members, 0, caps, 1, k, None, False, lists, slate)[0] == bad and eng_error(eng) == NAME + ": need 1 <= k <= min(64, I)"
    for days, k in ((0, 5), (-1, 5), (205, 5), (1025, 1), (17, 64), (2 ** 31 - 1, 64)):
        assert _abi(eng, members, 0, caps, days, k, None, False, lists, slate)[0] == bad
        assert eng_error(eng) == NAME + ": need days >= 1 and days * k <= M2D_PLAN_MAX_LIST = 1024", (days, k)
    for flag in (-1, 2):
        assert _abi(eng, members, 0, caps, 2, 5, flag=flag)[0] == bad and eng_error(eng) == NAME + ": caps_per_member must be 0 or 1"
    for nD in (0, -1, r.I + 1):
        assert _abi(eng, members, 0, caps, 2, 5, None, False, lists, slate, nD=nD)[0] == bad and eng_error(eng) == NAME + ": with a slate need 1 <= nD <= I"
    assert _abi(eng, members, 0, caps, 2, 5, None, False, lists, slate, null=("excl_ids",))[0] == bad
    assert eng_error(eng) == NAME + ": excl_off without excl_ids"
    for null in ("members", "caps", "scores", "out_ids"):
        assert _abi(eng, members, 0, caps, 2, 5, caps, False, lists, slate, null=(null,))[0] == bad and eng_error(eng) == NAME + ": null buffer"
    assert _abi(eng, members[:0], 0, caps[:0], 3, 5, None, False, [], slate)[0] == 0 and _latched(eng)[0] == 0      # nG == 0: nothing is launched
    for days, k in ((1024, 1), (16, 64), (204, 5)):          # the largest plans are in range
        _same(_plan(eng, members, 0, caps, days, k, None, False, lists, slate), _want(eng, members, 0, r.cats, caps, days, k, None, False, lists, slate))
    eng.close()
    bare = _engine(r, masks=False)
    assert _abi(bare, members, 0, caps, 2, 5)[0] == _native.M2D_ERR_NOT_CONFIGURED
    bare.close()


def test_bad_members_lists_and_slates_are_latched_as_the_calls_they_come_from_latch_them():
    from foodrec_amd import _native
    r = mc.normal_recipe(6, 64, 1300)
    base = 100
    eng = _engine(r, user_base=base)
    M, days, k = 4, 7, 3
    members = gc.member_matrix(r.U, 9, M, user_base=base)
    nG = len(members)
    mode = gc.LEAST
    W = _words(eng, members, mode)
    gcaps, gplan = mc.caps_mixed(nG, 6, seed=2), pc.plan_caps_of(nG, 6, days, k, seed=2)
    caps = pg.spread_caps(gcaps, members, "first", 0)
    slate = pg.slate_of(r.I, 257)
    lists = pg.group_exclusions(W, r.cats, gcaps, k, slate)
    want = pc.plan_lists(W, r.cats, gcaps, gplan, days, k, lists, slate)
    _same(_plan(eng, members, mode, caps, days, k, None, True, lists, slate),
          pc.plan_lists(W, r.cats, gcaps, None, days, k, lists, slate), mode)
    off, ids = pg.csr(lists)

    def groups_reports(m):                                   # what m2d_topk_groups latches for the same members
        s, i = eng.topk_groups(_dev(m), 5)
        return _latched(eng)

    def menus_reports(**kw):                                 # what m2d_plan_menus latches for the same lists and slate
        users = members[:, 0]
        o, x = kw.get("raw", (off, ids))
        eng._plan_menus(_dev(users), days, k, _dev(gcaps), None, (_dev(np.asarray(o, np.int64)), _dev(np.asarray(x, np.int32))),
                        _dev(np.asarray(kw["slate"], np.int32)) if kw.get("slate") is not None else None)
        return _latched(eng)

    for P in (dc.DEFAULT_P, 256):
        eng.set_option("deep_chunk_pairs", P)
        for g, j, value, code in ((0, 0, base + r.U, _native.M2D_ERR_BAD_USER_ID), (4, 1, base - 1, _native.M2D_ERR_BAD_USER_ID),
                                  (nG - 1, 0, -2, _native.M2D_ERR_BAD_USER_ID), (3, 0, -1, _native.M2D_ERR_INVALID_ARG)):
            m = members.copy()
            m[g, j] = value
            if value == -1:
                m[g] = -1                                    # an empty group
            ok = np.setdiff1d(np.arange(nG), [g])
            rc, s, i = _abi(eng, m, mode, gcaps, days, k, gplan, False, lists, slate)
            assert rc == 0
            got = _latched(eng)
            assert got == (code, value, g * M + j) == groups_reports(m), (g, j, value, got)
            _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), mode, "the other groups' rows")
            assert _abi(eng, m, mode, caps, days, k, None, True, lists, slate)[0] == 0 and _latched(eng) == got      # the fold stays in bounds
        m = members.copy()
        g = int(np.flatnonzero(gc.counts(members) == 1)[0])
        m[g, 2] = base + 1                                   # an id behind a -1
        assert _abi(eng, m, mode, gcaps, days, k, gplan, False, lists, slate)[0] == 0
        assert _latched(eng) == (_native.M2D_ERR_INVALID_ARG, base + 1, g * M + 2) == groups_reports(m)
    eng.set_option("deep_chunk_pairs", dc.DEFAULT_P)
    # a bad member AND a cap below 0: the member check comes first in stream order
    m, c = members.copy(), caps.copy()
    m[2, 0], c[0, 0, 0] = base + r.U, -1
    assert _abi(eng, m, mode, c, days, k, None, True)[0] == 0 and _latched(eng) == (_native.M2D_ERR_BAD_USER_ID, base + r.U, 2 * M)
    at = int(off[4]) - 1
    for pos, value in ((at, r.I), (at, -1), (at, int(ids[at - 1]) - 1), (len(ids) - 1, 2 ** 31 - 1)):
        x = ids.copy(); x[pos] = value
        for sl in (None, slate):
            assert _abi(eng, members, mode, gcaps, days, k, None, False, raw=(off, x), slate=sl)[0] == 0
            got = _latched(eng)
            assert got[0] != 0 and got == menus_reports(raw=(off, x), slate=sl), (pos, value, got)
    for q, value in ((0, 1), (4, int(off[3]) - 1), (nG, int(off[nG - 1]) - 1)):
        o = off.copy(); o[q] = value
        assert _abi(eng, members, mode, gcaps, days, k, None, False, raw=(o, ids), slate=slate)[0] == 0
        got = _latched(eng)
        assert got[0] != 0 and got == menus_reports(raw=(o, ids), slate=slate), (q, value, got)
    for pos, value in ((0, -1), (100, r.I), (256, 2 ** 31 - 1), (64, int(slate[63])), (256, int(slate[255]) - 1)):
        sl = slate.copy(); sl[pos] = value
        assert _abi(eng, members, mode, gcaps, days, k, None, False, lists, sl)[0] == 0
        got = _latched(eng)
        code = _native.M2D_ERR_BAD_ITEM_ID if not 0 <= value < r.I else _native.M2D_ERR_INVALID_ARG
        assert got == (code, value, pos) == menus_reports(slate=sl), (pos, value, got)
    _same(_plan(eng, members, mode, gcaps, days, k, gplan, False, lists, slate), want, mode, "after the latched errors")
    eng.close()


def test_refusals_name_the_call():
    from foodrec_amd import _native
    rng = np.random.default_rng(2)
    r7 = mc.normal_recipe(7, 64, 300)
    eng = _engine(r7)
    members = gc.member_matrix(r7.U, 4, 2)
    assert _abi(eng, members, 0, mc.caps_all(4, 7, 2), 3, 5, slate=np.arange(10))[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng).startswith(NAME + ": more than 6 categories")
    eng.close()
    r = dc.normal_recipe(64, I=300, U=8, seed=1, head=False)
    eng = _engine(r)
    members = gc.member_matrix(r.U, 6, 3)
    caps = mc.caps_all(6, 4, 2)
    slate, lists = pg.slate_of(r.I, 100), [np.asarray([3, 9], np.int64)] * 6
    want = _plan(eng, members, 1, caps, 7, 3, caps, False, lists, slate)
    nnz = 3 * r.I
    eng.set_ingredients((rng.standard_normal((50, r.E)) / 8).astype(np.float32), np.arange(0, nnz + 1, 3, dtype=np.int32),
                        rng.integers(0, 50, nnz).astype(np.int32))
    for kw in (dict(), dict(lists=lists), dict(slate=slate), dict(plan=caps)):
        for days in (1, 7):
            assert _abi(eng, members, 1, caps, days, 3, **kw)[0] == _native.M2D_ERR_UNSUPPORTED
            assert eng_error(eng) == NAME + ": the ingredient table is set (not supported)"
    eng.clear_ingredients()
    keep = eng.re[7, 3].item()
    eng.re[7, 3] = float("inf")
    eng.tables_updated()
    assert _abi(eng, members, 1, caps, 7, 3, caps, False, lists, slate)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng) == NAME + ": needs finite tables (a table value is not finite)"
    eng.re[7, 3] = keep
    eng.tables_updated()
    _same(_plan(eng, members, 1, caps, 7, 3, caps, False, lists, slate), want, gc.MEAN, "after the value was put back")
    eng.close()


# ---- 8. surroundings ---------------------------------------------------------------------------------------------------------------------------
def test_existing_calls_are_what_they_were_around_failed_and_refused_calls():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, head=False)
    users = _dev(r.users)
    n = len(r.users)
    eng = _engine(r)
    members = gc.member_matrix(r.U, 9, 3)
    caps = mc.caps_all(n, 4, 2)
    gcaps = mc.caps_all(9, 4, 2)
    slate = pg.slate_of(r.I, 300)
    lists = [np.asarray(sorted({(7 * j + 3 * q) % r.I for q in range(65)}), np.int64) for j in range(n)]
    glists = lists[:9]
    pairs_u = _dev(np.resize(r.users, 500).astype(np.int32))
    pairs_d = _dev((np.arange(500) * 7 % r.I).astype(np.int32))

    def existing():
        out = [_t(eng.topk_groups(_dev(members), 300, "mean", [x.tolist() for x in glists])),
               tuple(x.reshape(n, -1) for x in _plan_menus(eng, r.users, caps, 7, 3, caps, lists, slate)),
               _t(eng._topk_menu_filtered(users, 10, _dev(caps), [x.tolist() for x in lists], _dev(slate)))]
        sc = eng.score_pairs_bydish(pairs_u, pairs_d)
        eng.check()
        out.append((dc.words(sc.cpu().numpy())[None], np.zeros((1, 500), np.int64)))
        return out

    before = existing()
    for sl in (None, slate):                                 # calls that succeed
        _plan(eng, members, 0, gcaps, 7, 3, None, False, glists, sl)
        _plan(eng, members, 1, pg.spread_caps(gcaps, members, "last"), 16, 64, pg.spread_caps(gcaps + 3, members, "first"), True, glists, sl)
    assert _abi(eng, members, 0, gcaps, 17, 64, None, False, glists, slate)[0] == _native.M2D_ERR_INVALID_ARG       # refused calls
    assert _abi(eng, members, 7, gcaps, 7, 3)[0] == _native.M2D_ERR_INVALID_ARG
    bad = slate.copy(); bad[5] = r.I                                                                                # failed ones
    assert _abi(eng, members, 0, gcaps, 7, 3, None, False, glists, bad)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_ITEM_ID
    x = [np.asarray([5, 4], np.int64)] * 9
    assert _abi(eng, members, 0, gcaps, 7, 3, None, False, x, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_INVALID_ARG
    m = members.copy(); m[3, 0] = r.U
    assert _abi(eng, m, 0, gcaps, 7, 3, None, False, glists, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_USER_ID
    neg = pg.spread_caps(gcaps, members, "first"); neg[0, 0, 0] = -1
    assert _abi(eng, members, 0, neg, 7, 3, None, True, glists, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_INVALID_ARG
    assert _abi(eng, members, 0, gcaps, 7, 3, -gcaps, False, glists, slate)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_INVALID_ARG
    for a, b in zip(before, existing()):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]), "an existing call moved"
    eng.close()


def test_plans_follow_write_memory_and_tables_updated():
    import torch
    b = dc.normal_recipe(64, I=500, U=16, seed=2, head=False)
    rng = np.random.default_rng(8)
    eng = _engine(b, tables=(b.PM.copy(), b.RE.copy(), b.CE.copy()))
    members = gc.member_matrix(b.U, 9, 3)
    gcaps, gplan = mc.caps_all(9, 4, 2), pc.plan_caps_of(9, 4, 7, 3)
    caps, plan = pg.spread_caps(gcaps, members, "middle"), pg.spread_caps(gplan, members, "first")
    slate = pg.slate_of(b.I, 300)
    t = lambda a: torch.as_tensor(a, device="cuda")         # noqa: E731
    cats = [b.cats]

    def check(before, what):
        W = _words(eng, members, gc.MEAN)
        _same(_plan(eng, members, gc.MEAN, caps, 7, 3, plan, True, None, slate), pc.plan_lists(W, cats[0], gcaps, gplan, 7, 3, None, slate), gc.MEAN, what)
        free = _plan(eng, members, gc.MEAN, caps, 7, 3, plan, True)
        _same(free, pc.plan_lists(W, cats[0], gcaps, gplan, 7, 3), gc.MEAN, what + ", the catalogue")
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
    eng.dish_cats.copy_(t(cats[0]))
    eng.tables_updated()
    check(state, "tables_updated with changed masks")
    eng.close()


def test_inputs_that_arrive_late_on_a_side_stream():
    """Stream order: on a side stream a blocker (matrix products), then the copies that put the real members, caps, plan caps,
    exclusion lists and slate where decoys stood, then the call -- entered while the blocker runs.  The plans are the real request's,
    on an engine whose first menu call this is and again on the warmed engine."""
    import torch
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    days, k, M = 7, 3, 3
    twin = _engine(r)
    members = (gc.member_matrix(r.U, 9, M, seed=1), gc.member_matrix(r.U, 9, M, seed=2))
    nG = 9
    caps = tuple(pg.spread_caps(mc.caps_all(nG, 6, c), m, "last", 0) for c, m in zip((2, 1), members))
    plans = tuple(pg.spread_caps(pc.plan_caps_of(nG, 6, days, k, seed=s), m, "first", 0) for s, m in zip((1, 2), members))
    slates = (pg.slate_of(r.I, 700, seed=1), pg.slate_of(r.I, 700, seed=2))
    lists = [pg.group_exclusions(_words(twin, members[j], gc.LEAST), r.cats, mc.caps_all(nG, 6, 2), k, slates[j], sizes=(65,), seed=j) for j in (0, 1)]
    want, other = (_plan(twin, members[j], gc.LEAST, caps[j], days, k, plans[j], True, lists[j], slates[j]) for j in (0, 1))
    _same(want, _want(twin, members[0], gc.LEAST, r.cats, caps[0], days, k, plans[0], True, lists[0], slates[0]), None, "the twin")
    twin.close()
    assert pc.differs(want, other).mean() >= 0.9             # the decoy's answer is another one
    (off, ids), (doff, dids) = pg.csr(lists[0]), pg.csr(lists[1])
    assert len(ids) == len(dids)
    a = torch.randn((8192, 8192), device="cuda")
    side = torch.cuda.Stream()
    src = [_dev(x) for x in (off, ids, slates[0], caps[0], plans[0], members[0])]
    for episode in ("first use", "warmed"):
        bufs = [_dev(x) for x in (doff, dids, slates[1], caps[1], plans[1], members[1])]
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(6):
                a @ a
            for b, s in zip(bufs, src):
                b.copy_(s, non_blocking=True)
            arrived = torch.cuda.Event()
            arrived.record(side)
            late = not arrived.query()                        # the copies had not landed when the call was made
            got = torch.ops.m2d.plan_groups(eng.id, bufs[5], bufs[3], days, k, "least", bufs[4], True, bufs[0], bufs[1], bufs[2])
            side.synchronize()
            eng.check()
        assert late, "the blocker was too short to show anything"
        _same(_t(got), want, None, "side stream, " + episode)
    eng.close()


# ---- 9. the upper layers ---------------------------------------------------------------------------------------------------------------------
def test_torch_op_and_the_model():
    import types
    import torch
    import foodrec_amd
    r = dc.normal_recipe(64, head=False)
    eng = _engine(r)
    days, k, M = 7, 3, 3
    members = gc.member_matrix(r.U, 8, M)
    nG = len(members)
    cnt = gc.counts(members)
    gcaps, gplan = mc.caps_mixed(nG, 4), pc.plan_caps_of(nG, 4, days, k)
    caps, plan = pg.spread_caps(gcaps, members, "middle"), pg.spread_caps(gplan, members, "last")
    slate = pg.slate_of(r.I, 300)
    W = _words(eng, members, gc.MOST)
    lists = pg.group_exclusions(W, r.cats, gcaps, k, slate)
    off, ids = (_dev(x) for x in pg.csr(lists))
    want = _plan(eng, members, gc.MOST, caps, days, k, plan, True, lists, slate)
    _same(want, pc.plan_lists(W, r.cats, gcaps, gplan, days, k, lists, slate), gc.MOST, "oracle (a)")
    op = torch.ops.m2d.plan_groups
    got = op(eng.id, _dev(members), _dev(caps), days, k, "most", _dev(plan), True, off, ids, _dev(slate))
    assert tuple(got[0].shape) == tuple(got[1].shape) == (nG, days, k) and got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    _same(_t(got), want, gc.MOST, "torch.ops.m2d.plan_groups")
    _same(_t(op(eng.id, _dev(members), _dev(gcaps), days, k)), _plan(eng, members, gc.LEAST, gcaps, days, k), None, "the op's defaults")
    one = np.asarray([2, 0, 1, 3], np.int32)                  # a single row is broadcast, in either table
    _same(_t(op(eng.id, _dev(members), _dev(one), 5, 4, "mean", _dev(one + 3), among=_dev(slate))),
          _plan(eng, members, gc.MEAN, np.tile(one, (nG, 1)), 5, 4, np.tile(one + 3, (nG, 1)), False, None, slate), gc.MEAN, "tables [C]")
    _same(_t(eng._plan_groups([row[:c].tolist() for row, c in zip(members, cnt)], days, k, _dev(gcaps), _dev(gplan), "most",
                              [x.tolist() for x in lists], _dev(slate))), want, gc.MOST, "host members and lists")
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        eng._plan_groups(_dev(members), 2, 65, _dev(one))
    with pytest.raises(ValueError, match="days >= 1 and days \\* k <= 1024"):
        eng._plan_groups(_dev(members), 17, 64, _dev(one))
    with pytest.raises(ValueError, match="mode must be one of"):
        eng._plan_groups(_dev(members), 2, 5, _dev(one), mode="median")
    with pytest.raises(ValueError, match="with caps_per_member caps must be"):
        eng._plan_groups(_dev(members), 2, 5, _dev(gcaps), caps_per_member=True)
    with pytest.raises(TypeError):
        eng._plan_groups(_dev(members), 2, 5, _dev(one), _dev(one.astype(np.int64)))
    with pytest.raises(ValueError, match="at least one dish"):
        eng._plan_groups(_dev(members), 2, 5, _dev(one), among=_dev(slate[:0]))
    eng.close()

    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    groups = [[str(u) for u in row[:c]] for row, c in zip(members, cnt)]      # ids as the reference feeds them: str
    capped = sorted({int(u) for row, c in zip(members, cnt) for u in row[:c]})[::2]
    member_caps = {str(u): {1: 1 + u % 2, 3: 0} for u in capped}
    member_plan = {u: [4, days * k, 2 + u % 3, days * k] for u in capped}     # int keys: the same users
    had = {str(u): [str(d) for d in lists[u % nG][::-1]] for u in capped}
    by_group = [np.unique(np.asarray([d for u in row[:c] for d in had.get(str(u), [])], np.int64)) for row, c in zip(members, cnt)]
    tc = np.full((nG, M, 4), k, np.int32)
    tp = np.full((nG, M, 4), days * k, np.int32)
    for g in range(nG):
        for j in range(cnt[g]):
            u = int(members[g, j])
            if u in capped:
                tc[g, j] = [k, 1 + u % 2, k, 0]
                tp[g, j] = member_plan[u]
    for mode in ("least", "mean", "most"):
        s, i = model.plan_group(groups, days, k, mode, member_caps=member_caps, member_plan_caps=member_plan, exclude=had,
                                among=[str(d) for d in slate[::-1]] + [str(slate[0])])
        assert s.dtype == np.float32 and i.dtype == np.int32 and s.shape == i.shape == (nG, days, k)
        ref = _plan(model.engine, members, gc.MODES[mode], tc, days, k, tp, True, by_group, slate)
        _same((dc.words(s), i), ref, gc.MODES[mode], "Model.plan_group, member caps, a dict of exclusions, among")
        _same(ref, _want(model.engine, members, gc.MODES[mode], r.cats, tc, days, k, tp, True, by_group, slate), gc.MODES[mode], "oracle (a)")
    s, i = model.plan_group(groups, days, k, "mean", caps={1: 2, 3: 0}, plan_caps={0: 4}, exclude=by_group)
    cap2, plan2 = np.tile(np.asarray([k, 2, k, 0], np.int32), (nG, 1)), np.tile(np.asarray([4, days * k, days * k, days * k], np.int32), (nG, 1))
    _same((dc.words(s), i), _plan(model.engine, members, gc.MEAN, cap2, days, k, plan2, False, by_group), gc.MEAN, "Model.plan_group, household caps")
    s, i = model.plan_group(groups)                           # nothing given: 7 days of 3, the first 21 of topk_group's order
    ts, ti = model.topk_group(groups, 21)
    _same((dc.words(s).reshape(nG, 21), i.reshape(nG, 21)), (dc.words(ts), ti), None, "Model.plan_group, nothing given")
    model.set_recipes({str(d): [d % 50, (7 * d) % 50] for d in range(r.I)}, 50)
    market = list(range(0, 50, 2)) + [1, 3]
    for miss in (0, 1):
        cook = model.cookable(market, miss)
        assert 0 < len(cook) < r.I
        s, i = model.plan_group(groups, days, k, "least", member_caps=member_caps, exclude=had, market=market, max_missing=miss)
        _same((dc.words(s), i), _plan(model.engine, members, gc.LEAST, tc, days, k, None, True, by_group, cook), None, "Model.plan_group, a market")
    s, i = model.plan_group(groups, 4, 5, market=[49])
    assert len(model.cookable([49])) == 0 and (i == -1).all() and np.isnan(s).all() and i.shape == (nG, 4, 5)
    with pytest.raises(ValueError, match="among together with market"):
        model.plan_group(groups, among=[1], market=market)
    with pytest.raises(ValueError, match="together with member_caps"):
        model.plan_group(groups, caps={0: 1}, member_caps=member_caps)
