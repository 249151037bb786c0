"""CPU checks of household meal plans (m2d_plan_groups; build-defined): the boundary (header, ctypes table,
built library, engine method, torch op, Model.plan_group's argument checks), the cap fold restated in numpy against a plain loop, THE
IDENTITY THE CALL RESTS ON (a group's plan is m2d_plan_menus' walk over the group's words: the merged per-signature form over
group_cases.group_words under folded caps equals the day-by-day composition over words and caps computed by plain loops), the
wrong-kernel stand-ins of tests/plan_group_cases.py against the cases aimed at them, and the conditions the GPU cases of
tests/test_gpu_plan_groups.py rely on.

Only the boundary cases fail without the feature (with all of tests/test_gpu_plan_groups.py); the others check the inputs, the
restatement and the stand-ins, and import nothing of the engine."""
import inspect
import os

import numpy as np
import pytest

import deep_cases as dc
import group_cases as gc
import menu_cases as mc
import menu_filtered_cases as mf
import plan_cases as pc
import plan_group_cases as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_in_the_header():
    header = _read("include", "m2d.h")
    assert "int m2d_plan_groups(m2d_engine *h, const int32_t *members /* device [nG, M], -1 padded */, int64_t nG, int32_t M, int32_t mode," in header
    assert "const int32_t *caps, const int32_t *plan_caps /* or NULL */, int32_t caps_per_member," in header
    assert "NO reference counterpart (DESIGN.md 4.16)" in header
    plan_menus = header[header.index("NO reference counterpart (DESIGN.md 4.15)"):header.index("int m2d_plan_menus(")]
    assert "Not offered:" in plan_menus and "C above 6, households" not in plan_menus


def test_the_symbol_is_in_the_ctypes_table():
    import ctypes as c
    from foodrec_amd import _native
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_plan_groups"] == (c.c_int, [vp, vp, i64, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp])


def test_the_symbol_is_in_the_built_library():
    from foodrec_amd import _native
    assert getattr(_native.lib(), "m2d_plan_groups") is not None


def test_the_torch_ops_fake_kernel_and_the_engine_method():
    import torch
    from foodrec_amd import ops
    assert list(inspect.signature(ops.ScoringEngine._plan_groups).parameters) == ["self", "members", "days", "k", "caps", "plan_caps", "mode",
                                                                                  "exclude", "among", "caps_per_member"]
    assert "plan_groups" not in [n for n in vars(ops.ScoringEngine) if not n.startswith("_")]       # no public engine method
    members = torch.empty((7, 5), dtype=torch.int32, device="meta")
    off, ids = torch.empty(8, dtype=torch.int64, device="meta"), torch.empty(30, dtype=torch.int32, device="meta")
    among = torch.empty(50, dtype=torch.int32, device="meta")
    per_group = (torch.empty((7, 4), dtype=torch.int32, device="meta"), torch.empty(4, dtype=torch.int32, device="meta"))
    per_member = torch.empty((7, 5, 4), dtype=torch.int32, device="meta")
    for caps, flag in ((per_group[0], False), (per_group[1], False), (per_member, True)):
        for mode in ("least", "mean", "most"):
            for kw in ({}, dict(plan_caps=caps), dict(excl_off=off, excl_ids=ids), dict(among=among),
                       dict(plan_caps=caps, excl_off=off, excl_ids=ids, among=among)):
                s, i = torch.ops.m2d.plan_groups(1, members, caps, 5, 3, mode, caps_per_member=flag, **kw)      # the fake implementation
                assert s.shape == i.shape == (7, 5, 3) and s.dtype == torch.float32 and i.dtype == torch.int32


def test_the_models_argument_checks_and_the_empty_slate():
    """on a Model that has no engine behind it: every check below is made before the engine is reached"""
    import torch
    from foodrec_amd import recommender

    class NoEngine:
        C = 4
        id = 0

        def __getattr__(self, name):
            raise AssertionError("the engine was reached: " + name)

    sig = inspect.signature(recommender.Model.plan_group)
    assert list(sig.parameters) == ["self", "groups", "days", "k", "mode", "caps", "plan_caps", "member_caps", "member_plan_caps", "exclude",
                                    "among", "market", "max_missing"]
    assert sig.parameters["days"].default == 7 and sig.parameters["k"].default == 3 and sig.parameters["mode"].default == "least"
    assert inspect.signature(recommender.Model.topk_group).parameters.keys() == {"self", "groups", "k", "mode", "exclude", "among", "market",
                                                                                 "max_missing"}       # unchanged: no caps
    model = object.__new__(recommender.Model)
    model.device, model.engine = torch.device("cpu"), NoEngine()
    groups = [["3", "1"], ["2"], [0, 1, 2]]
    for kw in (dict(k=0), dict(k=65), dict(k=True), dict(days=0), dict(days=1.0), dict(days=17, k=64), dict(mode="median"),
               dict(among=[1, 2], market=[0]), dict(caps=[1, 2, 3]), dict(caps={4: 1}), dict(caps=[-1, 1, 1, 1]), dict(plan_caps={4: 1}),
               dict(caps=[{0: 1}]), dict(member_caps={"3": [1, 2, 3]}), dict(member_caps={"3": {4: 1}}), dict(member_caps={"3": [-1, 1, 1, 1]}),
               dict(member_plan_caps={2: {0: -1}}), dict(member_caps=[[1, 1, 1, 1]]), dict(exclude=[[1], [2]])):
        with pytest.raises(ValueError, match="plan_group"):
            model.plan_group(groups, among=[] if "among" not in kw else kw.pop("among"), **kw)
    for kw in (dict(caps={0: 1}, member_caps={"3": {0: 1}}), dict(plan_caps={0: 1}, member_caps={"3": {0: 1}}),
               dict(caps={0: 1}, member_plan_caps={"3": {0: 1}}), dict(plan_caps=[1, 1, 1, 1], member_plan_caps={})):
        with pytest.raises(ValueError, match="plan_group: caps / plan_caps .* together with member_caps / member_plan_caps"):
            model.plan_group(groups, among=[], **kw)
    with pytest.raises(ValueError, match="1 to 64 members"):
        model.plan_group([["1"], []], among=[])
    with pytest.raises(ValueError, match="1 to 64 members"):
        model.plan_group([list(range(65))], among=[])
    for kw in (dict(), dict(exclude={"3": [5, 4, 4]}), dict(caps={1: 2}, plan_caps={0: 3}, exclude=[[1], [], [2, 2]]),
               dict(member_caps={"1": {1: 2}, 7: [1, 1, 1, 1]}, member_plan_caps={2: {0: 3}}), dict(member_plan_caps={"3": [1, 2, 3, 4]})):
        for mode in ("least", "mean", "most"):
            s, i = model.plan_group(groups, 5, 7, mode, among=[], **kw)          # an empty slate: no dish can be taken
            assert s.shape == i.shape == (3, 5, 7) and s.dtype == np.float32 and i.dtype == np.int32
            assert np.isnan(s).all() and (i == -1).all()
    model.cookable = lambda market, max_missing: np.zeros(0, np.int32)
    s, i = model.plan_group(groups, market=[3, 4], max_missing=1)
    assert np.isnan(s).all() and (i == -1).all() and i.shape == (3, 7, 3)
    model.plan_group(groups, 16, 64, among=[])


# ---- the fold ------------------------------------------------------------------------------------------------------------------------
def test_the_cap_fold_in_numpy_is_the_plain_loop():
    rng = np.random.default_rng(416)
    for _ in range(300):
        nG, M, C = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(1, 7))
        cnt = rng.integers(1, M + 1, nG)
        members = np.where(np.arange(M)[None, :] < cnt[:, None], rng.integers(0, 50, (nG, M)), -1)
        table = rng.integers(-2, 6, (nG, M, C))
        got = pg.fold_caps(table, members)
        assert np.array_equal(got, pg.fold_caps_loop(table.tolist(), members.tolist()))
        assert got.min() >= 0
        neg = pg.negative_caps(table, members, offset=7)
        assert len(neg) == int((np.where(np.arange(M)[None, :, None] < cnt[:, None, None], table, 0) < 0).sum())
        assert all(v == table.reshape(-1)[p - 7] for v, p in neg)
    members = np.asarray([[4, 2, -1], [1, -1, -1]])
    table = np.asarray([[[3, 5], [2, 9], [0, -4]], [[7, 1], [0, 0], [-1, -1]]])
    assert pg.fold_caps(table, members).tolist() == [[2, 5], [7, 1]]              # filler rows bind nothing
    assert pg.negative_caps(table, members) == []                                  # ... and are not checked
    assert pg.fold_caps(table, members, "fold_max").tolist() == [[3, 9], [7, 1]]
    assert pg.fold_caps(table, members, "fold_all_slots").tolist() == [[0, 0], [0, 0]]
    assert pg.fold_caps(table, members, "fold_next_group").tolist() == [[0, 0], [7, 1]]


def test_spread_caps_fold_back_to_the_group_caps_wherever_the_binding_row_stands():
    for M in (1, 3, 8, 64):
        members = gc.member_matrix(6, M + 3, M)
        caps = mc.caps_mixed(len(members), 4, seed=M)
        for slot in ("first", "middle", "last"):
            for filler in (0, -5):
                t = pg.spread_caps(caps, members, slot, filler)
                assert np.array_equal(pg.fold_caps(t, members), caps) and pg.negative_caps(t, members) == []
                cnt = gc.counts(members)
                at = {"first": np.zeros_like(cnt), "middle": cnt // 2, "last": cnt - 1}[slot]
                for g in np.flatnonzero(cnt > 1):            # only one member holds the binding row
                    others = np.delete(t[g, :cnt[g]], at[g], axis=0)
                    assert (others > caps[g]).all()
                if M > 1:
                    assert (t[cnt < M][:, -1] == filler).all()
                    assert not np.array_equal(pg.fold_caps(t, members, "fold_all_slots"), caps)


# ---- the identity --------------------------------------------------------------------------------------------------------------------
def _random_case(rng):
    C = int(rng.integers(1, 5))
    I = int(rng.integers(1, 61))
    k = int(rng.integers(1, min(I, 5) + 1))
    days = int(rng.integers(1, 6))
    M = int(rng.integers(1, 6))
    nG = int(rng.integers(1, 4))
    U = 6
    mode = int(rng.integers(0, 3))
    sig = rng.integers(0, 1 << C, I)
    cats = mc._bits(sig, C)
    if rng.random() < 0.5:                                   # small integers: heavy ties, exact means
        S = rng.integers(-3, 4, (U, I)).astype(np.float32)
        S[rng.random((U, I)) < 0.1] = -0.0
    else:
        S = rng.standard_normal((U, I)).astype(np.float32)
    S[:, sig == 0] = np.nan                                  # an empty mask scores NaN for every member
    cnt = rng.integers(1, M + 1, nG)
    members = np.where(np.arange(M)[None, :] < cnt[:, None], rng.integers(0, U, (nG, M)), -1)
    per_member = bool(rng.random() < 0.5)
    shape = (nG, M, C) if per_member else (nG, C)
    caps = rng.integers(0, k + 2, shape)
    plan = rng.integers(0, days * k + 2, shape) if rng.random() < 0.7 else None
    if per_member:                                           # filler rows hold what must not show
        caps = np.where((members < 0)[:, :, None], rng.integers(-3, 1, shape), caps)
        plan = None if plan is None else np.where((members < 0)[:, :, None], rng.integers(-3, 1, shape), plan)
    slate = np.sort(rng.choice(I, int(rng.integers(1, I + 1)), replace=False)) if rng.random() < 0.4 else None
    lists = [np.sort(rng.integers(0, I, int(rng.integers(0, I // 2 + 1)))) if rng.random() < 0.5 else np.zeros(0, np.int64) for _ in range(nG)]
    return C, I, days, k, mode, cats, S, members, per_member, caps, plan, slate, lists


def _by_the_definition(S, members, mode, cats, caps, plan, days, k, per_member, lists, slate):
    """the definition by plain loops: every group word by group_cases.group_words_loop, the caps by fold_caps_loop, the days as
    calls of the filtered menu with the host growing the exclusion list and lowering the caps between them"""
    C = cats.shape[1]
    sig = mc.signatures(cats)
    w = dc.words(S)
    if per_member:
        caps = pg.fold_caps_loop(caps.tolist(), members.tolist())
        plan = None if plan is None else pg.fold_caps_loop(plan.tolist(), members.tolist())
    out_w, out_i = [], []
    for g, row in enumerate(members):
        ids = [int(u) for u in row if u >= 0]
        gw = np.asarray([gc.group_words_loop([w[u, d] for u in ids], mode) for d in range(S.shape[1])], np.uint32).view(np.float32)
        had, used, rows_w, rows_i = np.asarray(lists[g], np.int64), np.zeros(C, np.int64), [], []
        for d in range(days):
            today = pc.day_caps(caps[g], None if plan is None else plan[g], used)
            ww, ii = mf.filtered_lists(gw[None], cats, today[None], k, [np.sort(had)], slate)
            rows_w.append(ww[0])
            rows_i.append(ii[0])
            took = ii[0][ii[0] >= 0]
            used += pc.used_by(sig, took, C)
            had = np.concatenate([had, took])
        out_w.append(np.stack(rows_w))
        out_i.append(np.stack(rows_i))
    return np.stack(out_w), np.stack(out_i)


def test_a_group_plan_is_the_plan_walk_over_the_group_words_on_random_small_cases():
    rng = np.random.default_rng(4160)
    seen = {"modes": set(), "per_member": 0, "plan": 0, "slate": 0, "excl": 0, "ragged": 0, "binds": 0, "days": 0}
    for _ in range(1200):
        C, I, days, k, mode, cats, S, members, per_member, caps, plan, slate, lists = _random_case(rng)
        want = _by_the_definition(S, members, mode, cats, caps, plan, days, k, per_member, lists, slate)
        for merged in (False, True):
            got = pg.group_plan(S, members, mode, cats, caps, plan, days, k, per_member, lists, slate, merged=merged)
            assert pg.same(got, want, mode), (C, I, days, k, mode, per_member, merged)
        seen["modes"].add(mode)
        seen["per_member"] += per_member
        seen["plan"] += plan is not None
        seen["slate"] += slate is not None
        seen["excl"] += any(len(x) for x in lists)
        seen["ragged"] += bool((members < 0).any())
        seen["days"] += bool(pg.crosses_a_day(want[1]).any())
        free = pg.group_plan(S, members, mode, cats, np.full(C, days * k), None, days, k, False, lists, slate)
        seen["binds"] += not pg.same(free, want, mode)
    assert seen["modes"] == {0, 1, 2} and min(v for n, v in seen.items() if n != "modes") >= 300, seen


# ---- the stand-ins ---------------------------------------------------------------------------------------------------------------------
def _stand_in_case(C=4, E=64, I=257, M=3, nG=7, days=3, k=4, seed=0):
    r = mc.exact_recipe(C, E, I)
    S = pg.exact_words(r)
    members = gc.member_matrix(r.U, nG, M, seed=seed)
    return r, S, members


@pytest.mark.parametrize("mode", (gc.LEAST, gc.MEAN, gc.MOST))
def test_every_fold_stand_in_changes_every_case_aimed_at_it(mode):
    r, S, members = _stand_in_case()
    days, k = 3, 4
    cnt = gc.counts(members)
    W = gc.group_words(S, members, mode).view(np.float32)
    gcaps = mc.caps_all(len(members), 4, 1)
    assert pg.binds(W, r.cats, gcaps, None, days, k).all()
    # fold_max: the binding row in one slot, the others above it -> groups of two or more members
    table = pg.spread_caps(gcaps, members, "middle", filler=0)
    want = pg.group_plan(S, members, mode, r.cats, table, None, days, k, True)
    assert pg.same(want, pg.group_plan(S, members, mode, r.cats, gcaps, None, days, k), mode)
    wrong = pg.group_plan(S, members, mode, r.cats, table, None, days, k, True, standin="fold_max")
    assert pc.differs(want, wrong)[cnt > 1].all() and (cnt > 1).sum() >= 4
    # fold_all_slots: filler caps of 0 planted -> every group with a filler slot loses every capped dish
    wrong = pg.group_plan(S, members, mode, r.cats, table, None, days, k, True, standin="fold_all_slots")
    assert pc.differs(want, wrong)[cnt < members.shape[1]].all() and (cnt < members.shape[1]).sum() >= 4
    # fold_next_group: neighbours with different caps
    alt = gcaps.copy()
    alt[1::2] = 3
    table = pg.spread_caps(alt, members, "first", filler=0)
    want = pg.group_plan(S, members, mode, r.cats, table, None, days, k, True)
    wrong = pg.group_plan(S, members, mode, r.cats, table, None, days, k, True, standin="fold_next_group")
    assert pc.differs(want, wrong)[:-1].all()
    # the same three on the plan caps
    ptable = pg.spread_caps(mc.caps_all(len(members), 4, 2), members, "last", filler=0)
    free = mc.caps_uncapped(len(members), 4, k)
    ftable = np.repeat(free[:, None, :], members.shape[1], 1)
    want = pg.group_plan(S, members, mode, r.cats, ftable, ptable, days, k, True)
    assert pc.differs(want, pg.group_plan(S, members, mode, r.cats, ftable, None, days, k, True)).all()
    assert pc.differs(want, pg.group_plan(S, members, mode, r.cats, ftable, ptable, days, k, True, standin="fold_max"))[cnt > 1].all()
    assert pc.differs(want, pg.group_plan(S, members, mode, r.cats, ftable, ptable, days, k, True, standin="fold_all_slots"))[cnt < 3].all()


def test_every_row_stand_in_changes_every_case_aimed_at_it():
    r, S, members = _stand_in_case()
    days, k = 3, 4
    cnt = gc.counts(members)
    distinct = np.asarray([len(set(row[:c].tolist())) > 1 for row, c in zip(members, cnt)])
    assert distinct.sum() >= 3
    caps = mc.caps_all(len(members), 4, 2)
    plans = {mode: pg.group_plan(S, members, mode, r.cats, caps, None, days, k) for mode in (gc.LEAST, gc.MEAN, gc.MOST)}
    # the modes tell themselves apart on every group of two or more distinct members
    for a, b in ((gc.LEAST, gc.MEAN), (gc.LEAST, gc.MOST), (gc.MEAN, gc.MOST)):
        assert pc.differs(plans[a], plans[b])[distinct].all()
    for mode in (gc.MEAN, gc.MOST):                           # mode_ignored: aimed at the modes that are not the default
        wrong = pg.group_plan(S, members, mode, r.cats, caps, None, days, k, standin="mode_ignored")
        assert pc.differs(plans[mode], wrong)[distinct].all()
    for mode in (gc.LEAST, gc.MEAN, gc.MOST):
        # member_row: the list of the last member's row -> the groups whose last member differs from the group word's owner
        wrong = pg.group_plan(S, members, mode, r.cats, caps, None, days, k, standin="member_row")
        assert pc.differs(plans[mode], wrong)[distinct].all()
        assert pg.same((wrong[0][cnt == 1], wrong[1][cnt == 1]), (plans[mode][0][cnt == 1], plans[mode][1][cnt == 1]), mode)
    for mode in (gc.LEAST, gc.MEAN):                          # reduce_lists: the members' favourites are not the group's
        wrong = pg.group_plan(S, members, mode, r.cats, caps, None, days, k, standin="reduce_lists")
        assert pc.differs(plans[mode], wrong)[distinct].all()


# ---- the conditions the GPU cases rely on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,E,I", ((3, 64, 1300), (4, 4, 257), (4, 200, 257), (6, 64, 255)))
def test_float32_is_float64_on_the_exact_recipes(C, E, I):
    r = mc.exact_recipe(C, E, I)
    s32, s64 = mc.host_scores(r, np.float32), mc.host_scores(r, np.float64)
    ok = ~np.isnan(s64)
    assert np.array_equal(s32[ok].astype(np.float64), s64[ok]) and np.array_equal(np.isnan(s32), ~ok)
    members = gc.member_matrix(r.U, 9, 3)
    for mode in (gc.LEAST, gc.MOST):                          # (the mean of exact words need not be exact: it is restated in float32)
        w = gc.group_words(s32, members, mode)
        assert np.isin(w, dc.words(s32)).all()


@pytest.mark.parametrize("shape", pg.SHAPES, ids=lambda s: "%dx%d" % s)
def test_caps_bind_and_days_are_crossed_where_the_gpu_cases_say_so(shape):
    days, k = shape
    r = mc.exact_recipe(4, 64, 1300)
    S = pg.exact_words(r)
    members = gc.member_matrix(r.U, 8, 3)
    for mode in (gc.LEAST, gc.MEAN, gc.MOST):
        W = gc.group_words(S, members, mode).view(np.float32)
        caps = mc.caps_all(len(members), 4, max(1, (k + 1) // 2))
        plan = pc.plan_caps_of(len(members), 4, days, k)
        assert pg.binds(W, r.cats, caps, None, days, k).mean() >= 0.75     # a cap binds in most groups' plans
        got = pc.plan_lists(W, r.cats, caps, plan, days, k)
        assert days == 1 or pg.crosses_a_day(got[1]).all()
        if days > 1:
            assert pc.differs(got, pc.plan_lists(W, r.cats, caps, None, days, k)).any()


def test_the_modes_give_different_plans_on_the_exact_recipe():
    r = mc.exact_recipe(4, 64, 1300)
    S = pg.exact_words(r)
    members = gc.member_matrix(r.U, 12, 3)
    cnt = gc.counts(members)
    distinct = np.asarray([len(set(row[:c].tolist())) > 1 for row, c in zip(members, cnt)])
    caps = mc.caps_all(len(members), 4, 2)
    p = [pg.group_plan(S, members, mode, r.cats, caps, None, 7, 3) for mode in (gc.LEAST, gc.MEAN, gc.MOST)]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert pc.differs(p[a], p[b])[distinct].all() and distinct.sum() >= 6
    one = cnt == 1                                            # a group of one: the same plan in every mode
    assert one.any() and pg.same((p[0][0][one], p[0][1][one]), (p[2][0][one], p[2][1][one])) and pg.same((p[0][0][one], p[0][1][one]),
                                                                                                          (p[1][0][one], p[1][1][one]))


def test_the_host_workaround_is_short_where_one_signature_fills_the_first_1024():
    r = mc.one_signature_recipe(I=700)
    rng = np.random.default_rng(5)
    S = rng.standard_normal((r.U, r.I)).astype(np.float32)
    members = gc.member_matrix(r.U, 4, 2)
    caps = mc.caps_all(4, 4, 1)                              # one signature, cap 1 on its categories: one dish a day
    want = pg.group_plan(S, members, gc.LEAST, r.cats, caps, None, 3, 2)
    assert ((want[1] >= 0).sum(2) == 1).all()
    work = pg.host_workaround(S, members, gc.LEAST, r.cats, caps, None, 3, 2, depth=2)
    assert pc.differs(want, work).all()                      # a depth of 2 holds two days' dishes, not three
