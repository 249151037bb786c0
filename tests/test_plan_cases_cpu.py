"""CPU checks of meal plans (m2d_plan_menus; build-defined): the boundary (header, ctypes table, built
library, engine method, torch op, Model's argument checks), THE IDENTITY THE CALL RESTS ON (D sequential greedy menus over the order
less what was taken equal one walk over merged per-signature lists of D k with cursors that persist, plan caps included, the lists
built in ranges with a running list), float32 against float64 on the exact recipes, the wrong-kernel stand-ins of tests/plan_cases.py
against the cases aimed at them, and the conditions the GPU cases of tests/test_gpu_plan.py rely on, against the restatement alone.

Only the three boundary cases fail without the feature (with all of tests/test_gpu_plan.py); the others check the inputs, the
restatement and the stand-ins, and import nothing of the engine."""
import inspect
import os

import numpy as np
import pytest

import deep_cases as dc
import menu_cases as mc
import menu_filtered_cases as mf
import plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_in_the_header_the_ctypes_table_and_the_library():
    import ctypes as c
    from foodrec_amd import _native
    header = _read("include", "m2d.h")
    assert "int m2d_plan_menus(m2d_engine *h, const int32_t *users /* device [nU] */, int64_t nU, int32_t days, int32_t k," in header
    assert "const int32_t *plan_caps /* device [nU, C] or NULL: over the whole plan */," in header
    assert "#define M2D_PLAN_MAX_LIST 1024" in header and "NO reference counterpart (DESIGN.md 4.15)" in header
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_plan_menus"] == (c.c_int, [vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp])
    assert getattr(_native.lib(), "m2d_plan_menus") is not None               # the built library exports it


def test_python_surface():
    import torch
    from foodrec_amd import ops, recommender
    assert list(inspect.signature(ops.ScoringEngine._plan_menus).parameters) == ["self", "users", "days", "k", "caps", "plan_caps", "exclude",
                                                                                 "among"]
    sig = inspect.signature(recommender.Model.plan_menus)
    assert list(sig.parameters) == ["self", "users", "days", "k", "caps", "plan_caps", "exclude", "among", "market", "max_missing"]
    assert sig.parameters["days"].default == 7 and sig.parameters["k"].default == 3 and sig.parameters["max_missing"].default == 0
    assert all(sig.parameters[p].default is None for p in ("caps", "plan_caps", "exclude", "among", "market"))
    users = torch.empty(7, dtype=torch.int32, device="meta")
    off, ids = torch.empty(8, dtype=torch.int64, device="meta"), torch.empty(30, dtype=torch.int32, device="meta")
    among = torch.empty(50, dtype=torch.int32, device="meta")
    for caps in (torch.empty((7, 4), dtype=torch.int32, device="meta"), torch.empty(4, dtype=torch.int32, device="meta")):
        for kw in ({}, dict(plan_caps=caps), dict(excl_off=off, excl_ids=ids), dict(among=among),
                   dict(plan_caps=caps, excl_off=off, excl_ids=ids, among=among)):
            s, i = torch.ops.m2d.plan_menus(1, users, caps, 5, 3, **kw)       # the fake implementation
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

    model = object.__new__(recommender.Model)
    model.device, model.engine = torch.device("cpu"), NoEngine()
    users = ["3", "1", "2"]
    for kw in (dict(k=0), dict(k=65), dict(k=True), dict(k=2.0), dict(days=0), dict(days=True), dict(days=1.0), dict(days=342),
               dict(days=17, k=64), dict(among=[1, 2], market=[0]), dict(caps=[1, 2, 3]), dict(caps={4: 1}), dict(caps=[-1, 1, 1, 1]),
               dict(plan_caps=[1, 2, 3]), dict(plan_caps={4: 1}), dict(plan_caps=[-1, 1, 1, 1]), dict(plan_caps=[{0: 1}]),
               dict(exclude=[[1], [2]])):
        with pytest.raises(ValueError, match="plan_menus"):
            model.plan_menus(users, **kw)
    for kw in (dict(), dict(exclude={"3": [5, 4, 4]}), dict(caps={1: 2}, plan_caps={0: 3}, exclude=[[1], [], [2, 2]])):
        s, i = model.plan_menus(users, 5, 7, among=[], **kw)                   # an empty slate: no dish can be taken
        assert s.shape == i.shape == (3, 5, 7) and s.dtype == np.float32 and i.dtype == np.int32
        assert np.isnan(s).all() and (i == -1).all()
    model.cookable = lambda market, max_missing: np.zeros(0, np.int32)
    s, i = model.plan_menus(users, market=[3, 4], max_missing=1)
    assert np.isnan(s).all() and (i == -1).all() and i.shape == (3, 7, 3)
    model.plan_menus(users, 341, 3, among=[])                                  # days k = 1 023 is in range, and so is 16 x 64
    model.plan_menus(users, 16, 64, among=[])


# ---- the identity ---------------------------------------------------------------------------------------------------------------------
def _random_case(rng):
    C = int(rng.integers(1, 5))
    I = int(rng.integers(1, 61))
    k = int(rng.integers(1, min(I, 5) + 1))
    days = int(rng.integers(1, 6))
    sig = rng.integers(0, 1 << C, I)
    cats = mc._bits(sig, C)
    if rng.random() < 0.5:                                   # integer scores: heavy ties
        s = rng.integers(-3, 4, I).astype(np.float32)
        s[rng.random(I) < 0.1] = -0.0
    else:
        s = rng.standard_normal(I).astype(np.float32)
    s[sig == 0] = np.nan                                     # an empty mask scores NaN: it comes last and is never capped
    caps = rng.integers(0, k + 2, C)
    plan = rng.integers(0, days * k + 2, C) if rng.random() < 0.7 else None
    slate = np.sort(rng.choice(I, int(rng.integers(1, I + 1)), replace=False)) if rng.random() < 0.4 else None
    x = np.sort(rng.integers(0, I, int(rng.integers(0, I // 2 + 1)))) if rng.random() < 0.5 else np.zeros(0, np.int64)
    return C, I, days, k, cats, s, caps, plan, slate, x


def _sequential(s, cats, caps, plan, days, k, x, slate):
    """D calls of the filtered menu, the host growing the exclusion list and lowering the caps between them: the composition"""
    C = cats.shape[1]
    sig = mc.signatures(cats)
    had, used, rows = np.asarray(x, np.int64), np.zeros(C, np.int64), []
    for d in range(days):
        w, i = mf.filtered_lists(s[None], cats, pc.day_caps(caps, plan, used)[None], k, [np.sort(had)], slate)
        rows.append((w[0], i[0]))
        took = i[0][i[0] >= 0]
        used += pc.used_by(sig, took, C)
        had = np.concatenate([had, took])
    return np.stack([r[0] for r in rows])[None], np.stack([r[1] for r in rows])[None]


def test_the_prefix_identity_plan_caps_included():
    """D sequential greedy menus over the order less what was taken equal the plan over merged per-signature lists of D k with
    persistent cursors: 3 200 random cases, C 1 .. 4, I up to 60, k and D up to 5, caps 0 .. k + 1, plan caps 0 .. D k + 1 or none,
    slates and exclusion lists, dishes of the empty signature, integer scores with heavy ties; every third case without ranges, the
    others in ranges of 1 .. 19 dishes with a running list.  In most the days, the caps and the plan caps matter."""
    rng = np.random.default_rng(15)
    multi = planned = short = deep = 0
    for t in range(3200):
        C, I, days, k, cats, s, caps, plan, slate, x = _random_case(rng)
        seq = _sequential(s, cats, caps, plan, days, k, x, slate)
        full = pc.plan_lists(s[None], cats, caps[None], None if plan is None else plan[None], days, k, [x], slate)
        merged = pc.merged_plan(s[None], cats, caps[None], None if plan is None else plan[None], days, k, [x], slate,
                                W=None if t % 3 == 0 else int(rng.integers(1, 20)))
        assert pc.same(seq, full) and pc.same(full, merged), (t, C, I, days, k, caps.tolist(), None if plan is None else plan.tolist())
        ids = full[1][0]
        took = ids[ids >= 0]
        assert len(np.unique(took)) == len(took) and not np.isin(took, x).any()                    # no dish twice, none excluded
        empty = (ids >= 0).sum(1) == 0
        assert not empty.any() or empty[int(np.argmax(empty)):].all()                              # nothing, then nothing
        multi += int(days > 1 and (ids[1:] >= 0).any())
        planned += int(plan is not None and not pc.same(full, pc.plan_lists(s[None], cats, caps[None], None, days, k, [x], slate)))
        short += int((ids < 0).any())
        deep += int(pc.taken_per_signature(full[1], mc.signatures(cats))[0] > k)
    assert multi > 1500 and planned > 800 and short > 800 and deep > 400, (multi, planned, short, deep)


def test_one_day_without_plan_caps_is_the_filtered_menu():
    r = mc.normal_recipe(6, 64, 1300)
    W32 = mc.host_scores(r, np.float32, r.users)
    n = len(r.users)
    slate = mf.slate_of(r.I, 700)
    for caps in (mc.caps_all(n, 6, 2), mc.caps_mixed(n, 6)):
        lists = mf.own_menu_lists(W32, r.cats, caps, 10, slate)
        w, i = pc.plan_lists(W32, r.cats, caps, None, 1, 10, lists, slate)
        assert dc.same((w[:, 0], i[:, 0]), mf.filtered_lists(W32, r.cats, caps, 10, lists, slate))
        assert pc.same((w, i), pc.plan_lists(W32, r.cats, caps, np.full((n, 6), 10), 1, 10, lists, slate))      # a plan cap of days k binds nothing


@pytest.mark.parametrize("C,E", ((4, 4), (4, 64), (4, 200), (3, 64), (6, 64)))
def test_float32_equals_float64_on_the_exact_recipes(C, E):
    r = mc.exact_recipe(C, E, 1300 if E == 64 else 257)
    s64 = mc.host_scores(r, users=r.users)
    s32 = mc.host_scores(r, np.float32, r.users)
    assert np.array_equal(s64[~np.isnan(s64)], s32[~np.isnan(s32)].astype(np.float64))
    n = len(r.users)
    caps, plan = mc.caps_all(n, C, 2), pc.plan_caps_of(n, C, 7, 3)
    a = pc.plan_lists(s32, r.cats, caps, plan, 7, 3)
    assert pc.same(a, pc.plan_lists(s64.astype(np.float32), r.cats, caps, plan, 7, 3))
    assert pc.same(a, pc.merged_plan(s64.astype(np.float32), r.cats, caps, plan, 7, 3, W=64))


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
def _recipes():
    return [(r, mc.host_scores(r, np.float32, r.users)) for r in (mc.exact_recipe(4, 64, 1300), mc.normal_recipe(6, 64, 1300))]


def _aimed(standin):
    """(W32, cats, caps, plan_caps, days, k, lists, slate) of every case aimed at `standin`"""
    out = []
    if standin in ("cursor_reset", "day_counts_kept", "full_kept", "lists_of_k"):
        for r, W32 in _recipes():
            n = len(r.users)
            for days, k, cap in ((2, 1, 1), (7, 3, 2), (13, 5, 2), (8, 8, 5)):
                caps = mc.caps_all(n, r.C, cap)
                for slate in (None, mf.slate_of(r.I, 700)):
                    out.append((W32, r.cats, caps, None, days, k, None, slate))
    elif standin in ("plan_ignored", "plan_per_day"):
        for r, W32 in _recipes():
            n = len(r.users)
            for days, k in ((2, 1), (7, 3), (13, 5)):
                caps = mc.caps_all(n, r.C, max(1, k - 1))
                plan = np.full((n, r.C), max(1, days * k // 4) if days > 2 else 1, np.int32)
                out.append((W32, r.cats, caps, plan, days, k, mf.own_menu_lists(W32, r.cats, caps, k), None))
    elif standin == "higher_id":
        for group in mc.TIE_GROUPS:
            r = mc.tie_recipe(group)
            W32 = mc.host_scores(r, np.float32, r.users)
            for j in range(len(r.users)):
                days, k = tie_shape(r.k[j])
                out.append((W32[j:j + 1], r.cats, mc.caps_uncapped(1, r.C, k), None, days, k, None, None))
    return out


def tie_shape(at):
    """(days, k) whose first day ends at position `at` of the order: the tie group that lies across `at` straddles a day boundary"""
    return (2, at) if at <= 64 else (2, 64)


@pytest.mark.parametrize("standin", pc.STANDINS)
def test_every_standin_changes_the_answer_of_every_case_aimed_at_it(standin):
    cases = _aimed(standin)
    assert cases
    for W32, cats, caps, plan, days, k, lists, slate in cases:
        right = pc.plan_lists(W32, cats, caps, plan, days, k, lists, slate)
        assert pc.same(right, pc.merged_plan(W32, cats, caps, plan, days, k, lists, slate, W=mf.RANGE_W))
        assert not pc.same(right, pc.plan_lists(W32, cats, caps, plan, days, k, lists, slate, standin)), (standin, days, k)


# ---- the conditions of the GPU cases -----------------------------------------------------------------------------------------------------
def test_depth_cases_take_more_than_k_dishes_from_one_signature():
    for r in (mc.exact_recipe(3, 64, 1300), mc.exact_recipe(4, 64, 1300)):       # few signatures: the lists are read deep
        W32 = mc.host_scores(r, np.float32, r.users)
        n = len(r.users)
        for days, k in pc.SHAPES[1:]:
            caps = mc.caps_uncapped(n, r.C, k)
            got = pc.merged_plan(W32, r.cats, caps, None, min(days, 40), k)
            assert (pc.taken_per_signature(got[1], r.sig) > k).any(), (days, k)


def test_plan_cap_cases_differ_from_the_plan_without_plan_caps():
    for r, W32 in _recipes():
        n = len(r.users)
        for days, k in ((2, 1), (7, 3), (8, 8), (13, 5), (3, 64)):
            caps = mc.caps_all(n, r.C, max(1, (k + 1) // 2))
            plan = pc.plan_caps_of(n, r.C, days, k)
            a, b = pc.plan_lists(W32, r.cats, caps, plan, days, k), pc.plan_lists(W32, r.cats, caps, None, days, k)
            assert pc.differs(a, b).any(), (days, k)


def test_day_two_is_not_the_second_half_of_a_menu_of_2k_under_doubled_caps():
    for r, W32 in _recipes():
        n = len(r.users)
        for days, k, cap in ((7, 3, 1), (8, 8, 2), (13, 5, 2), (3, 32, 5)):
            caps = mc.caps_all(n, r.C, cap)
            w, i = pc.plan_lists(W32, r.cats, caps, None, 2, k)
            assert pc.differs((w[:, 1], i[:, 1]), pc.doubled_workaround(W32, r.cats, caps, k)).any(), (days, k)
