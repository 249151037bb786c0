"""CPU checks of filtered menu retrieval (m2d_topk_menu_filtered; build-defined): the boundary (header, ctypes
table, built library, engine method, torch op, Model's argument checks), THE IDENTITY THE CALL RESTS ON with dishes removed (the menu
over the allowed order equals the menu over the merge of each signature's own first k allowed dishes, ranges with a running list
included), float32 against float64 on the exact recipes, the wrong-kernel stand-ins of tests/menu_filtered_cases.py against the cases
aimed at them, and the conditions the GPU cases of tests/test_gpu_menu_filtered.py rely on, against the restatement alone.

Only the three boundary cases fail without the feature (with all of tests/test_gpu_menu_filtered.py); the others check the inputs, the
restatement and the stand-ins, and import nothing of the engine."""
import inspect
import os

import numpy as np
import pytest

import deep_cases as dc
import menu_cases as mc
import menu_filtered_cases as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_in_the_header_the_ctypes_table_and_the_library():
    import ctypes as c
    from foodrec_amd import _native
    header = _read("include", "m2d.h")
    assert "int m2d_topk_menu_filtered(m2d_engine *h, const int32_t *users /* device [nU] */, int64_t nU, int32_t k," in header
    assert "const int32_t *slate /* [nD] strictly ascending, or NULL: the whole catalogue */, int64_t nD," in header
    assert "NO reference counterpart (DESIGN.md 4.14)" in header and "ONE STREAM SYNCHRONISATION PER\n * CALL WITH A SLATE" in header
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_topk_menu_filtered"] == (c.c_int, [vp, vp, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp])
    assert getattr(_native.lib(), "m2d_topk_menu_filtered") is not None        # the built library exports it


def test_python_surface():
    import torch
    from foodrec_amd import ops, recommender
    assert list(inspect.signature(ops.ScoringEngine._topk_menu_filtered).parameters) == ["self", "users", "k", "caps", "exclude", "among"]
    sig = inspect.signature(recommender.Model.topk_menu_filtered)
    assert list(sig.parameters) == ["self", "users", "k", "caps", "exclude", "among", "market", "max_missing"]
    assert sig.parameters["k"].default == 10 and sig.parameters["max_missing"].default == 0
    assert all(sig.parameters[p].default is None for p in ("caps", "exclude", "among", "market"))
    users = torch.empty(7, dtype=torch.int32, device="meta")
    off, ids = torch.empty(8, dtype=torch.int64, device="meta"), torch.empty(30, dtype=torch.int32, device="meta")
    among = torch.empty(50, dtype=torch.int32, device="meta")
    for caps in (torch.empty((7, 4), dtype=torch.int32, device="meta"), torch.empty(4, dtype=torch.int32, device="meta")):
        for kw in ({}, dict(excl_off=off, excl_ids=ids), dict(among=among), dict(excl_off=off, excl_ids=ids, among=among)):
            s, i = torch.ops.m2d.topk_menu_filtered(1, users, caps, 10, **kw)       # the fake implementation
            assert s.shape == i.shape == (7, 10) and s.dtype == torch.float32 and i.dtype == torch.int32


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
    for kw in (dict(k=0), dict(k=65), dict(k=True), dict(k=2.0), dict(among=[1, 2], market=[0]), dict(caps=[1, 2, 3]), dict(caps={4: 1}),
               dict(caps=[-1, 1, 1, 1]), dict(caps=[{0: 1}]), dict(exclude=[[1], [2]]), dict(among=[1, 2], market=[0], exclude={"3": [1]})):
        with pytest.raises(ValueError, match="topk_menu_filtered"):
            model.topk_menu_filtered(users, **kw)
    for kw in (dict(), dict(exclude={"3": [5, 4, 4]}), dict(caps={1: 2}, exclude=[[1], [], [2, 2]])):
        s, i = model.topk_menu_filtered(users, 7, among=[], **kw)               # an empty slate: no dish can be taken
        assert s.shape == i.shape == (3, 7) and s.dtype == np.float32 and i.dtype == np.int32
        assert np.isnan(s).all() and (i == -1).all()
    model.cookable = lambda market, max_missing: np.zeros(0, np.int32)
    s, i = model.topk_menu_filtered(users, market=[3, 4], max_missing=1)
    assert np.isnan(s).all() and (i == -1).all() and i.shape == (3, 10)


# ---- the identity ---------------------------------------------------------------------------------------------------------------------
def _random_case(rng, one_signature=False):
    C = int(rng.integers(1, mc.MAX_C + 1))
    I = int(rng.integers(1, 401))
    k = int(rng.integers(1, min(I, mc.K_MAX) + 1))
    sig = np.full(I, rng.integers(0, 1 << C)) if one_signature else rng.integers(0, 1 << C, I)
    cats = mc._bits(sig, C)
    if rng.random() < 0.5:                                   # integer scores: heavy ties
        s = rng.integers(-3, 4, I).astype(np.float32)
        s[rng.random(I) < 0.1] = -0.0
    else:
        s = rng.standard_normal(I).astype(np.float32)
    s[sig == 0] = np.nan                                     # an empty mask scores NaN
    caps = rng.integers(0, k + 2, C)
    slate = None
    if rng.random() < 0.6:
        slate = np.sort(rng.choice(I, int(rng.integers(1, I + 1)), replace=False))
    x = np.sort(rng.integers(0, I, int(rng.integers(0, I + 1)))) if rng.random() < 0.8 else np.zeros(0, np.int64)    # with repeats
    return C, I, k, cats, s, caps, slate, x


def test_the_identity_the_call_rests_on_with_dishes_removed():
    """The menu over the allowed order equals the menu over the merged per-signature lists of the allowed dishes: 1 500 random cases, C
    from 1 to 6, I up to 400, random slates and exclusion lists (repeats, ids outside the slate), integer scores with heavy ties, caps
    0 .. k + 1, every third case without ranges, the others in ranges of 1 .. 49 dishes with a running list -- and in most of them the
    filters matter, as do the caps."""
    rng = np.random.default_rng(3)
    filtered = capped = short = 0
    for t in range(1500):
        C, I, k, cats, s, caps, slate, x = _random_case(rng, one_signature=t % 10 == 0)
        full = mf.filtered_lists(s[None], cats, caps[None], k, [x], slate)
        merged = mf.merged_filtered(s[None], cats, caps[None], k, [x], slate, W=None if t % 3 == 0 else int(rng.integers(1, 50)))
        assert dc.same(full, merged), (t, C, I, k, caps.tolist())
        allowed = np.setdiff1d(mf._base(I, slate), x)
        assert np.isin(full[1][full[1] >= 0], allowed).all()
        plain = mc.plain_menu(mc.order_of(dc.words(s)[allowed], allowed), mc.signatures(cats), list(caps) + [0] * (mc.MAX_C - C), k)
        assert full[1][0, :len(plain)].tolist() == plain and (full[1][0, len(plain):] == -1).all(), t
        filtered += int(not dc.same(full, mc.menu_lists(s[None], cats, caps[None], k)))
        capped += int(not dc.same(full, mf.filtered_lists(s[None], cats, np.full((1, C), k), k, [x], slate)))
        short += int(mc.short_rows(full)[0])
    assert filtered > 900 and capped > 600 and short > 300, (filtered, capped, short)


def test_no_filters_is_the_menu_and_caps_of_k_are_the_deep_lists():
    r = mc.normal_recipe(6, 64, 1300)
    W32 = mc.host_scores(r, np.float32, r.users)
    n = len(r.users)
    for caps in (mc.caps_all(n, 6, 2), mc.caps_mixed(n, 6)):
        assert dc.same(mf.filtered_lists(W32, r.cats, caps, 10), mc.menu_lists(W32, r.cats, caps, 10))
        assert dc.same(mf.filtered_lists(W32, r.cats, caps, 10, slate=np.arange(r.I)), mc.menu_lists(W32, r.cats, caps, 10))
    lists = mf.own_menu_lists(W32, r.cats, mc.caps_uncapped(n, 6, 64), 64)
    assert dc.same(mf.filtered_lists(W32, r.cats, mc.caps_uncapped(n, 6, 64), 64, lists), dc.key_lists(W32, 64, lists))
    slate = mf.slate_of(r.I, 257)
    assert dc.same(mf.filtered_lists(W32, r.cats, mc.caps_uncapped(n, 6, 64), 64, None, slate), dc.key_lists(W32[:, slate], 64, ids=slate))


@pytest.mark.parametrize("C,E", ((4, 4), (4, 64), (4, 200), (3, 64), (5, 64), (6, 64)))
def test_float32_equals_float64_on_the_exact_recipes(C, E):
    r = mc.exact_recipe(C, E, 1300 if E == 64 else 257)
    s64 = mc.host_scores(r, users=r.users)
    s32 = mc.host_scores(r, np.float32, r.users)
    assert np.array_equal(s64[~np.isnan(s64)], s32[~np.isnan(s32)].astype(np.float64))
    n = len(r.users)
    caps = mc.caps_mixed(n, C)
    slate = mf.slate_of(r.I, r.I // 2)
    lists = mf.own_menu_lists(s32, r.cats, caps, 10, slate)
    assert dc.same(mf.filtered_lists(s32, r.cats, caps, 10, lists, slate), mf.filtered_lists(s64.astype(np.float32), r.cats, caps, 10, lists, slate))
    assert dc.same(mf.filtered_lists(s32, r.cats, caps, 10, lists, slate), mf.merged_filtered(s64.astype(np.float32), r.cats, caps, 10, lists, slate, W=64))


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
def _outside_lists(W32, cats, caps, k, slate):
    """per row one excluded id that is NOT in the slate and whose successor in the slate is listed"""
    _, own = mf.filtered_lists(W32, cats, caps, k, None, slate)
    out = []
    for row in own:
        d = next(int(d) for d in row if d > 0 and d - 1 not in set(slate.tolist()))
        out.append(np.asarray([d - 1], np.int64))
    return out


def _aimed(standin):
    """(W32, cats, caps, k, lists, slate) of every case aimed at `standin`"""
    out = []
    sizes = (1, 63, 64, 65, 300)
    if standin in ("counted", "by_position", "consume_others"):
        for r in (mc.exact_recipe(4, 64, 1300), mc.normal_recipe(6, 64, 1300)):
            W32 = mc.host_scores(r, np.float32, r.users)
            for cap in (1, 2):
                caps = mc.caps_all(len(r.users), r.C, cap)
                for slate in (None, mf.slate_of(r.I, 700)):
                    use = sizes[1:] if standin == "consume_others" else sizes
                    out.append((W32, r.cats, caps, 10, mf.own_menu_lists(W32, r.cats, caps, 10, slate, use), slate))
    elif standin == "first_range_only":
        r = mc.edge_recipe()
        W32 = mc.host_scores(r, np.float32, r.users)
        for caps, k in ((mc.caps_uncapped(len(r.users), 4, 64), 64), (mc.caps_all(len(r.users), 4, 8), 64)):
            out.append((W32, r.cats, caps, k, mf.range_edge_lists(r, r.users)[0], None))
    elif standin == "slate_descending":
        r = mc.tie_recipe(65)
        W32 = mc.host_scores(r, np.float32, r.users)
        for j in range(len(r.users)):
            for slate in (None, mf.slate_of(r.I, 900, keep=r.copies)):
                out.append((W32[j:j + 1], r.cats, mc.caps_uncapped(1, r.C, r.k[j]), r.k[j], None, slate))
    elif standin == "outside_shift":
        for r in (mc.exact_recipe(4, 64, 1300), mc.normal_recipe(6, 64, 1300)):
            W32 = mc.host_scores(r, np.float32, r.users)
            caps = mc.caps_all(len(r.users), r.C, 2)
            for nD in (257, 700):
                slate = mf.slate_of(r.I, nD)
                out.append((W32, r.cats, caps, 10, _outside_lists(W32, r.cats, caps, 10, slate), slate))
    return out


@pytest.mark.parametrize("standin", mf.STANDINS)
def test_every_standin_changes_the_answer_of_every_case_aimed_at_it(standin):
    cases = _aimed(standin)
    assert cases
    for W32, cats, caps, k, lists, slate in cases:
        right = mf.filtered_lists(W32, cats, caps, k, lists, slate)
        assert dc.same(right, mf.merged_filtered(W32, cats, caps, k, lists, slate, W=mf.RANGE_W))
        assert not dc.same(right, mf.filtered_lists(W32, cats, caps, k, lists, slate, standin)), (standin, k)


def test_the_host_workaround_is_wrong_where_the_caps_are_not_filled_within_its_depth():
    r = mc.exact_recipe(4, 64, 1300)
    W32 = mc.host_scores(r, np.float32, r.users)
    caps = mc.caps_zero_on(len(r.users), 4, 10, 0)
    lists = mf.own_menu_lists(W32, r.cats, caps, 10)
    right = mf.filtered_lists(W32, r.cats, caps, 10, lists)
    assert dc.same(mf.host_workaround(W32, r.cats, caps, 10, lists, r.I), right)
    assert not dc.same(mf.host_workaround(W32, r.cats, caps, 10, lists, 12), right)


# ---- the conditions of the GPU cases -----------------------------------------------------------------------------------------------------
def test_exclusion_cases_change_every_row_that_excludes_anything():
    """lists built from each user's own unfiltered menu: a row with a non-empty list differs from its unfiltered menu, the row with an
    empty list is its unfiltered menu"""
    recipes = [mf.segment_recipe_n(n, multi=m) for n in mf.SEGMENT_NS for m in (False, True)]
    recipes += [mc.exact_recipe(C, 64, 1300) for C in (3, 4, 5, 6)] + [mc.normal_recipe(6, 64, 1300)]
    for r in recipes:
        W32 = mc.host_scores(r, np.float32, r.users)
        n = len(r.users)
        for caps in (mc.caps_all(n, r.C, 2), mc.caps_uncapped(n, r.C, 10)):
            lists = mf.own_menu_lists(W32, r.cats, caps, 10)
            free, got = mc.menu_lists(W32, r.cats, caps, 10), mf.filtered_lists(W32, r.cats, caps, 10, lists)
            some = np.asarray([len(x) > 0 for x in lists])
            assert (mf.differs(got, free) == some).all(), (r.I, r.C)
            assert len({len(x) for x in lists}) == min(n, len(mf.EXCL_SIZES)) or r.I < 300
    r = mf.segment_recipe_n(257)                             # a whole segment excluded: its dishes were listed, now none of them is
    W32 = mc.host_scores(r, np.float32, r.users)
    caps = mc.caps_uncapped(len(r.users), 4, 64)
    free = mc.menu_lists(W32, r.cats, caps, 64)
    got = mf.filtered_lists(W32, r.cats, caps, 64, [r.segment] * len(r.users))
    assert np.isin(free[1], r.segment).any(1).all() and not np.isin(got[1], r.segment).any()


@pytest.mark.parametrize("n,multi", ((1025, True), (1025, False), (257, True)))
def test_boundary_cases_exclude_a_dish_that_would_be_listed_next_to_one_that_is(n, multi):
    r = mf.slice_edge_recipe(n, multi)
    W32 = mc.host_scores(r, np.float32, r.users)
    caps = mc.caps_uncapped(len(r.users), 4, 64)
    lists, kept = mf.edge_lists(r, r.users)
    free, got = mc.menu_lists(W32, r.cats, caps, 64), mf.filtered_lists(W32, r.cats, caps, 64, lists)
    edges = {q for u in r.planted for q, _ in r.planted[u]}
    assert {0, n - 1} <= edges and all(p - 1 in edges and p in edges for p in mf.step_edges(n))
    assert sum(len(x) > 0 for x in lists) >= len(r.users) - 1
    for j in range(len(r.users)):
        assert np.isin(lists[j], free[1][j]).all(), "a planted excluded dish would not be listed"
        assert np.isin(kept[j], got[1][j]).all() and not np.isin(lists[j], got[1][j]).any()


def test_range_edge_cases_exclude_on_both_sides_of_range_and_segment_edges():
    r = mc.edge_recipe()
    W32 = mc.host_scores(r, np.float32, r.users)
    caps = mc.caps_uncapped(len(r.users), 4, 64)
    lists, pairs = mf.range_edge_lists(r, r.users)
    free, got = mc.menu_lists(W32, r.cats, caps, 64), mf.filtered_lists(W32, r.cats, caps, 64, lists)
    sides = set()
    for j in range(len(r.users)):
        assert not np.isin(lists[j], got[1][j]).any()
        for x, keep in pairs[j]:
            if x in free[1][j] and keep in got[1][j]:        # would be listed, and its neighbour across the edge is
                p = int(np.flatnonzero(r.perm == x)[0])
                edge = p if p in r.edges else p + 1
                sides.add((p in r.edges, edge in r.segment_edges))
    assert len(sides) >= 3, sides                            # excluded in front of and behind an edge, at range edges and at segment edges


def test_slate_cases_differ_from_the_catalogue_menu_filtered_afterwards():
    for r in (mc.normal_recipe(6, 64, 1300), mc.normal_recipe(6, 64, 16385)):
        W32 = mc.host_scores(r, np.float32, r.users)
        caps = mc.caps_all(len(r.users), 6, 2)
        free = mc.menu_lists(W32, r.cats, caps, 10)
        for nD in mf.SLATE_NDS:
            if nD >= r.I:
                continue
            slate = mf.slate_of(r.I, nD, seed=nD)
            got = mf.filtered_lists(W32, r.cats, caps, 10, None, slate)
            after = [[d for d in row if d in set(slate.tolist())] for row in free[1]]
            assert any(got[1][j][got[1][j] >= 0].tolist() != after[j] for j in range(len(after))), (r.I, nD)
