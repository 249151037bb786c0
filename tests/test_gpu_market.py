"""GPU tests of market retrieval (m2d_set_recipes, m2d_cookable_dishes, topk_market): the cookable-dish list,
its count and the missing counts as integers against the numpy restatement at every edge of the kernel's constants, in poisoned
buffers; the bitmap's word edges in both forms; the tolerance; order and repeatability; errors; independence from every scoring call;
and the composed call bit for bit on exact tables.  Recipes, restatement and stand-ins: tests/market_cases.py.

Slowest case: see README.md (status row "market retrieval")."""
import types

import numpy as np
import pytest

import market_cases as mc
import seen_dish_cases as sd
import slate_cases as sc

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # no dish id, no missing count
GUARD = 64


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


@pytest.fixture(scope="module")
def tiny():
    """engines of E = 4, U = 8 over n dishes: the filter reads none of the tables"""
    made = []

    def make(n_dishes, recipe=None):
        from foodrec_amd import ScoringEngine
        PM, RE, CE, cats = sd.exact_tables(np.random.default_rng(n_dishes), 8, n_dishes, 4)
        eng = ScoringEngine(PM, RE, CE, coef=sd.COEF)
        eng.set_dish_categories(cats)
        if recipe is not None:
            eng.set_recipes(recipe.off, recipe.ids, recipe.R)
        made.append(eng)
        return eng

    yield make
    for eng in made:
        eng.close()


def _cook(eng, market, max_missing=0):
    """cookable_dishes into poisoned buffers: out_ids of capacity I between two guard rows, out_missing.  Returns (ids, missing)
    after checking that nothing but ids[0 .. count) and missing[0 .. I) was written, and that the ids ascend strictly."""
    import torch
    I = eng.I
    buf = torch.full((I + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda")
    miss = torch.full((I,), POISON, dtype=torch.int32, device="cuda")
    ids, m = eng.cookable_dishes(_dev(np.asarray(market, np.int32)), max_missing, return_missing=True, out_ids=buf[GUARD:GUARD + I], out_missing=miss)
    whole, count = buf.cpu().numpy(), ids.numel()
    assert (whole[:GUARD] == POISON).all() and (whole[GUARD + I:] == POISON).all(), "a guard row was written"
    assert (whole[GUARD + count:GUARD + I] == POISON).all(), "out_ids was written at or past count = %d" % count
    got, missing = ids.cpu().numpy(), m.cpu().numpy()
    assert np.array_equal(got, whole[GUARD:GUARD + count]) and m.data_ptr() == miss.data_ptr()
    assert (missing != POISON).all(), "%d words of out_missing not written" % int((missing == POISON).sum())
    assert np.all(np.diff(got) > 0) and (count == 0 or (got[0] >= 0 and got[-1] < I)), "not strictly ascending dish ids"
    return got, missing


def _assert_restated(eng, r, market, max_missing, what=""):
    got = _cook(eng, market, max_missing)
    want = mc.restate(r.off, r.ids, r.R, market, max_missing)
    assert len(got[0]) == len(want[0]), "%s: count %d, restated %d" % (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), "%s: ids differ" % what
    assert np.array_equal(got[1], want[1]), "%s: missing counts of %d dishes differ" % (what, int((got[1] != want[1]).sum()))
    assert mc.same_answer(got, want)
    return got


# ---- 1. catalogue edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.CATALOGUES)
def test_catalogue_edges_equal_the_restatement(tiny, n):
    r = mc.catalogue_recipe(n)
    eng = tiny(n, r)
    for mm in (0, 1, 2, r.longest):
        ids, missing = _assert_restated(eng, r, r.market, mm, "I = %d, max_missing = %d" % (n, mm))
        assert eng.last_kernel() == mc.FLAG_LDS
    assert np.array_equal(ids, np.flatnonzero(np.diff(r.off) > 0))            # the longest list as tolerance: the non-empty dishes
    plain = eng.cookable_dishes(_dev(r.market), 0)                            # without buffers of the caller's, without the counts
    assert plain.dtype.is_floating_point is False and np.array_equal(plain.cpu().numpy(), mc.restate(r.off, r.ids, r.R, r.market, 0)[0])


# ---- 2. bitmap edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", mc.BITMAP_ROWS)
def test_bitmap_edges_in_both_forms(tiny, R):
    r = mc.bitmap_recipe(R)
    eng = tiny(r.I, r)
    for name in mc.MARKETS:
        _assert_restated(eng, r, mc.market_ids(name, R), 0, "R = %d, market %s" % (R, name))
        assert eng.last_kernel() == (mc.FLAG_LDS if R <= mc.LB else mc.FLAG_L2)
    _assert_restated(eng, r, mc.market_ids("every second", R), 1, "R = %d, one missing" % R)


# ---- 3. tolerance ----------------------------------------------------------------------------------------------------------------------
def test_tolerance_counts_every_occurrence(tiny):
    r = mc.tolerance_recipe()
    eng = tiny(r.I, r)
    kept = {}
    for mm in (0, 1, 2, r.longest):
        ids, missing = _assert_restated(eng, r, r.market, mm, "max_missing = %d" % mm)
        kept[mm] = set(ids.tolist())
    assert missing[5] == 2 and 5 in kept[2] and 5 not in kept[1]              # [7, 7], 7 absent: two missing entries
    assert missing[6] == 1 and 6 in kept[1] and 6 not in kept[0] and missing[9] == -1
    assert kept[r.longest] == set(np.flatnonzero(np.diff(r.off) > 0).tolist())


# ---- 4. extremes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("none", "every", "hollow", "last wave"))
def test_extremes(tiny, which):
    r = mc.extreme_recipe(which)
    eng = tiny(r.I, r)
    ids, _ = _assert_restated(eng, r, r.market, 0, which)
    if which == "none":
        assert len(ids) == 0
    if which == "every":
        assert np.array_equal(ids, np.arange(r.I))
    if which == "last wave":
        assert len(ids) and ids[0] >= r.I - mc.DW


def test_no_entries_at_all(tiny):
    """nnz = 0 is legal: nothing is ever cookable"""
    n = mc.DB + 3
    r = types.SimpleNamespace(off=np.zeros(n + 1, np.int32), ids=np.zeros(0, np.int32), R=1)
    eng = tiny(n, r)
    for market in ([], [0]):
        ids, missing = _assert_restated(eng, r, market, 3, "nnz = 0")
        assert len(ids) == 0 and (missing == -1).all()


# ---- 5. order and repeatability ----------------------------------------------------------------------------------------------------------
def test_the_same_call_returns_the_same_list_and_new_recipes_the_new_one(tiny):
    a, b = mc.catalogue_recipe(3 * mc.DB + 5), mc.extreme_recipe("hollow")
    assert a.I > b.I
    eng = tiny(a.I, a)
    first = _assert_restated(eng, a, a.market, 1, "first")
    for _ in range(2):
        again = _cook(eng, a.market, 1)
        assert mc.same_answer(first, again)
    # other lists for the same catalogue: b's, and empty lists for the dishes b does not have
    off = np.concatenate([b.off, np.full(a.I - b.I, b.off[-1], np.int32)])
    eng.set_recipes(off, b.ids, b.R)
    nb = types.SimpleNamespace(off=off, ids=b.ids, R=b.R)
    second = _assert_restated(eng, nb, b.market, 0, "replaced")
    assert not mc.same_answer(first, second) and mc.same_answer(second, _cook(eng, b.market, 0))


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
def test_bad_market_ids_are_named_and_the_next_call_is_correct(tiny):
    r = mc.catalogue_recipe(mc.DB + 1)
    eng = tiny(r.I, r)
    n = len(r.market)
    for pos in (n // 2, n - 1):
        for bad_id in (-1, r.R):
            market = r.market.copy()
            market[pos] = bad_id
            with pytest.raises(IndexError, match=r"ingredient id %d at position %d " % (bad_id, pos)):
                eng.cookable_dishes(_dev(market), 0)
            eng.check()                                           # the latch is clear again
            _assert_restated(eng, r, r.market, 0, "after a bad market id")
    with pytest.raises(ValueError, match="max_missing"):
        eng.cookable_dishes(_dev(r.market), -1)
    _assert_restated(eng, r, r.market, 0, "after max_missing = -1")


def test_bad_recipes_are_refused_and_leave_the_engine_unconfigured(tiny):
    import torch
    r = mc.catalogue_recipe(mc.DB + 1)
    eng = tiny(r.I)
    market = _dev(r.market)
    with pytest.raises(ValueError, match="m2d_set_recipes first"):
        eng.cookable_dishes(market, 0)
    with pytest.raises(ValueError, match="m2d_set_recipes first"):
        eng.topk_market(_dev(np.arange(4, dtype=np.int32)), market, 3)

    def refused(off, ids, match):
        eng.set_recipes(r.off, r.ids, r.R)                        # configured ...
        with pytest.raises(IndexError, match=match):
            eng.set_recipes(off, ids, r.R)
        with pytest.raises(ValueError, match="m2d_set_recipes first"):   # ... and not any more
            eng.cookable_dishes(market, 0)

    off = r.off.copy()
    off[100] = off[99] - 1
    refused(off, r.ids, "not a CSR row pointer")
    refused(r.off, r.ids[:-1], "not a CSR row pointer")           # off[I] != nnz
    off = r.off.copy()
    off[0] = 1
    refused(off, r.ids, "not a CSR row pointer")
    for pos in (0, len(r.ids) // 2, len(r.ids) - 1):
        for bad_id in (-1, r.R):
            ids = r.ids.copy()
            ids[pos] = bad_id
            refused(r.off, ids, r"ingredient id %d at position %d " % (bad_id, pos))
    with pytest.raises(ValueError):
        eng.set_recipes(r.off[:-1], r.ids, r.R)
    with pytest.raises(ValueError):
        eng.set_recipes(r.off, r.ids, 0)
    eng.set_recipes(r.off, r.ids, r.R)
    _assert_restated(eng, r, r.market, 0, "set again")
    eng.clear_recipes()
    with pytest.raises(ValueError, match="m2d_set_recipes first"):
        eng.cookable_dishes(market, 0)
    with pytest.raises(TypeError):
        eng.cookable_dishes(market.to(torch.int64), 0)


def test_a_call_refused_before_anything_is_replaced_keeps_the_previous_recipes_served(tiny):
    """A bad argument and an id error latched by an earlier launch return before the lists are touched: the engine goes on serving
    the previous ones, whose device arrays it still borrows -- they must not have gone back to the allocator.  (Blocks of the lists'
    sizes are taken and zeroed after each refusal: a list read from a recycled block would come out empty.)"""
    import torch
    r = mc.catalogue_recipe(mc.DB + 1)
    eng = tiny(r.I, r)
    first = _assert_restated(eng, r, r.market, 1, "before")
    assert len(first[0]) > 0

    def churn():
        return [torch.zeros(n, dtype=torch.int32, device="cuda") for n in (r.I + 1, len(r.ids)) for _ in range(4)]

    with pytest.raises(ValueError, match="m2d_set_recipes: bad argument"):
        eng.set_recipes(r.off, r.ids, 0)
    junk = churn()
    assert mc.same_answer(first, _cook(eng, r.market, 1)), "after a refused num_ingredients = 0"
    eng.score_slate(_dev(np.asarray([0, 99], np.int32)), _dev(np.asarray([0, 1], np.int32)))     # user 99 of 8, not checked
    with pytest.raises(IndexError, match="user id 99 at position 1 "):
        eng.set_recipes(r.off, r.ids, r.R)
    junk += churn()
    assert mc.same_answer(first, _cook(eng, r.market, 1)), "after a set refused for an earlier launch's id error"
    other = mc.extreme_recipe("every")                          # and a set that succeeds still replaces them
    off = other.off[:r.I + 1]
    eng.set_recipes(off, other.ids[:off[-1]], other.R)
    junk += churn()
    _assert_restated(eng, types.SimpleNamespace(off=off, ids=other.ids[:off[-1]], R=other.R), other.market, 0, "replaced")
    del junk


def test_host_arrays_are_copied_and_owned_by_the_engine(tiny):
    """m2d_set_recipes with M2D_TABLES_HOST through the C ABI: the engine copies, so the caller's arrays may change; a second set
    frees the first copies, a refused set frees its own, destroy frees the last"""
    from foodrec_amd import _native
    lib = _native.lib()
    a, b = mc.catalogue_recipe(mc.DB + 1), mc.extreme_recipe("hollow")
    eng = tiny(a.I)

    def set_host(r, n_dishes, ids=None):
        off = np.ascontiguousarray(np.concatenate([r.off, np.full(max(0, n_dishes - r.I), r.off[-1], np.int32)])[:n_dishes + 1])
        ids = np.array(r.ids[:off[-1]] if ids is None else ids, dtype=np.int32)
        rc = lib.m2d_set_recipes(eng._h, r.R, off.ctypes.data, ids.ctypes.data, len(ids), _native.M2D_TABLES_HOST)
        shape = types.SimpleNamespace(off=off.copy(), ids=ids.copy(), R=r.R)
        off[:] = 0                                               # the caller's arrays are the caller's again
        ids[:] = 0
        return rc, shape

    rc, shape = set_host(a, a.I)
    assert rc == 0
    _assert_restated(eng, shape, a.market, 1, "host arrays")
    rc, shape = set_host(b, a.I)                                 # b's first a.I dishes: replaces, frees a's copies
    assert rc == 0
    _assert_restated(eng, shape, b.market, 0, "host arrays, replaced")
    bad = a.ids.copy()
    bad[7] = a.R
    rc, _ = set_host(a, a.I, bad)
    assert rc == _native.M2D_ERR_BAD_INGREDIENT and "ingredient id %d at position 7 " % a.R in _native.error_text(eng._h)
    with pytest.raises(ValueError, match="m2d_set_recipes first"):
        eng.cookable_dishes(_dev(a.market), 0)
    assert lib.m2d_set_recipes(eng._h, a.R, a.off.ctypes.data, a.ids.ctypes.data, len(a.ids), 7) == _native.M2D_ERR_INVALID_ARG
    rc, shape = set_host(a, a.I)
    assert rc == 0
    _assert_restated(eng, shape, a.market, 0, "host arrays, set again")
    eng.close()                                                  # m2d_destroy with owned copies


# ---- 7. independence -------------------------------------------------------------------------------------------------------------------
def _raw(x):
    return np.ascontiguousarray(x.cpu().numpy()).view(np.int32)


def test_recipes_and_scoring_do_not_touch_each_other():
    from foodrec_amd import ScoringEngine
    from helpers import mlp_head
    r, m = sc.exact_recipe(64), mc.composed_recipe()
    eng = ScoringEngine(r.PM, r.RE, r.CE, coef=r.coef)
    eng.set_dish_categories(r.cats)
    rng = np.random.default_rng(3)
    u, sl, market = _dev(r.users), _dev(r.slate), _dev(m.market)
    pu, pd = _dev(rng.integers(0, r.U, 5000).astype(np.int32)), _dev(rng.integers(0, r.I, 5000).astype(np.int32))
    pc = _dev(r.cats[pd.cpu().numpy()])

    def scoring():
        out = [eng.score_pairs(pu, pd, pc), *eng.topk_users(u, 10), eng.score_slate(u, sl), *eng.topk_slate(u, sl, 10)]
        eng.check()
        return [_raw(x) for x in out]

    before = scoring()
    eng.set_recipes(m.off, m.ids, m.R)
    assert all(np.array_equal(a, b) for a, b in zip(before, scoring())), "a scoring call changed with the recipes set"
    want = m.cookable
    assert np.array_equal(eng.cookable_dishes(market).cpu().numpy(), want)
    assert all(np.array_equal(a, b) for a, b in zip(before, scoring())), "a scoring call changed after cookable_dishes"

    eng.set_ingredients((rng.integers(-4, 5, (7, 64)) / 4).astype(np.float32), np.arange(r.I + 1, dtype=np.int32), rng.integers(0, 7, r.I).astype(np.int32))
    assert np.array_equal(eng.cookable_dishes(market).cpu().numpy(), want), "the ingredient table changed the cookable list"
    with pytest.raises(ValueError, match="m2d_topk_slate: the ingredient table is set"):
        eng.topk_market(u, market, 10)
    eng.clear_ingredients()
    assert np.array_equal(eng.cookable_dishes(market).cpu().numpy(), want), "clear_ingredients cleared the recipes"
    eng.set_mlp_head(*mlp_head(320, 256, 64, rng))
    assert np.array_equal(eng.cookable_dishes(market).cpu().numpy(), want)
    with pytest.raises(ValueError, match="m2d_topk_slate: the MLP head is set"):
        eng.topk_market(u, market, 10)
    eng.clear_mlp_head()
    eng.clear_recipes()                                          # and the other way round: the scoring calls without the recipes
    assert all(np.array_equal(a, b) for a, b in zip(before, scoring()))
    eng.close()


# ---- 8. the composed call ----------------------------------------------------------------------------------------------------------------
def _assert_lists(s, i, S, users, cookable, k, what):
    """ids as integers, scores as words: slate_cases.exact_lists over the cookable columns, -1 / NaN from the count on"""
    s, i = np.asarray(s), np.asarray(i)
    kk = min(k, len(cookable))
    assert s.shape == i.shape == (len(users), k), what
    assert (i[:, kk:] == -1).all() and np.isnan(s[:, kk:]).all(), "%s: columns past the count" % what
    if kk:
        ws, wi = sc.exact_lists(S[users][:, cookable], cookable, kk)
        assert np.array_equal(i[:, :kk], wi), "%s: ids of %d users differ" % (what, int((i[:, :kk] != wi).any(1).sum()))
        nan = np.isnan(ws)
        assert np.array_equal(np.isnan(s[:, :kk]), nan), what
        assert np.array_equal(sc.bits(np.where(nan, 0, s[:, :kk])), sc.bits(np.where(nan, 0, ws))), "%s: score words differ" % what


@pytest.mark.parametrize("E", (4, 64, 200))
def test_topk_market_equals_the_slate_over_the_cookable_dishes(E):
    from foodrec_amd import ScoringEngine
    r, m = sc.exact_recipe(E), mc.composed_recipe()
    assert 300 <= len(m.cookable) <= 400
    for base in (0, 1000):
        eng = ScoringEngine(r.PM, r.RE, r.CE, coef=r.coef, user_base=base)
        eng.set_dish_categories(r.cats)
        eng.set_recipes(m.off, m.ids, m.R)
        users = _dev(r.users + base)
        for k in (10, 64):
            s, i, count = eng.topk_market(users, _dev(m.market), k)
            eng.check()
            assert count == len(m.cookable)
            _assert_lists(s.cpu().numpy(), i.cpu().numpy(), r.S, r.users, m.cookable, k, "E = %d, k = %d, base %d" % (E, k, base))
        s, i, count = eng.topk_market(users, _dev(m.market7), 10)             # seven cookable dishes: three trailing columns
        eng.check()
        assert count == 7
        _assert_lists(s.cpu().numpy(), i.cpu().numpy(), r.S, r.users, m.cookable7, 10, "E = %d, seven" % E)
        s, i, count = eng.topk_market(users, _dev(np.zeros(0, np.int32)), 10)  # none
        assert count == 0 and (i.cpu().numpy() == -1).all() and np.isnan(s.cpu().numpy()).all() and tuple(s.shape) == (len(r.users), 10)
        wider = mc.restate(m.off, m.ids, m.R, m.market, 2)[0]
        s, i, count = eng.topk_market(users, _dev(m.market), 10, max_missing=2)
        eng.check()
        assert count == len(wider) > len(m.cookable)
        _assert_lists(s.cpu().numpy(), i.cpu().numpy(), r.S, r.users, wider, 10, "E = %d, max_missing = 2" % E)
        for bad_k in (0, 65, True):
            with pytest.raises(ValueError, match="k must be"):
                eng.topk_market(users, _dev(m.market), bad_k)
        eng.close()


def test_model_surface():
    import torch
    import foodrec_amd
    r, m = sc.exact_recipe(64), mc.composed_recipe()
    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    users = [4, 0, 31, 4]
    plain = model.topk(users, 10)
    with pytest.raises(ValueError, match="m2d_set_recipes first"):
        model.cookable([1, 2])
    model.set_recipes(m.lists, m.R)                              # the dict, str keys, empty dishes left out
    market = [str(v) for v in m.market[::-1]] + ["3", "3"]       # str ids, any order, repeats
    got = model.cookable(market)
    assert got.dtype == np.int32 and np.array_equal(got, m.cookable)
    assert np.array_equal(model.cookable(market, max_missing=2), mc.restate(m.off, m.ids, m.R, m.market, 2)[0])
    s, i = model.topk([str(u) for u in users], 10, market=market)
    _assert_lists(s, i, r.S, users, m.cookable, 10, "Model.topk(market)")
    s, i = model.topk(users, 10, market=[mc.RARE])
    _assert_lists(s, i, r.S, users, m.cookable7, 10, "Model.topk(market), seven")
    model.set_recipes((m.off, m.ids), m.R)                       # the CSR pair
    assert np.array_equal(model.cookable(m.market), m.cookable)
    for key in ("600", -1):                                      # a dish the catalogue does not have: refused, nothing replaced
        with pytest.raises(IndexError, match="dish id %d is outside the catalogue" % int(key)):
            model.set_recipes({"3": [1, 2], key: [1]}, m.R)
    assert np.array_equal(model.cookable(m.market), m.cookable)
    for kw, name in (({"exclude": [[1], [2], [3], [4]]}, "exclude"), ({"head": True}, "head=True"), ({"candidates": 8}, "candidates"),
                     ({"among": [1, 2, 3]}, "among")):
        with pytest.raises(ValueError, match="market together with %s" % name):
            model.topk(users, 5, market=market, **kw)
    with pytest.raises(IndexError, match=r"ingredient id %d at position 1 " % m.R):
        model.cookable([0, m.R])
    again = model.topk(users, 10)                                # without market: what it returned before
    assert np.array_equal(again[1], plain[1]) and np.array_equal(again[0].view(np.int32), plain[0].view(np.int32))


# ---- 9. after writers ------------------------------------------------------------------------------------------------------------------
def test_lists_follow_the_engines_writers():
    """topk_market after write_memory and after a train_step equals a fresh engine built from the written tables, ids and score words"""
    import torch
    from foodrec_amd import ScoringEngine
    r = sc.normal_recipe(64, U=64, I=500, nD=300)
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 6, r.I)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(0, 12, int(off[-1])).astype(np.int32)
    market = np.arange(9, dtype=np.int32)
    want = mc.restate(off, ids, 12, market, 0)[0]
    assert 100 < len(want) < 400
    users = _dev(np.arange(r.U, dtype=np.int32))
    t = lambda a: torch.as_tensor(a, device="cuda")

    def engine(PM, RE, CE):
        e = ScoringEngine(PM, RE, CE, coef=0.5)
        e.set_dish_categories(r.cats)
        e.set_recipes(off, ids, 12)
        return e

    def lists(e):
        s, i, count = e.topk_market(users, _dev(market), 10)
        e.check()
        assert count == len(want)
        return _raw(s), i.cpu().numpy()

    def fresh():
        f = engine(eng.pm.cpu().numpy(), eng.re.cpu().numpy(), eng.ce.cpu().numpy())
        out = lists(f)
        f.close()
        return out

    eng = engine(r.PM.copy(), r.RE.copy(), r.CE.copy())
    before = lists(eng)
    B, L = 600, 7
    wu = (np.arange(B) % r.U).astype(np.int32)
    masked = np.flatnonzero(r.cats.sum(1) > 0)
    wi = rng.choice(masked, B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, r.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(r.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    after_write, f = lists(eng), fresh()
    assert (after_write[0] != before[0]).mean() > 0.5, "write_memory changed nothing"
    assert np.array_equal(after_write[0], f[0]) and np.array_equal(after_write[1], f[1]), "after write_memory"
    eng.train_begin("sgd", 200.0)
    tu = (rng.permutation(256) % r.U).astype(np.int32)
    ti = rng.choice(masked, 256).astype(np.int32)
    eng.train_step(t(tu), t(ti), t(r.cats[ti]), t(rng.integers(0, 2, 256).astype(np.float32))); eng.check()
    after_step, f = lists(eng), fresh()
    assert (after_step[0] != after_write[0]).mean() > 0.5, "train_step changed nothing"
    assert np.array_equal(after_step[0], f[0]) and np.array_equal(after_step[1], f[1]), "after train_step"
    eng.train_end()
    eng.close()
