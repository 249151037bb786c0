"""CPU checks of the market-retrieval tests (tests/test_gpu_market.py): the new symbols at the boundary, the kernel's constants restated
in tests/market_cases.py against their source lines, the conditions on every recipe, and the comparison against stand-ins for what a
subtly wrong kernel would return -- each stand-in must change the answer of every case aimed at it."""
import inspect
import os

import numpy as np
import pytest

import market_cases as mc
import seen_dish_cases as sd
import slate_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2d_set_recipes", "m2d_clear_recipes", "m2d_cookable_dishes")


def _squeeze(text):
    return " ".join(text.split())


def test_symbols_are_declared_in_the_header_and_the_ctypes_table():
    import ctypes as c
    from foodrec_amd import _native
    header = open(os.path.join(ROOT, "include", "m2d.h")).read()
    for name in NEW:
        assert "int %s(m2d_engine *h" % name in header, name
        assert name in _native.SIGNATURES
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_set_recipes"][1] == [vp, i64, vp, vp, i64, i32]
    assert _native.SIGNATURES["m2d_clear_recipes"][1] == [vp]
    assert _native.SIGNATURES["m2d_cookable_dishes"][1] == [vp, vp, i64, i32, vp, vp, c.POINTER(i64), vp]
    assert _native.ABI_VERSION == 2 and "SYNCHRONISES" in _squeeze(header).upper()
    assert "m2d_market.hip" in open(os.path.join(ROOT, "foodrec_amd", "csrc", "Makefile")).read()


def test_python_surface():
    from foodrec_amd import ops, recommender
    eng, model = ops.ScoringEngine, recommender.Model
    assert list(inspect.signature(eng.set_recipes).parameters) == ["self", "offsets", "ids", "num_ingredients"]
    assert list(inspect.signature(eng.cookable_dishes).parameters)[:4] == ["self", "market", "max_missing", "return_missing"]
    assert list(inspect.signature(eng.topk_market).parameters) == ["self", "users", "market", "k", "max_missing"]
    assert list(inspect.signature(model.cookable).parameters) == ["self", "market", "max_missing"]
    p = inspect.signature(model.topk).parameters
    assert p["market"].default is None and p["max_missing"].default == 0
    assert list(p)[:7] == ["self", "users", "k", "exclude", "head", "candidates", "among"]       # the earlier keywords, where they were
    assert "torch.library" in eng.cookable_dishes.__doc__ and "EXTENSION, `market=" in model.topk.__doc__
    import torch
    assert not hasattr(torch.ops.m2d, "cookable_dishes")


@pytest.fixture(scope="module", autouse=True)
def kernel_constants():
    """every recipe below aims at an edge of these constants: without the source that states them no case here means anything"""
    src = _squeeze(open(os.path.join(ROOT, "foodrec_amd", "csrc", "m2d_market.hip")).read())
    assert all("constexpr int MK_%s = %d;" % (name, value) in src for name, value in (("DW", mc.DW), ("WAVES", mc.WAVES), ("EB", mc.EB)))
    return src


def test_restated_constants_match_their_source_lines(kernel_constants):
    src = kernel_constants
    for line in ("constexpr int MK_DW = %d;" % mc.DW,
                 "constexpr int MK_WAVES = %d;" % mc.WAVES,
                 "constexpr int MK_DB = MK_DW * MK_WAVES;",
                 "constexpr int MK_EB = %d;" % mc.EB,
                 "constexpr int MK_LDS_BITS = 1 << 16;",
                 "const bool lds = R <= MK_LDS_BITS;",
                 'h->last_kernel = lds ? "%s" : "%s";' % (mc.FLAG_LDS, mc.FLAG_L2)):
        assert line in src, line
    assert mc.DB == mc.DW * mc.WAVES and mc.LB == 1 << 16


# ---- the recipes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.CATALOGUES)
def test_catalogue_recipes_hold_the_fixed_layout(n):
    r = mc.catalogue_recipe(n)
    lens = np.diff(r.off)
    assert len(lens) == n and lens[0] == 0 and lens[-1] == 0 and r.off[-1] == len(r.ids) and r.ids.min(initial=0) >= 0 and r.ids.max(initial=0) < r.R
    if n > mc.DW:
        assert lens[mc.DW - 1] == 0
    if n >= 2 * mc.DW:
        assert (lens[mc.DW:2 * mc.DW] == 0).all()
    if n > 3 * mc.DW:
        assert tuple(lens[2 * mc.DW:2 * mc.DW + 4]) == mc.LONG_LISTS and lens[3 * mc.DW - 1] == 0 and r.longest == 3 * mc.EB + 1
    free = np.setdiff1d(np.arange(n), list(mc.fixed_lengths(n)))
    assert ((lens[free] >= 1) & (lens[free] <= 12)).all()
    ids0, miss = mc.restate(r.off, r.ids, r.R, r.market, 0)
    if n > mc.DW:
        assert 0 < len(ids0) < (lens > 0).sum()
        for mm in (1, 2):                                        # every tolerance changes the list
            assert len(mc.restate(r.off, r.ids, r.R, r.market, mm)[0]) > len(mc.restate(r.off, r.ids, r.R, r.market, mm - 1)[0])
    # the longest list as tolerance: exactly the non-empty dishes
    assert np.array_equal(mc.restate(r.off, r.ids, r.R, r.market, r.longest)[0], np.flatnonzero(lens > 0))
    assert np.array_equal(miss < 0, lens == 0)


@pytest.mark.parametrize("R", mc.BITMAP_ROWS)
def test_bitmap_recipes_name_the_word_edges(R):
    r = mc.bitmap_recipe(R)
    assert set(r.ids.tolist()) == set(i for i in (0, 31, 32, R - 1) if i < R) and (np.diff(r.off) == 0).sum() >= 20
    answers = [mc.restate(r.off, r.ids, R, mc.market_ids(m, R), 0)[0] for m in mc.MARKETS]
    assert len(answers[0]) == 0 and len(answers[3]) == (np.diff(r.off) > 0).sum() and np.array_equal(answers[3], answers[4])
    if R > 33:
        assert len({a.tobytes() for a in answers}) == 5          # five different lists from six markets ("all" twice)


def test_tolerance_and_extreme_recipes_are_what_they_are_named():
    t = mc.tolerance_recipe()
    kept = [set(mc.restate(t.off, t.ids, t.R, t.market, mm)[0].tolist()) for mm in (0, 1, 2, t.longest)]
    assert 5 not in kept[1] and 5 in kept[2] and 6 not in kept[0] and 6 in kept[1] and 7 in kept[0] and 8 not in kept[2] and 8 in kept[3]
    assert all(9 not in k for k in kept) and kept[3] == set(np.flatnonzero(np.diff(t.off) > 0).tolist())
    count = lambda r: mc.restate(r.off, r.ids, r.R, r.market, 0)[0]
    assert len(count(mc.extreme_recipe("none"))) == 0
    e = mc.extreme_recipe("every")
    assert len(count(e)) == e.I and e.I % mc.DB
    blocks = np.bincount(count(mc.extreme_recipe("hollow")) // mc.DB, minlength=3)
    assert blocks[0] > 0 and blocks[1] == 0 and blocks[2] > 0
    lw = mc.extreme_recipe("last wave")
    assert lw.I == 2 * mc.DB and len(count(lw)) > 0 and count(lw).min() >= lw.I - mc.DW


def test_composed_recipe_counts():
    r = mc.composed_recipe()
    assert r.I == sc.exact_recipe(4).I == 600
    assert 300 <= len(r.cookable) <= 400 and all(d in r.cookable for d in sd.LAUNCH_EMPTY)
    assert tuple(r.cookable7) == mc.SEVEN and len(mc.restate(r.off, r.ids, r.R, [], 0)[0]) == 0
    assert len(r.lists) == (np.diff(r.off) > 0).sum() < r.I     # the dict form leaves the empty dishes out


# ---- the stand-ins ------------------------------------------------------------------------------------------------------------------
def _catalogue_cases():
    for n in mc.CATALOGUES:
        r = mc.catalogue_recipe(n)
        for mm in (0, 1, 2, r.longest):
            yield r, r.market, mm


def test_standin_last_entry_of_a_long_list_dropped():
    """aimed at every catalogue that holds the long lists"""
    hit = 0
    for r, market, mm in _catalogue_cases():
        if r.I > 2 * mc.DW + 2:                                  # a list of EB + 1 entries is in
            hit += 1
            assert not mc.same_answer(mc.restate(r.off, r.ids, r.R, market, mm), mc.restate(r.off, r.ids, r.R, market, mm, "drop_last_long"))
    assert hit == 4 * 4
    r = mc.catalogue_recipe(3 * mc.DB + 5)                       # and it changes the LIST where the tolerance is 0: the two dishes appear
    assert len(mc.restate(r.off, r.ids, r.R, r.market, 0, "drop_last_long")[0]) == len(mc.restate(r.off, r.ids, r.R, r.market, 0)[0]) + 2


def test_standin_bit_31_of_a_word_absent():
    """aimed at every bitmap case whose market holds a named id 32 w + 31"""
    hit = 0
    for R in mc.BITMAP_ROWS:
        r = mc.bitmap_recipe(R)
        for name in mc.MARKETS:
            market = mc.market_ids(name, R)
            good, alt = mc.restate(r.off, r.ids, R, market, 0), mc.restate(r.off, r.ids, R, market, 0, "bit31")
            if mc.bit31_is_aimed(R, market):
                hit += 1
                assert not mc.same_answer(good, alt) and len(alt[0]) < len(good[0]), (R, name)
            else:
                assert mc.same_answer(good, alt), (R, name)
    assert hit == 3 * 6 + 3                                      # R >= 32: "all", "all twice", "every second"; R = 32, 64, LB: "last" as well


def test_standin_empty_lists_cookable():
    """aimed at every case with an empty list: all of them"""
    cases = list(_catalogue_cases()) + [(mc.bitmap_recipe(R), mc.market_ids(m, R), 0) for R in mc.BITMAP_ROWS for m in mc.MARKETS]
    for r, market, mm in cases:
        good, alt = mc.restate(r.off, r.ids, r.R, market, mm), mc.restate(r.off, r.ids, r.R, market, mm, "empty_cookable")
        assert len(alt[0]) == len(good[0]) + (np.diff(r.off) == 0).sum() > len(good[0])


def test_standin_descending_inside_a_block():
    """aimed at every case in which some block keeps two dishes; the GPU file's `strictly ascending` check refuses it as well"""
    hit = 0
    for r, market, mm in list(_catalogue_cases()) + [(mc.extreme_recipe(w), mc.extreme_recipe(w).market, 0) for w in ("every", "hollow", "last wave")]:
        good = mc.restate(r.off, r.ids, r.R, market, mm)
        if np.bincount(good[0] // mc.DB).max(initial=0) >= 2:
            hit += 1
            alt = mc.restate(r.off, r.ids, r.R, market, mm, "descending")
            assert not mc.same_answer(good, alt) and not np.all(np.diff(alt[0]) > 0) and sorted(alt[0]) == list(good[0])
    assert hit >= 4 * 7 - 2 + 3
