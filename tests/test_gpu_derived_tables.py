"""The pair kernels that read a table the engine derives itself, on the MI355X: uh[u][c] = <U_high[u], CE_c> (option "user_high_table":
m2d_build_user_high<LPP>, read by m2d_score_pairs_c4<..., UH = true>) and H[d] (m2d_dish_high_from_ingredients<NQ>, read by the HV forms
of m2d_score_pairs_c4 and m2d_score_pairs_c4_small).  Neither table has an accessor: a wrong row shows in a score or nowhere.

The inputs are tests/derived_table_cases.py's exact-arithmetic recipes (tests/test_derived_table_cases_cpu.py holds their conditions):
float32 equals float64 on them whatever the order of summation, so every comparison below is an equality of score bits with the
float64 restatement, on every pair -- 2^18 + 77 of them over every user and dish, so every row of both tables is read many times."""
import numpy as np
import pytest
import torch

import derived_table_cases as dt

pytestmark = pytest.mark.gpu

C4, UH, HV, SMALL_HV, GENERIC = ("m2d_score_pairs_c4", "m2d_score_pairs_c4_uh", "m2d_score_pairs_c4_hv", "m2d_score_pairs_c4_small_hv",
                                 "m2d_score_pairs_generic")
FEEDS = ("pairs", "bydish")


def _engine(r, user_base=0):
    import foodrec_amd
    eng = foodrec_amd.ScoringEngine(r.PM, r.RE, r.CE, coef=dt.COEF, device=torch.device("cuda", 0), user_base=user_base)
    eng.set_dish_categories(r.cats)
    return eng


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def _pairs(r, n=None, user_base=0):
    """(users, items, per-pair masks) of the recipe's first n pairs on the device"""
    n = r.B if n is None else n
    return _i32(r.users[:n] + user_base), _i32(r.items[:n]), torch.from_numpy(np.ascontiguousarray(r.cats[r.items[:n]])).cuda()


def _bits(t):
    return t.view(torch.int32)


def _score(eng, feed, ut, it, ct, kernel):
    got = eng.score_pairs(ut, it, ct) if feed == "pairs" else eng.score_pairs_bydish(ut, it)
    eng.check()
    assert eng.last_kernel() == kernel, (feed, eng.last_kernel())
    return got


def _score_ingredients(eng, ut, it, ct, kernel):
    got = eng.score_pairs_ingredients(ut, it, ct)
    eng.check()
    assert eng.last_kernel() == kernel, eng.last_kernel()
    return got


def _assert_bits(got, ref, what=""):
    """got == the float64 reference as float32 bit patterns, NaN positions as positions"""
    got = got.cpu().numpy()
    want = np.asarray(ref).astype(np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions", int(np.isnan(got).sum()), int(nan.sum()),
                                                np.flatnonzero(np.isnan(got) != nan)[:8])
    bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)) & ~nan)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _set_ingredients(eng, r):
    eng.set_ingredients(r.ING, r.off, r.ids, r.w)


# ---- 1. user_high_table, every width --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", dt.WIDTHS)
def test_user_high_table_every_width(E):
    r = dt.pair_recipe(E)
    eng = _engine(r)
    ut, it, ct = _pairs(r)
    plain = {feed: _score(eng, feed, ut, it, ct, C4) for feed in FEEDS}
    for feed in FEEDS:
        _assert_bits(plain[feed], r.ref, "option off, " + feed)
    eng.set_option("user_high_table", 1)
    for pf in (2, 4):
        eng.set_option("prefetch", pf)
        for feed in FEEDS:
            got = _score(eng, feed, ut, it, ct, UH)
            _assert_bits(got, r.ref, "prefetch %d, %s" % (pf, feed))
            assert torch.equal(_bits(got), _bits(plain[feed])), (pf, feed)


# ---- 2. the reader's second trip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", (36, 256))
def test_user_high_reader_wraps_its_chunk_loop(E):
    r = dt.pair_recipe(E)
    eng = _engine(r)
    ut, it, ct = _pairs(r)
    eng.set_option("user_high_table", 1)
    wide = {feed: _score(eng, feed, ut, it, ct, UH) for feed in FEEDS}
    eng.set_option("blocks_per_cu", 1)
    assert -(-r.B // 64) > 2 * dt.reader_chunks_per_trip(eng.get_option("num_cu"), 1)      # more than two trips
    for feed in FEEDS:
        got = _score(eng, feed, ut, it, ct, UH)
        _assert_bits(got, r.ref, feed)
        assert torch.equal(_bits(got), _bits(wide[feed])), feed


# ---- 3. threshold and fall-through ----------------------------------------------------------------------------------------------------
def test_user_high_threshold_and_fall_through():
    r = dt.pair_recipe(64)
    eng = _engine(r)
    ut, it, ct = _pairs(r)
    eng.set_option("user_high_table", 1)
    for n, kernel in ((2 ** 18 - 1, C4), (2 ** 18, UH)):
        for feed in FEEDS:
            _assert_bits(_score(eng, feed, ut[:n], it[:n], ct[:n], kernel), r.ref[:n], "%d pairs, %s" % (n, feed))
    for option, value, back, kernel in (("prefetch", 1, 2, C4), ("nt_loads", 0, 1, C4), ("variant", 9, 0, GENERIC)):
        eng.set_option(option, value)
        _assert_bits(_score(eng, "pairs", ut, it, ct, kernel), r.ref, "%s = %d" % (option, value))
        eng.set_option(option, back)
    _assert_bits(_score(eng, "pairs", ut, it, ct, UH), r.ref, "options back")
    # one user-range shard
    shard = _engine(r, user_base=7000)
    shard.set_option("user_high_table", 1)
    us = _pairs(r, user_base=7000)[0]
    for feed in FEEDS:
        _assert_bits(_score(shard, feed, us, it, ct, UH), r.ref, "user_base 7000, " + feed)
    # ids out of range past the first 2^18 pairs: the latch, then a clean call
    for what, pos, value in (("user", 2 ** 18 + 5, -1), ("item", 2 ** 18 + 70, r.I)):
        ids = (r.users if what == "user" else r.items).copy()
        ids[pos] = value
        bad = eng.score_pairs(_i32(ids), it, ct) if what == "user" else eng.score_pairs(ut, _i32(ids), ct)
        with pytest.raises(IndexError, match="%s id %d at position %d" % (what, value, pos)):
            eng.check()
        assert eng.last_kernel() == UH and bool(torch.isnan(bad[pos]))
        _assert_bits(_score(eng, "pairs", ut, it, ct, UH), r.ref, "after a bad %s id" % what)


# ---- 4. the builder's second trip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", (8, 16, 32, 64))
def test_user_high_builder_second_trip(lanes):
    import foodrec_amd
    probe = foodrec_amd.ScoringEngine(np.zeros((1, 5, 4), np.float32), np.zeros((1, 4), np.float32), np.zeros((4, 4), np.float32))
    num_cu = probe.get_option("num_cu")
    del probe
    r = dt.big_user_recipe(lanes, num_cu)
    ref = dt.big_user_reference(lanes, num_cu)
    assert r.first_trip < r.U and dt.lpp(r.E) == lanes
    eng = _engine(r)
    assert eng.get_option("num_cu") == num_cu
    ut, it, ct = _pairs(r)
    eng.set_option("user_high_table", 1)
    for pf in (2, 4):
        eng.set_option("prefetch", pf)
        for feed in FEEDS:
            _assert_bits(_score(eng, feed, ut, it, ct, UH), ref, "prefetch %d, %s" % (pf, feed))


# ---- 5. ingredient forms, every width -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("E", dt.WIDTHS)
def test_ingredient_forms_every_width(E, weighted):
    r = dt.ingredient_recipe(E, weighted)
    eng = _engine(r)
    _set_ingredients(eng, r)
    ut, it, ct = _pairs(r)
    _assert_bits(_score_ingredients(eng, ut, it, ct, HV), r.ref, "per-pair masks")
    _assert_bits(_score_ingredients(eng, ut, it, None, HV), r.ref, "resident masks")
    for n, kernel in ((8192, SMALL_HV), (8193, HV)):
        _assert_bits(_score_ingredients(eng, ut[:n], it[:n], ct[:n], kernel), r.ref[:n], "%d pairs" % n)
        _assert_bits(_score_ingredients(eng, ut[:n], it[:n], None, kernel), r.ref[:n], "%d pairs, resident masks" % n)
    if E in (36, 256):                                       # the chunk loop's second trip
        eng.set_option("blocks_per_cu", 1)
        n = 2 * 256 * eng.get_option("num_cu") + 77
        assert n <= r.B
        _assert_bits(_score_ingredients(eng, ut[:n], it[:n], ct[:n], HV), r.ref[:n], "blocks_per_cu 1")
        _assert_bits(_score_ingredients(eng, ut[:n], it[:n], None, HV), r.ref[:n], "blocks_per_cu 1, resident masks")


# ---- 6. the H builder's edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", dt.EDGE_WIDTHS)
def test_ingredient_builder_small_catalogues(E):
    cases = [dt.small_catalogue_recipe(E, n) for n in dt.SMALL_CATALOGUES] + [dt.small_catalogue_recipe(E, 40, all_empty=True)]
    for r in cases:
        eng = _engine(r)
        _set_ingredients(eng, r)
        ut, it, ct = _pairs(r)
        _assert_bits(_score_ingredients(eng, ut, it, ct, SMALL_HV), r.ref, "I = %d, nnz = %d" % (r.I, r.ids.size))
        _assert_bits(_score_ingredients(eng, ut, it, None, SMALL_HV), r.ref, "I = %d, nnz = %d, resident masks" % (r.I, r.ids.size))
    assert np.isnan(cases[-1].ref).all() and cases[-1].ids.size == 0


@pytest.mark.parametrize("E", dt.EXTRA_WIDTHS)
def test_ingredient_builder_second_column_block(E):
    r = dt.ingredient_recipe(E, True, dt.EXTRA_PAIRS)
    eng = _engine(r)
    _set_ingredients(eng, r)
    ut, it, ct = _pairs(r)
    _assert_bits(_score_ingredients(eng, ut, it, ct, GENERIC), r.ref, "per-pair masks")
    _assert_bits(_score_ingredients(eng, ut, it, None, GENERIC), r.ref, "resident masks")


@pytest.mark.parametrize("E", dt.EDGE_WIDTHS)
def test_ingredient_table_set_twice(E):
    r = dt.ingredient_recipe(E, False, dt.EXTRA_PAIRS)
    off, ids, ref2 = dt.second_lists(r)
    eng = _engine(r)
    _set_ingredients(eng, r)
    ut, it, ct = _pairs(r)
    _assert_bits(_score_ingredients(eng, ut, it, ct, HV), r.ref, "first table")
    eng.set_ingredients(r.ING, off, ids, None)
    _assert_bits(_score_ingredients(eng, ut, it, ct, HV), ref2, "second table")


# ---- 7. bad ingredient ids ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", dt.EDGE_WIDTHS)
def test_bad_ingredient_ids_latch_and_recover(E):
    r = dt.ingredient_recipe(E, True)
    eng = _engine(r)
    n = 8193
    ut, it, ct = _pairs(r, n)
    for pos in dt.bad_id_positions(r):
        for value in (-1, r.R):
            ids = r.ids.copy()
            ids[pos] = value
            with pytest.raises(IndexError, match="ingredient id %d at position %d " % (value, pos)):
                eng.set_ingredients(r.ING, r.off, ids, r.w)
            with pytest.raises(ValueError):                   # the table was not kept
                eng.score_pairs_ingredients(ut, it, ct)
            _set_ingredients(eng, r)
            _assert_bits(_score_ingredients(eng, ut, it, ct, HV), r.ref[:n], "after id %d at %d" % (value, pos))
