"""The inputs of tests/test_gpu_derived_tables.py, checked without a GPU (tests/derived_table_cases.py).

The GPU file compares score bits with the float64 restatement.  That rests on four conditions, asserted here on the oracle alone:
float32 arithmetic is exact on every recipe (the float32 restatement equals the float64 one bit for bit, NaN for NaN); every user and
every dish of a recipe is in a pair, and the fixed ingredient layout sits on the wave boundaries it is meant for; big_user_recipe
reaches the builder's second trip from the launcher's own block formula; and the comparison can see a subtly wrong table -- the
scores are recomputed under a stand-in of each fault and at least VISIBLE of the pairs the fault touches must change."""
import numpy as np
import pytest

import derived_table_cases as dt

VISIBLE = 0.95


def _assert_exact(ref, f32):
    assert f32.dtype == np.float32 and ref.dtype == np.float64
    assert np.array_equal(np.isnan(f32), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(f32[ok].view(np.int32), ref[ok].astype(np.float32).view(np.int32)), "float32 differs from float64 on the exact recipe"
    assert np.array_equal(f32[ok].astype(np.float64), ref[ok])


def _assert_pairs_exact(r, ref, pick=slice(None)):
    _assert_exact(ref, dt.pair_scores(r.PM, r.RE, r.CE, r.cats, r.users[pick], r.items[pick], np.float32))
    assert not np.isnan(ref).any() and np.unique(ref).size > 1000


def _assert_ingredients_exact(r):
    _assert_exact(r.ref, dt.ingredient_scores(r.PM, r.RE, r.cats, r.ING, r.off, r.ids, r.w, r.users, r.items, np.float32))
    assert np.array_equal(np.isnan(r.ref), (np.diff(r.off) == 0)[r.items])      # NaN for the dishes without a list and no others


def _assert_covered(r, least):
    assert np.bincount(r.users, minlength=r.U).min() >= least[0], np.bincount(r.users, minlength=r.U).min()
    assert np.bincount(r.items, minlength=r.I).min() >= least[1], np.bincount(r.items, minlength=r.I).min()


def _assert_visible(r, standin, least=VISIBLE, ref=None):
    pairs, alt = standin(r)
    assert pairs.size >= 20, (standin.__name__, pairs.size)
    share = dt.changed_share((r.ref if ref is None else ref)[pairs], alt)
    print("E = %d %s: %.4f of %d pairs" % (r.E, standin.__name__, share, pairs.size))
    assert share >= least, (standin.__name__, r.E, share)
    return share


def _assert_layout(r):
    lens = np.diff(r.off)
    assert r.off[0] == 0 and r.off[-1] == r.ids.size and (r.w is None or r.w.size == r.ids.size)
    assert set(lens.tolist()) <= set(dt.LENGTHS)
    for d, n in dt.fixed_lengths(r.I).items():
        assert lens[d] == n, (d, lens[d], n)
    waves = [lens[s:s + dt.DB] for s in range(0, r.I, dt.DB)]
    assert waves[0][0] == 0 and lens[r.I - 1] == 0          # the first dish of a wave, the last dish of the last wave
    if r.I >= 16:
        assert waves[0][15] == 0                              # the last dish of a full wave
    if r.I > 48:
        assert not waves[1].any() and waves[2][0] == 64 and waves[2][15] == 0 and waves[0].any()
        assert 64 >= 4 * dt.row_batch(r.E)                    # longer than three row batches
    if r.w is not None:                                       # one weight a list: the total is a power of two
        for d in np.flatnonzero(lens):
            w = r.w[r.off[d]:r.off[d + 1]]
            assert (w == w[0]).all() and w[0] in dt.LIST_WEIGHTS and np.log2(float(w.sum())).is_integer()
    assert r.ids.size == 0 or (r.ids.min() >= 0 and r.ids.max() < r.R)


@pytest.mark.parametrize("E", dt.WIDTHS)
def test_pair_recipe_conditions(E):
    r = dt.pair_recipe(E)
    assert (r.U, r.I, r.B) == (1003, 517, 2 ** 18 + 77) and r.E == E
    _assert_pairs_exact(r, r.ref)
    _assert_covered(r, (250, 250))
    assert all(r.U % g for g in (2, 4, 8)) and r.I % dt.DB and r.B % 64
    _assert_visible(r, dt.standin_uh_no_last_column)
    _assert_visible(r, dt.standin_uh_no_fourth)


def test_widths_reach_every_form():
    """every LPP full and partial; every NQ with a full and a partial last column block"""
    forms = {(dt.lpp(E), E // 4 == dt.lpp(E)) for E in dt.WIDTHS}
    assert forms == {(l, f) for l in (8, 16, 32, 64) for f in (True, False)}
    blocks = {(dt.nq(E), E == 64 * dt.nq(E)) for E in dt.WIDTHS}
    assert blocks == {(q, f) for q in (1, 2, 4) for f in (True, False)}
    assert [dt.lpp(E) for E in dt.BIG_WIDTH.values()] == list(dt.BIG_WIDTH) and all(E // 4 < l for l, E in dt.BIG_WIDTH.items())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("E", dt.WIDTHS)
def test_ingredient_recipe_conditions(E, weighted):
    r = dt.ingredient_recipe(E, weighted)
    p = dt.pair_recipe(E)
    assert r.PM is p.PM and np.array_equal(r.users, p.users) and np.array_equal(r.items, p.items) and r.R == 301
    assert (r.w is not None) == weighted
    assert np.array_equal(r.ING * 16, np.round(r.ING * 16)) and np.abs(r.ING).max() <= 1
    _assert_layout(r)
    _assert_ingredients_exact(r)
    _assert_visible(r, dt.standin_h_no_last_entry)
    _assert_visible(r, dt.standin_h_neighbour_row)
    _assert_visible(r, dt.standin_h_no_last_column)
    first, last = dt.bad_id_positions(r)
    assert r.off[32] + dt.row_batch(E) <= first < r.off[32] + 2 * dt.row_batch(E) <= r.off[33] and last == r.ids.size - 1


@pytest.mark.parametrize("E", dt.EXTRA_WIDTHS)
def test_extra_width_conditions(E):
    r = dt.ingredient_recipe(E, True, dt.EXTRA_PAIRS)
    assert r.B == dt.EXTRA_PAIRS and (E % 4 or E > 256)
    _assert_layout(r)
    _assert_covered(r, (16, 31))
    _assert_ingredients_exact(r)
    _assert_visible(r, dt.standin_h_no_last_column)
    off, ids, ref = dt.second_lists(dt.ingredient_recipe(64, False, dt.EXTRA_PAIRS))
    assert not np.array_equal(off, dt.ingredient_recipe(64, False, dt.EXTRA_PAIRS).off) and np.isfinite(ref).mean() > 0.8


@pytest.mark.parametrize("E", dt.EDGE_WIDTHS)
def test_small_catalogue_conditions(E):
    for n in dt.SMALL_CATALOGUES:
        r = dt.small_catalogue_recipe(E, n)
        assert r.I == n
        _assert_layout(r)
        _assert_covered(r, (100, 100))
        _assert_ingredients_exact(r)
        assert np.isnan(r.ref).all() == (n == 1)
    r = dt.small_catalogue_recipe(E, 40, all_empty=True)
    assert r.ids.size == 0 and not np.diff(r.off).any() and np.isnan(r.ref).all()
    _assert_ingredients_exact(r)
    r2 = dt.ingredient_recipe(E, False, dt.EXTRA_PAIRS)         # set_ingredients a second time: another table, exact as well
    off, ids, ref = dt.second_lists(r2)
    _assert_exact(ref, dt.ingredient_scores(r2.PM, r2.RE, r2.cats, r2.ING, off, ids, None, r2.users, r2.items, np.float32))
    assert dt.changed_share(r2.ref, ref) > 0.8


@pytest.mark.parametrize("num_cu", (64, 256, 304))
@pytest.mark.parametrize("lanes", (8, 16, 32, 64))
def test_big_user_recipe_reaches_the_second_trip(lanes, num_cu):
    r = dt.big_user_recipe(lanes, num_cu)
    gpw = 64 // lanes
    assert dt.lpp(r.E) == lanes and r.E // 4 < lanes and r.gpw == gpw
    assert dt.uh_blocks(r.U, r.E, num_cu) == 16 * num_cu                     # the grid is at its cap ...
    assert r.first_trip == 16 * num_cu * 4 * gpw < r.U                      # ... and does not cover the users
    second = r.U - r.first_trip
    assert second == 3 * gpw + (1 if gpw > 1 else 0)
    assert (second % gpw != 0) == (gpw > 1)                                 # a live group whose other users fail `u < U`
    assert r.U * 5 * r.E * 4 < 90e6 and r.B >= 2 ** 18
    _assert_covered(r, (2, 250))
    if num_cu == 256:                                                       # (the MI355X's count: every pair; elsewhere a part)
        ref = dt.big_user_reference(lanes, num_cu)
        _assert_pairs_exact(r, ref)
    else:
        pick = np.union1d(np.arange(2 ** 15), np.flatnonzero(r.users >= r.first_trip))
        ref = np.full(r.B, np.nan)
        ref[pick] = dt.pair_scores(r.PM, r.RE, r.CE, r.cats, r.users[pick], r.items[pick])
        _assert_pairs_exact(r, ref[pick], pick)
    _assert_visible(r, dt.standin_uh_second_trip_zero, ref=ref)
    assert r.B > 64 * dt.reader_chunks_per_trip(num_cu, 1)                  # (the reader wraps at blocks_per_cu = 1 as well)
