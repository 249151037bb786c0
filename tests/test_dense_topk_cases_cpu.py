"""CPU checks of the dense-retrieval tests (tests/test_gpu_dense_topk.py): the conditions on every input recipe of
tests/dense_topk_cases.py -- evaluated with the oracle alone --, the launcher's rules restated there against their source lines, and the
comparisons against stand-ins for what a subtly wrong kernel would return: each stand-in must change a list of every case aimed at
it, and fail the comparison."""
import os

import numpy as np
import pytest

import dense_topk_cases as dc
import slate_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [(C, E, w, False) for C, E in dc.MFMA_SHAPES + dc.GENERIC_SHAPES for w in (False, True)] + \
        [(4, 64, False, True), (4, 128, False, True), (4, 200, False, True)]
ALL_USERS = np.arange(dc.U)


def _squeeze(text):
    return " ".join(text.split())


def _source(name):
    """the file with every run of whitespace (line breaks, indentation, alignment) as one blank: a reformatted source still matches"""
    return _squeeze(open(os.path.join(ROOT, "foodrec_amd", "csrc", name)).read())


# ---- the launcher's rules ----------------------------------------------------------------------------------------------------------------
def test_restated_launcher_rules_match_their_source_lines():
    src = _source("m2d_catalogue_dense.hip")
    for line in ("M2D_TOPK(20, 8) M2D_TOPK(40, 8) M2D_TOPK(80, 4)",                         # mfma_form
                 "const bool lds_lists = k > 16;",
                 "if (lds_lists) return launch_mfma<NBV, 2, 0>(h, a, out_scores, out_ids, stream);",
                 "return k <= 10 ? launch_mfma<NBV, WV, 10>(h, a, out_scores, out_ids, stream)",
                 ": launch_mfma<NBV, WV, 16>(h, a, out_scores, out_ids, stream);",
                 "if (!force_generic && K % 8 == 0) {",
                 "const bool force_generic = h->opt_variant == 9;",
                 "const int64_t ublocks = (a.nU + 32 * WAVES - 1) / (32 * WAVES);",          # users_per_block
                 "a.tiles = (h->I + 31) / 32;",                                             # tiles
                 "const int64_t per = (p.tiles + p.nsplit - 1) / p.nsplit;",                # per_range
                 "const int64_t t_begin = (int64_t)blockIdx.y * per;",                      # dish_ranges
                 "const int64_t t_end = min(p.tiles, t_begin + per);",
                 "const int64_t want = 2 * (int64_t)h->num_cu;",                            # auto_nsplit
                 "if (ublocks < want) {",
                 "int64_t ns = (want + ublocks - 1) / ublocks;",
                 "const int64_t cap = a.tiles / 8 > 1 ? a.tiles / 8 : 1;",
                 "if (ns > 64) ns = 64;",
                 "if (ns > cap) ns = cap;",
                 "a.nsplit = nsplit = topk_split_hook(h->opt_variant, nsplit, 64);",        # forced_nsplit: the shared hook, capped at 64
                 "for (int64_t d = wave; d < p.I; d += 4) {"):                              # m2d_topk_generic: four waves stride the dishes
        assert _squeeze(line) in src, line
    hook = _source("m2d_grouped_policy.h")
    for line in ("inline int topk_split_hook(const int variant, int nsplit, const int max_splits)",
                 "if (variant >= 100) {",
                 "nsplit = variant - 100;",
                 "if (nsplit < 1) nsplit = 1;",
                 "if (nsplit > max_splits) nsplit = max_splits;"):
        assert _squeeze(line) in hook, line
    assert "while (lpu < nsplit) lpu <<= 1;" in _source("m2d_catalogue_merge.hip")
    plan = _source("m2d_catalogue_plan.hip")
    assert "h->opt_topk_grouped != 0 && h->opt_variant != 7 && h->opt_variant != 9;" in plan and "h->C == 4 &&" in plan
    # the forms and their blocks
    assert [dc.mfma_form(C, E, 10)[0] for C, E in dc.MFMA_SHAPES] == [20, 40, 80, 20, 40, 80]
    assert all(dc.mfma_form(C, E, k) is None for C, E in dc.GENERIC_SHAPES for k in dc.KS)
    assert [dc.mfma_form(4, 64, k)[2] for k in dc.KS] == [10, 10, 16, 16, 0, 0]
    assert [dc.users_per_block(dc.mfma_form(4, E, k)) for E in (32, 64, 128) for k in (10, 16, 17)] == [256, 256, 64] * 2 + [128, 128, 64]
    # the ranges of I = 600 (19 tiles) that the issue names
    per = [dc.per_range(19, n) for n in dc.RANGE_COUNTS]
    assert per == [19, 10, 7, 3, 3, 1, 1, 1]
    empty = lambda n: sum(hi == lo for lo, hi in dc.dish_ranges(dc.I, n))     # noqa: E731
    assert [empty(n) for n in dc.RANGE_COUNTS] == [0, 0, 0, 0, 1, 0, 1, 45]
    assert dc.dish_ranges(dc.I, 7)[-1] == (576, 600) and dc.dish_ranges(dc.I, 8)[6:] == [(576, 600), (600, 600)]
    assert dc.dish_ranges(33, 2) == [(0, 32), (32, 33)] and dc.dish_ranges(33, 3) == [(0, 32), (32, 33), (33, 33)]
    for n in dc.RANGE_COUNTS:
        rg = dc.dish_ranges(dc.I, n)
        assert rg[0][0] == 0 and max(hi for _, hi in rg) == dc.I and all(a[1] == b[0] for a, b in zip(rg, rg[1:]))
        assert np.array_equal(dc.range_of(dc.I, n), np.concatenate([np.full(hi - lo, s) for s, (lo, hi) in enumerate(rg)]))
    assert [dc.forced_nsplit(v) for v in (100, 101, 119, 164, 165, 300)] == [1, 1, 19, 64, 64, 64]
    # the automatic choice, on the MI355X's 256 units and on a small device
    form = dc.mfma_form(4, 64, 10)
    assert dc.auto_nsplit(1, dc.I, form, 256) == 2 and dc.auto_nsplit(517, dc.I, form, 256) == 2      # tiles / 8 caps it
    assert dc.auto_nsplit(1, 32 * 1000, form, 256) == 64 and dc.auto_nsplit(256 * 512, 32 * 1000, form, 256) == 1
    assert dc.auto_nsplit(256 * 100 + 1, 32 * 1000, form, 256) == 6 and dc.auto_nsplit(1, dc.NORMAL_I, form, 256) == 1
    assert dc.auto_nsplit(1, 32 * 1000, form, 8) == 16


# ---- exact recipes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,E,weighted,ing", EXACT)
def test_exact_recipes_are_exact(C, E, weighted, ing):
    """float32 = float64 on every exact recipe, in the reference's own form and in the factored form the kernels contract: an f32
    chain in ANY order is exact."""
    r = dc.exact_recipe(C, E, weighted, ing)
    S32 = dc.score_matrix(r, np.float32)
    assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), r.S, equal_nan=True)
    Dt32, Dt64 = dc.dish_vectors(r, np.float32), dc.dish_vectors(r, np.float64)
    assert Dt32.dtype == np.float32 and np.array_equal(Dt32.astype(np.float64), Dt64, equal_nan=True)
    P = r.PM.astype(np.float64).reshape(r.U, -1)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(P @ Dt64.T, r.S, equal_nan=True)
    fin = ~np.isnan(Dt64).any(1)
    assert np.array_equal(fin, ~np.isnan(r.S).all(0)) and np.array_equal(fin, ~np.isnan(r.S).any(0))
    # products are multiples of 2^-(4 + q); every partial sum of a score stays below 2^(20 - q): 24 bits hold it
    q = next(q for q in range(4, 20) if np.array_equal(np.round(Dt64[fin] * 2.0 ** q), Dt64[fin] * 2.0 ** q))
    assert np.array_equal(np.round(P * 16), P * 16)
    assert (np.abs(P) @ np.abs(Dt64[fin]).T).max() < 2.0 ** (20 - q), (q, (np.abs(P) @ np.abs(Dt64[fin]).T).max())
    # masks
    n = r.cats.sum(1)
    assert set(np.unique(n)) <= {0.0, 1.0, 2.0, 4.0} and np.array_equal(np.flatnonzero(n == 0), dc.EMPTY)
    if weighted:
        assert not np.isin(r.cats, (0.0, 1.0)).all() and {0.5, 1.5, 2.0} <= set(np.unique(r.cats))
    else:
        assert np.isin(r.cats, (0.0, 1.0)).all()
    # negative and all-zero users
    for u in dc.NEGATIVE_USERS:
        assert (r.S[u][fin] < 0).all()
    for u in dc.ZERO_USERS:
        assert (r.S[u][fin] == 0).all()
    assert (r.S[8:][:, fin] > 0).any() and (r.S[8:][:, fin] < 0).any()
    # ties decide lists
    s, i = dc.lists(r.S, ALL_USERS, 64)
    assert (s[:, :-1] == s[:, 1:]).sum() >= 100


def test_reference_lists_are_the_oracles():
    from oracle import m2d_oracle as oracle
    for args, ingredients in (((3, 40, True), None), ((4, 64, False, True), True)):
        r = dc.exact_recipe(*args)
        users = dc.call_users(12)
        ws, wi = oracle.topk_catalogue(r.PM, r.RE, r.CE, r.cats, users, 64, r.coef, np.float64, ingredients=r.ing if ingredients else None)
        dc.assert_lists(*dc.lists(r.S, users, 64), ws, wi)
    r = dc.short_recipe(64)
    ws, wi = oracle.topk_catalogue(r.PM, r.RE[:14], r.CE, r.cats[:14], ALL_USERS, 14, r.coef)
    dc.assert_lists(*dc.lists(r.S, ALL_USERS, 14, 14), ws, wi)
    for r in (r, dc.remasked_recipe(64)):                     # the two recipes outside test_exact_recipes_are_exact: exact as well
        assert np.array_equal(dc.score_matrix(r, np.float32).astype(np.float64), r.S, equal_nan=True)
    assert dc.changed_lists(dc.lists(dc.remasked_recipe(64).S, ALL_USERS, 16), dc.lists(dc.exact_recipe(4, 64).S, ALL_USERS, 16)) >= 24


def test_where_empty_tied_and_negative_dishes_stand():
    E0 = np.asarray(dc.EMPTY)
    last = (dc.tiles(dc.I) - 1) * dc.TILE
    for tile in (E0[E0 < dc.TILE], E0[E0 >= last] - last):
        assert {0, 1} == set(((tile >> 2) & 1).tolist())       # both half-lanes of the first and of the last, partial tile
    assert dc.I % dc.TILE != 0
    for n in dc.RANGE_COUNTS[1:]:                             # empty dishes on both sides of every forced range boundary
        for lo, hi in dc.dish_ranges(dc.I, n)[1:]:
            if hi > lo:
                assert (E0 < lo).any() and (E0 >= lo).any()
    for n, b in ((2, 320), (3, 224), (7, 96), (8, 96)):        # ... and next to it
        assert b in [lo for lo, _ in dc.dish_ranges(dc.I, n)] and {b - 1, b} <= set(dc.EMPTY)
    # tied dishes stand on both sides of a boundary as NEIGHBOURS of a list: every (ranges, k) of the dish-range cases, users whose
    # scores are not all alike (the all-zero users tie every dish of every range with their list's last entry besides)
    others = ALL_USERS[8:]
    for C, E in ((4, 64), (4, 128)):
        r = dc.exact_recipe(C, E)
        for src, dst, n in dc.COPIES:
            keep = ~np.isin(np.arange(src, src + n), dc.EMPTY)      # (an emptied original's copy keeps its mask)
            assert np.array_equal(r.S[:, src:src + n][:, keep], r.S[:, dst:dst + n][:, keep]) and keep.sum() >= n - 2
        for n in dc.RANGE_COUNTS[1:]:
            for k in dc.RANGE_KS:
                assert dc.cross_range_ties(r.S, others, k, dc.I, n) >= 1, (E, n, k)
        assert dc.cross_range_ties(r.S, list(dc.ZERO_USERS), 33, 33, 2) == len(dc.ZERO_USERS)
    # the generic kernel's waves: tied neighbours whose ids are equal mod 4 and tied neighbours whose ids differ mod 4
    for C, E in dc.GENERIC_SHAPES:
        for w in (False, True):
            r = dc.exact_recipe(C, E, w)
            s, i = dc.lists(r.S, others, 64)
            tied = s[:, :-1] == s[:, 1:]
            same = (i[:, :-1] - i[:, 1:]) % 4 == 0
            assert (tied & same).sum() >= 1 and (tied & ~same).sum() >= 1, (C, E, w)
    # lists longer than the rankable dishes
    r = dc.short_recipe(64)
    n = r.cats.sum(1)
    assert np.array_equal(np.flatnonzero(n == 0), dc.SHORT_EMPTY) and (n[:dc.SHORT_CUT] == 0).sum() == 5
    s, i = dc.lists(r.S, ALL_USERS, 64)
    assert np.isnan(s[:, 60:]).all() and not np.isnan(s[:, :60]).any() and np.array_equal(i[0, 60:], dc.SHORT_EMPTY[:4])
    for k in (10, 14):
        s, i = dc.lists(r.S, ALL_USERS, k, dc.SHORT_CUT)
        assert np.isnan(s[:, 9:]).all() and not np.isnan(s[:, :9]).any()


# ---- stand-ins -----------------------------------------------------------------------------------------------------------------------------
def _refused(want, alt, what):
    assert dc.changed_lists(want, alt) >= 1, what
    with pytest.raises(AssertionError):
        dc.assert_lists(*alt, *want, what)


def _dish_edge_ks(n):
    return sorted({1, min(10, n), min(16, n), min(64, n)})


@pytest.mark.parametrize("E", (64, 128))
@pytest.mark.parametrize("weighted", (False, True))
def test_standin_pad_rows_rank(E, weighted):
    """(a): every dish-edge case whose last tile is partial, through the negative users (a pad row's 0 beats all they have)"""
    r = dc.exact_recipe(4, E, weighted)
    for n in dc.PREFIXES + (dc.I,):
        for k in _dish_edge_ks(n):
            want = dc.lists(r.S, ALL_USERS, k, n)
            alt = dc.standin_pad_rows(r.S, ALL_USERS, k, n)
            if n % dc.TILE == 0:
                assert dc.changed_lists(want, alt) == 0
                continue
            assert (np.asarray(alt[1])[list(dc.NEGATIVE_USERS), 0] >= n).all(), (n, k)
            _refused(want, alt, "pad rows, I = %d, k = %d" % (n, k))


@pytest.mark.parametrize("E", (64, 128))
def test_standins_of_the_dish_ranges(E):
    """(b) the last tile of every range dropped, (c) a tie across a range boundary to the higher range: every (ranges, k) of case 4"""
    r = dc.exact_recipe(4, E)
    for n_dishes, counts in ((dc.I, dc.RANGE_COUNTS), (33, (2, 3))):
        for n in counts:
            for k in dc.RANGE_KS if n_dishes == dc.I else dc.RANGE_KS_33:
                want = dc.lists(r.S, ALL_USERS, k, n_dishes)
                _refused(want, dc.standin_no_last_tile(r.S, ALL_USERS, k, n_dishes, n), "no last tile, %d ranges, k = %d" % (n, k))
                alt = dc.standin_tie_to_higher_range(r.S, ALL_USERS, k, n_dishes, n)
                if n == 1:
                    assert dc.changed_lists(want, alt) == 0
                else:
                    _refused(want, alt, "ties to the higher range, %d ranges, k = %d" % (n, k))
                    assert np.array_equal(sc.bits(np.nan_to_num(alt[0])), sc.bits(np.nan_to_num(want[0])))     # the same scores: only the ids tell


def test_standin_absent_descending():
    """(d): every case of lists longer than the rankable dishes"""
    r = dc.short_recipe(64)
    for n_dishes, k in ((dc.SHORT_I, 64), (dc.SHORT_CUT, 14)):
        want = dc.lists(r.S, ALL_USERS, k, n_dishes)
        _refused(want, dc.standin_absent_descending(r.S, ALL_USERS, k, n_dishes), "absent descending, I = %d" % n_dishes)
    # k = 10 of the 14: nine rankable dishes and one absent entry, the lowest absent id -- the stand-in lists the highest
    want = dc.lists(r.S, ALL_USERS, 10, dc.SHORT_CUT)
    alt = dc.standin_absent_descending(r.S, ALL_USERS, 10, dc.SHORT_CUT)
    assert (np.asarray(alt[1])[:, 9] == 13).all() and (np.asarray(want[1])[:, 9] == 0).all()
    _refused(want, alt, "absent descending, k = 10")
    dc.assert_whole_lists(want[1], dc.SHORT_CUT)
    with pytest.raises(AssertionError):
        dc.assert_whole_lists(np.where(np.isnan(want[0]), -1, want[1]), dc.SHORT_CUT)
    with pytest.raises(AssertionError):
        dc.assert_whole_lists(np.asarray(want[1])[:, [0, 0, 1]], dc.SHORT_CUT)


@pytest.mark.parametrize("C,E,weighted,ing", [(4, 128, False, False), (4, 128, True, False), (3, 160, False, False), (3, 160, True, False),
                                              (4, 128, False, True)])
def test_standin_no_second_k_stage(C, E, weighted, ing):
    """(e): every NB = 80 recipe, every k"""
    r = dc.exact_recipe(C, E, weighted, ing)
    alt = dc.standin_no_second_stage(r)
    fin = ~np.isnan(r.S)
    assert (alt[fin] != r.S[fin]).mean() > 0.5
    for k in dc.KS + (20,):
        _refused(dc.lists(r.S, ALL_USERS, k), dc.lists(alt, ALL_USERS, k), "no second stage, k = %d" % k)


# ---- normal tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", dc.NORMAL_MFMA + dc.NORMAL_GENERIC)
@pytest.mark.parametrize("weighted", (False, True))
def test_list_recipes_are_sharp_enough(E, weighted):
    for coef, k in dc.NORMAL_LISTS.items():
        r = dc.normal_recipe(E, weighted, coef)
        assert r.k == k and float(r.sharp.mean()) >= sc.MIN_SHARP, "E = %d, blend %g, k = %d: %.2f of the users are sharp only: inputs refused" % (
            E, coef, k, float(r.sharp.mean()))
        assert np.isnan(r.ref).all(0).sum() == len(dc.NORMAL_EMPTY) and set(np.unique(r.cats)) == ({0.0, 0.5, 1.0, 2.0} if weighted else {0.0, 1.0})
        good = sc.exact_lists(r.ref, r.dishes, k)
        assert sc.compare_lists(*good, r.ref, r.bound, r.dishes, k).mean() >= sc.MIN_SHARP
        if k > 1:
            with pytest.raises(AssertionError):                  # right scores, ids reversed
                sc.compare_lists(good[0], good[1][:, ::-1].copy(), r.ref, r.bound, r.dishes, k)
        lost = np.where((np.arange(r.I)[None, :] // dc.TILE) % 2 == 1, np.nan, r.ref)      # every second tile never scanned
        with pytest.raises(AssertionError):
            sc.compare_lists(*sc.exact_lists(lost, r.dishes, k), r.ref, r.bound, r.dishes, k)
