"""The inputs of the non-finite GPU tests (helpers.nonfinite_case), checked on the CPU against the float64 restatement alone:
every case holds the scores it is there for (+-inf, NaN made by the poison, finite ones), the float32 restatement agrees on
where they are, and a numpy stand-in of the C = 4 kernels' lane arithmetic shows which cases tell the two idle-lane rules apart.
Plus oracle.topk_catalogue's order of -inf and NaN scores."""
import numpy as np
import pytest

from helpers import (NONFINITE_COLS, NONFINITE_E_FULL, NONFINITE_E_PARTIAL, NONFINITE_TABLES, NONFINITE_VALUES,
                     assert_scores_match_nonfinite, c4_lane_standin, nonfinite_case, nonfinite_case_conditions, nonfinite_patterns)

# (C, E, B) of the pair launches of test_gpu_nonfinite.py
SHAPES = ([(4, E, 300) for E in NONFINITE_E_PARTIAL + NONFINITE_E_FULL] + [(4, 24, 9000), (4, 200, 9000), (4, 256, 9000)] +
          [(3, 16, 9000), (6, 36, 9000), (4, 7, 300), (9, 64, 300)])


def _cases(C, E, B):
    for table in NONFINITE_TABLES:
        for col in NONFINITE_COLS:
            for value in NONFINITE_VALUES:
                yield nonfinite_case(C, E, B, table, col, value, seed=E + C)


def test_patterns_hold_every_mask_once():
    pat = nonfinite_patterns(4, np.random.default_rng(0))
    assert pat.shape == (20, 4)
    binary = [tuple(p) for p in pat if set(p.tolist()) <= {0.0, 1.0}]
    assert len(set(binary)) == 16 and len(binary) == 16                     # 15 non-empty patterns and the empty one
    weighted = [p for p in pat if not set(p.tolist()) <= {0.0, 1.0}]
    assert len(weighted) == 4 and all((p != 0).all() for p in weighted)
    for C in (3, 6, 9):
        assert nonfinite_patterns(C, np.random.default_rng(0)).shape == (20, C)


@pytest.mark.parametrize("C,E,B", SHAPES)
def test_every_case_holds_the_scores_it_is_there_for(C, E, B):
    from oracle import m2d_oracle as oracle
    for case in _cases(C, E, B):
        nonfinite_case_conditions(case)
        # the poisoned element is the only difference, and it sits where `col` says
        diff = [np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).ravel()) for a, b in
                ((case.PM, case.PM0), (case.RE, case.RE0), (case.CE, case.CE0))]
        assert sum(len(x) for x in diff) == 1
        assert case.e == (1 if case.col == "first" else E - 1)
        # the float32 restatement: NaN and +-inf at the same pairs (on the pairs the poison reaches, and once on all)
        t = np.flatnonzero(case.touched)
        f32 = oracle.inference_f32(case.PM, case.RE, case.CE, case.users[t], case.items[t], case.cats[t])
        assert np.array_equal(np.isnan(f32), np.isnan(case.ref[t]))
        inf = np.isinf(case.ref[t])
        assert np.array_equal(np.isinf(f32), inf) and np.array_equal(f32[inf], case.ref[t][inf])
    f32 = oracle.inference_f32(case.PM0, case.RE0, case.CE0, case.users, case.items, case.cats)
    assert np.array_equal(np.isnan(f32), np.isnan(case.ref0)) and not np.isinf(f32).any() and not np.isinf(case.ref0).any()


def test_reference_subset_equals_the_whole():
    sel = np.r_[0:64, 64:300:7]
    for table in NONFINITE_TABLES:
        whole = nonfinite_case(4, 24, 300, table, "first", np.inf, seed=28)
        part = nonfinite_case(4, 24, 300, table, "first", np.inf, seed=28, ref_on=sel)
        assert np.array_equal(part.ref, whole.ref[sel], equal_nan=True)
        assert np.array_equal(part.touched, whole.touched[sel])


@pytest.mark.parametrize("E", NONFINITE_E_PARTIAL + NONFINITE_E_FULL)
def test_lane_standin_tells_the_idle_lane_rules_apart(E):
    """The rule "idle lanes keep hs" (cef = 0 times the re-read column 0 of U_high) must fail on U_high / first / +-inf where the
    lane group is partial, and nowhere else; "idle lanes zero hs" passes everything.  So the GPU cases can see that fault."""
    for case in _cases(4, E, 300):
        args = (case.PM, case.RE, case.CE, case.users, case.items, case.cats)
        assert_scores_match_nonfinite(c4_lane_standin(*args, zero_idle_hs=True), case.ref, what="zeroed")
        kept = c4_lane_standin(*args, zero_idle_hs=False)
        expect_fail = (E in NONFINITE_E_PARTIAL and case.table == "U_high" and case.col == "first" and np.isinf(case.value))
        if expect_fail:
            with pytest.raises(AssertionError):
                assert_scores_match_nonfinite(kept, case.ref, what="kept")
            ok = ~case.touched                                   # ... and only on the poisoned user's pairs
            assert_scores_match_nonfinite(kept[ok], case.ref[ok], what="kept, other users")
        else:
            assert_scores_match_nonfinite(kept, case.ref, what="kept")


def test_topk_catalogue_ranks_minus_inf_before_nan():
    """One dish that scores -inf and one of LOWER id that scores NaN: -inf comes first (include/m2d.h: NaN scores last)."""
    from oracle import m2d_oracle as oracle
    from helpers import random_case
    U, I, C, E = 3, 12, 4, 8
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=2)
    cats = np.ones((I, C), np.float32)
    cats[4] = 0                                                  # dish 4: empty mask, 0 / 0 = NaN
    RE = RE.copy(); RE[9, 3] = -np.inf                           # dish 9: -inf for a user whose low rows are positive there
    PM = PM.copy(); PM[1, 1:, 3] = np.abs(PM[1, 1:, 3])
    s, i = oracle.topk_catalogue(PM, RE, CE, cats, [1], I)
    assert np.isneginf(s[0, I - 2]) and i[0, I - 2] == 9 and np.isnan(s[0, I - 1]) and i[0, I - 1] == 4
    assert np.all(np.diff(s[0, :I - 1]) <= 0) and np.isfinite(s[0, :I - 2]).all()
    cats[2] = 0                                                  # two NaN dishes: by id, both after -inf
    s, i = oracle.topk_catalogue(PM, RE, CE, cats, [1], I)
    assert i[0, -3:].tolist() == [9, 2, 4]
    s, i = oracle.topk_catalogue(PM, RE, CE, cats, [1], I - 2)    # k cuts inside the tail: the -inf dish is in, the NaN dishes are not
    assert i[0, -1] == 9
