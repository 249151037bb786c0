"""The MLP head's comparison (helpers.assert_mlp_scores) rejects wrong kernels and accepts a right one -- shown without a GPU,
with the oracle on altered inputs standing in for the kernel, on the five shapes the producer / consumer kernel exists for.

assert_scores_close alone does not: at the default blend 0.99 the C low-level blocks of z carry weight 0.01, and scores that
lost a whole 32-value period of one of them stay inside 1e-4 for a third to two thirds of the pairs they touch at E >= 128
(test_default_blend_hides_a_lost_period).  assert_mlp_scores therefore also demands, of the INPUTS, that losing any one period
of any block moves 80 % of the affected pairs by more than 10 bounds (helpers.mlp_visibility).  Blend 0.5 meets that on all
five shapes with random_case's tables and the scale-4 head -- narrowly at (256, 4): 0.76 to 0.84 over a dozen draws of the
tables, masks and head, 0.81 at the draw used here, >= 0.92 on the other shapes -- and 0.99 on none.  The all-categories pattern
is the hardest (each low-level block then enters with weight 0.5 / 4): 0.64 to 0.74 at (256, 4) on its own, which is why the GPU
tests that run whole batches of one pattern double the tables (test_doubled_tables_make_the_all_categories_pattern_visible)."""
import functools

import numpy as np
import pytest

from helpers import MLP_VISIBLE, TOL, assert_mlp_scores, mlp_case, mlp_head, mlp_periods, mlp_visibility, random_case

SHAPES = [(32, 5), (64, 2), (64, 4), (128, 4), (256, 4)]         # every (E, C) m2d_mlp_pc is instantiated for
U, I, B = 300, 200, 4096
NAN_DISH = 3


@functools.lru_cache(maxsize=None)
def _case(E, C, coef):
    from oracle import m2d_oracle as oracle
    PM, RE, CE, users, items, _ = random_case(U, I, C, E, B, seed=E)
    rng = np.random.default_rng(E * 7 + C)
    cats = rng.integers(0, 2, (I, C)).astype(np.float32)
    cats[cats.sum(1) == 0, 0] = 1                                # binary, non-empty ...
    cats[NAN_DISH] = 0                                           # ... but for one dish without categories: its score is NaN
    head = mlp_head((C + 1) * E, 256, 64, rng, scale=4.0)
    case = mlp_case(PM, RE, CE, cats, head, users, items, coef)
    ref = oracle.inference_mlp(PM, RE, CE, cats, *head, users, items, coef=coef)
    return case, ref


def _oracle(case, **over):
    from oracle import m2d_oracle as oracle
    a = dict(PM=case.PM, RE=case.RE, CE=case.CE, cats=case.cats, users=case.users, items=case.items, dtype=np.float64)
    a.update(over)
    return oracle.inference_mlp(a["PM"], a["RE"], a["CE"], a["cats"], *case.head, a["users"], a["items"], coef=case.coef, dtype=a["dtype"])


def _pattern(cats):
    return ((cats != 0) << np.arange(cats.shape[1])).sum(axis=1)


def _lost_period(case, ref):
    """One low-level period zeroed for the pairs of one mask pattern: the commonest pattern among the pairs, its first
    category, the block's last period."""
    pat = _pattern(case.cats)[case.items]
    pat[case.items == NAN_DISH] = 0
    q = np.bincount(pat[pat > 0]).argmax()
    c = int(np.flatnonzero((q >> np.arange(case.cats.shape[1])) & 1)[0])
    lo, hi = mlp_periods(case.PM.shape[2])[-1]
    PM = case.PM.copy()
    PM[:, c + 1, lo:hi] = 0
    got = ref.copy()
    sel = pat == q
    got[sel] = _oracle(case, PM=PM)[sel]
    return got, sel


def _stale_masks(case, ref):
    """The scores of the mask table BEFORE a set_dish_categories that gave every second dish with two or more categories one it did not have."""
    old = case.cats.copy()
    dishes = np.arange(0, I, 2)
    dishes = dishes[dishes != NAN_DISH]
    for d in dishes:
        on = np.flatnonzero(case.cats[d] != 0)
        if len(on) > 1:
            old[d, on[-1]] = 0                                   # (the new table turns this zero weight non-zero)
    turned = np.any((old == 0) & (case.cats != 0), axis=1)
    assert turned.mean() >= 0.10, turned.mean()
    return _oracle(case, cats=old), turned[case.items]


def _slots_swapped(case, ref):
    got = ref.copy()
    got[256:384], got[1024:1152] = ref[1024:1152], ref[256:384]
    return got, None


def _user_row_off_by_one(case, ref):
    return _oracle(case, users=(case.users + 1) % U), None


def _finite_for_a_dish_without_categories(case, ref):
    got = ref.copy()
    assert np.isnan(got).sum() == (case.items == NAN_DISH).sum() > 0
    got[np.isnan(got)] = 0.25
    return got, None


STAND_INS = [_lost_period, _stale_masks, _slots_swapped, _user_row_off_by_one, _finite_for_a_dish_without_categories]


@pytest.mark.parametrize("E,C", SHAPES)
def test_float32_restatement_passes(E, C):
    case, ref = _case(E, C, 0.5)
    err, vis = assert_mlp_scores(_oracle(case, dtype=np.float32), case, what="float32 restatement")
    assert vis >= MLP_VISIBLE and err < TOL


@pytest.mark.parametrize("stand_in", STAND_INS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("E,C", SHAPES)
def test_wrong_kernels_fail(E, C, stand_in):
    case, ref = _case(E, C, 0.5)
    got, _ = stand_in(case, ref)
    with pytest.raises(AssertionError, match="max err|NaN positions differ"):
        assert_mlp_scores(got, case, what=stand_in.__name__)


@pytest.mark.parametrize("E,C", SHAPES)
def test_even_blend_makes_every_period_visible(E, C):
    case, _ = _case(E, C, 0.5)
    vis = mlp_visibility(case.PM, case.RE, case.CE, case.cats, case.head, case.users, case.items, 0.5, detail=True)
    assert len(vis) == (C + 1) * len(mlp_periods(E))
    assert min(vis.values()) >= MLP_VISIBLE, min(vis.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("E,C", [(128, 4), (256, 4)])
def test_default_blend_hides_a_lost_period(E, C):
    """Why the coefficient matters: at 0.99 the inputs fail the condition (so assert_mlp_scores refuses them even for the right
    scores), and the lost-period stand-in stays inside assert_scores_close's bound for a large share of the pairs it touched."""
    case, ref = _case(E, C, 0.99)
    vis = mlp_visibility(case.PM, case.RE, case.CE, case.cats, case.head, case.users, case.items, 0.99, detail=True)
    assert min(vis.values()) < MLP_VISIBLE
    assert min(v for (b, _), v in vis.items() if b == 0) >= MLP_VISIBLE          # the high-level block is visible at any blend but 0
    with pytest.raises(AssertionError, match="visibility"):
        assert_mlp_scores(ref, case, what="the oracle itself")
    got, sel = _lost_period(case, ref)
    inside = np.abs(got[sel] - ref[sel]) <= TOL * np.maximum(1.0, np.abs(ref[sel]))
    assert sel.sum() > 100 and inside.mean() > 0.1, (sel.sum(), inside.mean())


@pytest.mark.parametrize("E,C", [(64, 2), (256, 4)])
def test_visibility_is_the_oracle_on_altered_tables(E, C):
    """mlp_visibility takes the altered scores from layer 1's linearity; the same share from oracle.inference_mlp on a
    Personal_Memory with that period zeroed."""
    case, ref = _case(E, C, 0.5)
    vis = mlp_visibility(case.PM, case.RE, case.CE, case.cats, case.head, case.users, case.items, 0.5, detail=True)
    for b, p in ((0, 0), (C, len(mlp_periods(E)) - 1), (1, 0)):
        lo, hi = mlp_periods(E)[p]
        PM = case.PM.copy()
        PM[:, b, lo:hi] = 0
        alt = _oracle(case, PM=PM)
        aff = np.isfinite(ref) & (True if b == 0 else case.cats[case.items, b - 1] != 0)
        share = np.mean(np.abs(alt[aff] - ref[aff]) > 10 * TOL * np.maximum(1.0, np.abs(ref[aff])))
        assert abs(share - vis[(b, p)]) <= 1.0 / aff.sum(), (b, p, share, vis[(b, p)])


def test_periods_and_ingredient_block():
    assert mlp_periods(6) == [(0, 6)] and mlp_periods(64) == [(0, 32), (32, 64)] and mlp_periods(200)[-1] == (160, 200)
    case, _ = _case(64, 4, 0.5)
    H = np.random.default_rng(0).standard_normal((I, 64)) / 8
    vis = mlp_visibility(case.PM, case.RE, case.CE, case.cats, case.head, case.users, case.items, 0.5, dish_high=H, detail=True)
    assert all(b != 0 for b, _ in vis) and len(vis) == 4 * 2


@pytest.mark.parametrize("E,C", SHAPES)
def test_doubled_tables_make_the_all_categories_pattern_visible(E, C):
    """tests/test_gpu_mlp.py's batches of ONE mask pattern use random_case's tables times two: with every category present
    each low-level block enters z with weight 0.5 / C, and at (256, 4) the pairs of that pattern alone miss the condition at
    random_case's scale and meet it at twice that."""
    case, _ = _case(E, C, 0.5)
    allc = (case.cats != 0).sum(axis=1)[case.items] == C
    assert allc.sum() > 100
    vis = lambda f: mlp_visibility(case.PM * f, case.RE * f, case.CE * f, case.cats, case.head, case.users[allc], case.items[allc], 0.5)
    assert vis(2.0) >= MLP_VISIBLE
    if (E, C) == (256, 4):
        assert vis(1.0) < MLP_VISIBLE
