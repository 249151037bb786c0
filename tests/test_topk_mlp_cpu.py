"""CPU checks of retrieval under the MLP head (m2d_topk_users_mlp / m2d_rank_candidates_mlp): the boundary (header, exported
symbols, ctypes table), the conditions on every input recipe tests/test_gpu_topk_mlp.py uses -- evaluated with the oracle alone,
so a refused input shows up here and not on the GPU -- and the list comparison itself against stand-ins that must not pass."""
import os
import re

import numpy as np
import pytest

import topk_mlp_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2d_topk_users_mlp", "m2d_rank_candidates_mlp")


def test_symbols_declared_exported_and_bound(native_lib):
    from foodrec_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m2d.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "include/m2d.h does not declare %s" % name
        assert hasattr(native_lib, name), "libm2d.so does not export %s" % name
        assert name in _native.SIGNATURES
    # the ctypes rows follow the header's parameter lists: (engine, users, nU, k, candidates, scores, ids, stream) and
    # m2d_rank_candidates' own list
    vp, i64, i32 = _native._vp, _native._i64, _native._i32
    assert _native.SIGNATURES["m2d_topk_users_mlp"][1] == [vp, vp, i64, i32, i32, vp, vp, vp]
    assert _native.SIGNATURES["m2d_rank_candidates_mlp"] == _native.SIGNATURES["m2d_rank_candidates"]
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(decl.split(",")) == len(_native.SIGNATURES[name][1]), name
    assert native_lib.m2d_abi_version() == 2 == _native.ABI_VERSION


def test_python_surface_without_a_device():
    import inspect
    import torch
    from foodrec_amd import ops, recommender
    assert list(inspect.signature(ops.ScoringEngine.topk_users_mlp).parameters) == ["self", "users", "k", "candidates"]
    assert inspect.signature(ops.ScoringEngine.rank_candidates).parameters["head"].default is False
    p = inspect.signature(recommender.Model.topk).parameters
    assert (p["k"].default, p["exclude"].default, p["head"].default, p["candidates"].default) == (10, None, False, 0)
    assert hasattr(torch.ops.m2d, "topk_users_mlp")
    s, i = torch.ops.m2d.topk_users_mlp(1, torch.empty(7, dtype=torch.int32, device="meta"), 5, 0)     # the fake implementation
    assert (tuple(s.shape), s.dtype, tuple(i.shape), i.dtype) == ((7, 5), torch.float32, (7, 5), torch.int32)


@pytest.mark.parametrize("name", sorted(tc.CONDITIONED))
def test_recipe_meets_both_conditions(name):
    r = tc.recipe(name)
    tc.assert_conditions(tc.reference(name), tc.base_scores(r, r.users), tc.CONDITIONED[name], what=name)


def test_generic_recipe_has_sharp_users_at_k64():
    """Its input conditions are asked at k = 10 (topk_mlp_cases.CONDITIONED); at its own k = 64 exact ids are still asserted for
    the users sharp there: there must be a fair number of them."""
    rs, _ = tc.ranked(tc.reference("generic"))
    assert tc.sharp_users(rs, 64).mean() >= 0.3


def _stage_candidates(r, users, K1):
    """The K1 best by the base score, as the oracle ranks them (the GPU tests take them from ScoringEngine.topk_users)."""
    base = tc.base_scores(r, users)
    _, bi = tc.ranked(base)
    cand = bi[:, :K1]
    return cand, np.take_along_axis(base, cand, axis=1)


def test_two_stage_recipes_meet_the_conditions_within_the_candidates():
    r = tc.recipe("stage3000")
    users = r.users[:400]                                    # a sample of the 3 000: a share, not a census
    cand, base = _stage_candidates(r, users, 64)
    tc.assert_conditions(tc.head_scores(r, users, cand), base, 10, cand, what="K1 = 64, k = 10")
    cand, _ = _stage_candidates(r, users, 16)                # K1 = k: the id set is the candidate set, only the order is the head's
    rs, ri = tc.ranked(tc.head_scores(r, users, cand), cand)
    assert tc.sharp_users(rs, 16).mean() >= tc.MIN_SHARE
    assert np.mean([not np.array_equal(a, b) for a, b in zip(ri, cand)]) >= tc.MIN_SHARE
    r = tc.recipe("i33")
    cand, base = _stage_candidates(r, r.users, 33)
    tc.assert_conditions(tc.head_scores(r, r.users, cand), base, 10, cand, what="K1 = I = 33")


def test_tie_recipe_holds_listed_pairs_and_a_split_pair():
    r, ref = tc.recipe("ties"), tc.reference("ties")
    assert np.array_equal(ref[:, :tc.TIE_COPIES], ref[:, tc.TIE_SHIFT:tc.TIE_SHIFT + tc.TIE_COPIES])
    _, ri = tc.ranked(ref)
    both = sum(1 for row in ri for d in row[:r.k] if d < tc.TIE_COPIES and d + tc.TIE_SHIFT in row[:r.k])
    split = sum(1 for row in ri if row[r.k - 1] < tc.TIE_COPIES and row[r.k] == row[r.k - 1] + tc.TIE_SHIFT)
    assert both >= 5 and split >= 1, (both, split)


def test_nan_recipe_has_ten_rankable_dishes():
    r, ref = tc.recipe("nan40"), tc.reference("nan40")
    assert (r.cats.sum(1) == 0).sum() == 30 and np.array_equal(np.isnan(ref[0]), r.cats.sum(1) == 0)


def _reference_lists(name, k):
    rs, ri = tc.ranked(tc.reference(name))
    return rs[:, :k].copy(), ri[:, :k].copy()


def test_comparison_accepts_the_reference_and_rejects_stand_ins():
    r, ref = tc.recipe("pc"), tc.reference("pc")
    s, i = _reference_lists("pc", r.k)
    sharp = tc.compare_lists(s, i, ref, r.k)
    assert sharp.mean() >= tc.MIN_SHARE
    # an engine that ignores the head: the base lists
    bs, bi = tc.ranked(tc.base_scores(r, r.users))
    with pytest.raises(AssertionError):
        tc.compare_lists(bs[:, :r.k], bi[:, :r.k], ref, r.k)
    # ... or returns the base ids with head scores
    with pytest.raises(AssertionError):
        tc.compare_lists(np.take_along_axis(ref, bi[:, :r.k], axis=1), bi[:, :r.k], ref, r.k)
    # two adjacent sharp entries swapped (ids and scores together: the list is then out of order; ids alone: not the reference's)
    j = int(np.flatnonzero(sharp)[0])
    s2, i2 = s.copy(), i.copy()
    s2[j, [3, 4]], i2[j, [3, 4]] = s2[j, [4, 3]], i2[j, [4, 3]]
    with pytest.raises(AssertionError):
        tc.compare_lists(s2, i2, ref, r.k)
    i3 = i.copy()
    i3[j, [3, 4]] = i3[j, [4, 3]]
    with pytest.raises(AssertionError):
        tc.compare_lists(s, i3, ref, r.k)


def test_comparison_rejects_a_tie_pair_in_descending_id():
    r, ref = tc.recipe("ties"), tc.reference("ties")
    s, i = _reference_lists("ties", r.k)
    tc.compare_lists(s, i, ref, r.k)
    rows = [(j, a) for j in range(i.shape[0]) for a in range(r.k - 1) if i[j, a] < tc.TIE_COPIES and i[j, a + 1] == i[j, a] + tc.TIE_SHIFT]
    assert rows
    j, a = rows[0]
    assert s[j, a] == s[j, a + 1]
    i[j, [a, a + 1]] = i[j, [a + 1, a]]
    with pytest.raises(AssertionError, match="order broken"):
        tc.compare_lists(s, i, ref, r.k)


def test_comparison_orders_nan_entries_last_by_id():
    r, ref = tc.recipe("nan40"), tc.reference("nan40")
    s, i = _reference_lists("nan40", r.k)
    tc.compare_lists(s, i, ref, r.k)
    empty = np.flatnonzero(r.cats.sum(1) == 0)
    assert np.array_equal(i[0, 10:], empty[:6]) and np.isnan(s[0, 10:]).all() and not np.isnan(s[0, :10]).any()
    i[0, [10, 11]] = i[0, [11, 10]]
    with pytest.raises(AssertionError, match="NaN entries"):
        tc.compare_lists(s, i, ref, r.k)


def test_chunk_geometry_of_the_documented_cases():
    assert tc.chunk_geometry(37, 1000, 32768) == (1000, 32, 2)          # 32 rows x 1 000 = 32 000 pairs, the last block partial
    assert tc.chunk_geometry(37, 1000, 4096) == (1000, 4, 10)
    assert tc.chunk_geometry(37, 1000, 256) == (256, 1, 37 * 4)
    assert tc.chunk_geometry(37, 1000, 1 << 22) == (1000, 37, 1)
    assert tc.chunk_geometry(24, 5000, 2048) == (2048, 1, 24 * 3)       # ranges of 2 048, 2 048 and 904
    assert tc.chunk_geometry(3000, 1000, 1 << 22, candidates=64) == (64, 3000, 1)
