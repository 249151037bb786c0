"""CPU checks of household retrieval (m2d_topk_groups / m2d_score_groups_slate / m2d_topk_groups_slate; DESIGN.md section 4.12;
build-defined): the boundary (header, ctypes table, built library, engine methods, torch ops), the numpy restatement of the group
word against a plain Python loop on random and planted rows, the conditions the GPU cases of tests/test_gpu_groups.py rely on, and
the wrong-kernel stand-ins under the same comparisons: each must change the answer of every case aimed at it.

Of these cases only the three boundary cases fail without the feature (with all of tests/test_gpu_groups.py); the others check the
test inputs, the restatement and the stand-ins, and import nothing of the engine.

"last_tie" is aimed at the sign case (group_cases.sign_recipe: finite tables on which the slate kernels' chain ends in -0 for one
user and +0 for another).  "float_least" and "float_row0" are aimed at the NaN case (group_cases.nan_recipe: finite tables whose dish
vectors overflow, so that one member's word is a NaN where the others' are infinite or finite) -- an overflowing PRODUCT does not
do it (a fused multiply-add adds the exact product: -inf + 2.4e39 is -inf), an overflowing dish vector does (fma(0, inf, .) = NaN)."""
import inspect
import os
import re

import numpy as np
import pytest

import deep_cases as dc
import group_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2d_topk_groups", "m2d_score_groups_slate", "m2d_topk_groups_slate")


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_in_the_header_the_ctypes_table_and_the_library():
    import ctypes as c
    from foodrec_amd import _native
    header = _read("include", "m2d.h")
    for name in NEW:
        assert "int %s(m2d_engine *h" % name in header, name
        assert name in _native.SIGNATURES
        assert getattr(_native.lib(), name) is not None           # the built library exports it
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_topk_groups"][1] == [vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp]
    assert _native.SIGNATURES["m2d_score_groups_slate"][1] == [vp, vp, i64, i32, i32, vp, i64, vp, vp]
    assert _native.SIGNATURES["m2d_topk_groups_slate"][1] == [vp, vp, i64, i32, i32, vp, i64, i32, vp, vp, vp]
    assert _native.ABI_VERSION == 2
    for name, value in (("LEAST", gc.LEAST), ("MEAN", gc.MEAN), ("MOST", gc.MOST), ("MAX_MEMBERS", gc.MAX_MEMBERS)):
        assert re.search(r"#define M2D_GROUP_%s %d\b" % (name, value), header), name
    assert "NO reference counterpart (DESIGN.md 4.12)" in header and "KNOWN COST: filler rows are scored too" in header
    assert re.search(r"^SRCS\s*:=.*\bm2d_groups\.hip\b", _read("foodrec_amd", "csrc", "Makefile"), flags=re.M)
    src = _read("foodrec_amd", "csrc", "m2d_groups.hip")
    assert "GR_COLS = %d" % gc.GR_COLS in src and "m2d_block_rows(P, (int64_t)M * W, nG)" in src
    eng = _read("foodrec_amd", "csrc", "m2d_engine.h")
    assert "int m2d_slate_prepare(" in eng and "int m2d_launch_slate_scores(" in eng and "struct SlateArgs {" in eng


def test_python_surface():
    import torch
    from foodrec_amd import ops, recommender
    assert ops.GROUP_MODES == gc.MODES and ops.GROUP_MAX_MEMBERS == gc.MAX_MEMBERS
    assert list(inspect.signature(ops.ScoringEngine.topk_groups).parameters) == ["self", "members", "k", "mode", "exclude", "among"]
    assert list(inspect.signature(ops.ScoringEngine.score_groups).parameters) == ["self", "members", "slate", "mode"]
    sig = inspect.signature(recommender.Model.topk_group)
    assert list(sig.parameters) == ["self", "groups", "k", "mode", "exclude", "among", "market", "max_missing"]
    assert sig.parameters["k"].default == 10 and sig.parameters["mode"].default == "least"
    m = torch.empty((7, 5), dtype=torch.int32, device="meta")
    slate = torch.empty(9, dtype=torch.int32, device="meta")
    off, ids = torch.empty(8, dtype=torch.int64, device="meta"), torch.empty(3, dtype=torch.int32, device="meta")
    for got in (torch.ops.m2d.topk_groups(1, m, 300), torch.ops.m2d.topk_groups(1, m, 300, "mean", off, ids),
                torch.ops.m2d.topk_groups(1, m, 300, "most", None, None, slate)):
        s, i = got                                                                  # the fake implementations
        assert s.shape == i.shape == (7, 300) and s.dtype == torch.float32 and i.dtype == torch.int32
    out = torch.ops.m2d.score_groups(1, m, slate, "mean")
    assert out.shape == (7, 9) and out.dtype == torch.float32


def test_arguments_are_checked_before_the_native_call():
    import torch
    from foodrec_amd import ops
    eng = object.__new__(ops.ScoringEngine)                  # no engine: the checks stand in front of everything native
    eng.device = torch.device("cpu")
    with pytest.raises(ValueError, match="at most 64 members"):
        eng.topk_groups([[0] * 65], 5)
    with pytest.raises(ValueError, match="at most 64 members"):
        eng.score_groups([[1], list(range(65))], torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="cannot be combined"):
        eng.topk_groups([[0, 1]], 5, "least", [[3]], torch.zeros(8, dtype=torch.int32))
    for k in (0, 1025, True, 2.5):
        with pytest.raises(ValueError, match="1 <= k <= 1024"):
            eng.topk_groups([[0, 1]], k)
    for fn in (lambda: eng.topk_groups([[0]], 5, "median"), lambda: eng.score_groups([[0]], torch.zeros(3, dtype=torch.int32), "min")):
        with pytest.raises(ValueError, match="mode must be one of"):
            fn()
    padded = eng._group_members([[4], [7, 8, 7], []], "x")
    assert padded.dtype == torch.int32 and padded.tolist() == [[4, -1, -1], [7, 8, 7], [-1, -1, -1]]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _loop(S, members, mode):
    w = dc.words(S)
    cnt = gc.counts(members)
    out = np.zeros((len(members), S.shape[1]), np.uint32)
    for g in range(len(members)):
        for d in range(S.shape[1]):
            out[g, d] = gc.group_words_loop([w[members[g][j], d] for j in range(cnt[g])], mode)
    return out


def test_restatement_equals_the_plain_loop_on_random_rows():
    rng = np.random.default_rng(12)
    pool = np.concatenate([rng.standard_normal(30), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, np.nextafter(np.float32(1), 2), 3e38, -3e38]])
    for M in (1, 2, 3, 8):
        S = pool.astype(np.float32)[rng.integers(0, pool.size, (20, 200))]
        S[:10] = rng.standard_normal((10, 200)).astype(np.float32)
        members = gc.member_matrix(20, 2 * M + 3, M, seed=M)
        for mode in (gc.LEAST, gc.MEAN, gc.MOST):
            assert gc.same_words(gc.group_words(S, members, mode), _loop(S, members, mode), mode), (M, mode)
    assert gc.counts([[3, -1, 5], [1, 2, 3], [-1, -1, -1]]).tolist() == [1, 3, 0]


def _one(words, mode, standin=None):
    """the group word of one group whose member j holds words[j], through the matrix restatement"""
    S = np.asarray(words, np.float32).reshape(-1, 1)
    return int(gc.group_words(S, np.arange(len(S))[None], mode, standin=standin)[0, 0])


def test_restatement_on_the_planted_rows():
    w = lambda x: int(dc.words(np.float32(x)).ravel()[0])   # noqa: E731
    nz, pz, nan = w(-0.0), w(0.0), w(np.nan)
    nxt = np.nextafter(np.float32(1), np.float32(2))
    planted = [([-0.0, 0.0], nz, nz), ([0.0, -0.0], pz, pz),                        # -0 against +0, both orders: equal, the first wins
               ([1.5, 1.5, 1.5], w(1.5), w(1.5)),                                     # equal words
               ([1.0, np.nan, -2.0], nan, w(1.0)),                                    # one NaN member: worst for LEAST, never best
               ([np.nan, np.nan], nan, nan),                                          # all NaN
               ([np.inf, 1.0, -np.inf], w(-np.inf), w(np.inf)),
               ([1.0, nxt], w(1.0), w(nxt)), ([nxt, 1.0], w(1.0), w(nxt)),          # neighbouring floats
               ([-1.0, -nxt], w(-nxt), w(-1.0))]
    for words, least, most in planted:
        for mode, want in ((gc.LEAST, least), (gc.MOST, most)):
            assert _one(words, mode) == want == gc.group_words_loop(dc.words(np.asarray(words, np.float32)), mode), (words, mode)
    # ties to the last member show on the two zero rows only; a float minimum that ignores NaN on the NaN rows
    assert _one([-0.0, 0.0], gc.LEAST, "last_tie") == pz and _one([0.0, -0.0], gc.MOST, "last_tie") == nz
    assert _one([1.0, np.nan, -2.0], gc.LEAST, "float_least") == w(-2.0) and _one([np.nan, np.nan], gc.LEAST, "float_least") == w(np.inf)
    # a mean whose sequential sum differs from the pairwise sum in the last bit
    x = np.asarray([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], np.float32)
    seq = np.float32(np.float32(np.float32(x[0] + x[1]) + x[2]) + x[3])
    pair = np.float32(np.float32(x[0] + x[1]) + np.float32(x[2] + x[3]))
    assert abs(w(seq) - w(pair)) == 1
    assert _one(x, gc.MEAN) == w(seq / np.float32(4)) == gc.group_words_loop(dc.words(x), gc.MEAN)
    assert _one(x, gc.MEAN) != w(pair / np.float32(4))
    # one division, not a reciprocal: 5 / 3 differs from 5 * (1 / 3) in float32
    y = np.asarray([1.0, 2.0, 2.0], np.float32)
    assert _one(y, gc.MEAN) == w(np.float32(5) / np.float32(3)) != w(np.float32(5) * (np.float32(1) / np.float32(3)))
    assert _one([np.nan], gc.MEAN) == nan and _one([-0.0], gc.MEAN) == nz           # a group of one: the member's word


# ---- the stand-ins ---------------------------------------------------------------------------------------------------------------------
def _aimed(M, nD, mode):
    """The stand-ins aimed at the reduction-word case (M, nD, mode).  A wrong mean shows in every word; one member too many or too few
    under LEAST / MOST shows only in the columns where that member decides, so those stand-ins are aimed at the slates of 63 dishes
    and more (the shorter ones are there for the scalar and tail paths); the float minimum shows in the NaN column every slate of
    three or more dishes holds."""
    out = []
    if nD >= 63 and (mode == gc.MEAN or M <= 3):             # (the recipes hold 6 to 24 users: a group of 8 or 64 holds most of them already)
        out += ["next_group"] + (["forget_last"] if M >= 2 else [])
    if mode == gc.MEAN and nD >= 4:
        out += (["div_M"] if M >= 2 else []) + (["filler"] if M >= 3 else [])     # (M = 2: the one filler copies the one member: (a + a) / 2 = a)
    if mode == gc.LEAST and nD >= 3:
        out.append("float_least")
    return out


@pytest.mark.parametrize("tables,E", (("exact", 4), ("exact", 64), ("exact", 200), ("normal", 64)))
def test_wrong_kernel_standins_change_every_word_case_aimed_at_them(tables, E):
    r, S = gc.words_recipe(tables, E), gc.restated_matrix(tables, E)
    assert not np.nan_to_num(S[1]).any() and np.isnan(S[:, 5]).all()        # the all-zero user, a NaN column
    aimed = set()
    for M in gc.MEMBER_COUNTS:
        members = gc.member_matrix(r.U, gc.words_groups(M), M)
        cnt = gc.counts(members)
        assert set(cnt.tolist()) == set(range(1, M + 1)) and (M == 1 or (members[:, 1] == members[:, 0]).any())
        for nD in gc.SLATE_SIZES:
            slate = gc.slate_of(r.I, nD)
            assert np.all(np.diff(slate) > 0) and (nD < 3 or 5 in slate)
            for mode in (gc.LEAST, gc.MEAN, gc.MOST):
                want = gc.group_words(S[:, slate], members, mode)
                for s in _aimed(M, nD, mode):
                    assert not gc.same_words(gc.group_words(S[:, slate], members, mode, standin=s), want, mode), (M, nD, mode, s)
                    aimed.add(s)
    assert aimed == set(gc.STANDINS) - {"last_tie", "float_row0", "excl_row"}      # (those three: the sign, the NaN and the exclusion case below)


def test_the_sign_case_holds_both_zeros_and_infinities_and_the_tie_standin_changes_it():
    r, u = gc.sign_recipe(), gc.SIGN_USERS
    w = dc.words(r.S)
    assert (w[u["neg"], :4] == 0x80000000).all() and (w[u["pos"], :4] == 0).all() and (w[u["zero"]] == 0).all()
    assert (w[u["huge"], 4:6] == 0xFF800000).all() and (w[u["huge"], 6:] == 0x7F800000).all() and not np.isnan(r.S).any()
    assert np.isfinite(r.PM).all() and np.isfinite(r.RE).all() and np.isfinite(r.CE).all()      # finite tables: the calls serve them
    members = gc.sign_members()
    for mode in (gc.LEAST, gc.MOST):
        want = gc.group_words(r.S, members, mode)
        assert (want[0, :4] == 0x80000000).all() and (want[1, :4] == 0).all()       # -0 | +0 and +0 | -0: the first member's word
        assert not gc.same_words(gc.group_words(r.S, members, mode, standin="last_tie"), want, mode), mode
        assert np.array_equal(want, _loop(r.S, members, mode))
    # the float minimum that ignores NaN does not show here (no NaN): it is aimed at the NaN case below
    assert gc.same_words(gc.group_words(r.S, members, gc.LEAST, standin="float_least"), gc.group_words(r.S, members, gc.LEAST), gc.LEAST)
    assert gc.same_words(gc.group_words(r.S, members, gc.MEAN), _loop(r.S, members, gc.MEAN), gc.MEAN)


def test_the_nan_case_has_a_nan_in_one_member_alone_and_the_float_standins_change_it():
    r, u, multi = gc.nan_recipe(), gc.NAN_USERS, list(gc.NAN_MULTI)
    assert np.isfinite(r.PM).all() and np.isfinite(r.RE).all() and np.isfinite(r.CE).all()      # finite tables: the calls serve them
    w = dc.words(r.S)
    assert np.isnan(r.S[u["zero"], multi]).all() and np.isnan(r.S[u["opp"], multi]).all() and np.isfinite(r.S[:, 4:6]).all()
    assert (w[u["plain"], multi] == 0x7F800000).all() and (w[u["neg"], multi] == 0xFF800000).all()
    members = gc.nan_members()
    least, most = gc.group_words(r.S, members, gc.LEAST), gc.group_words(r.S, members, gc.MOST)
    for g in (0, 1, 2):                                      # a NaN member behind, in front of and between members without one
        assert np.isnan(least[g, multi].view(np.float32)).all() and (most[g, multi] == 0x7F800000).all()
    assert np.isnan(most[3, multi].view(np.float32)).all()
    for mode, want, standins in ((gc.LEAST, least, ("float_least", "float_row0")), (gc.MOST, most, ("float_row0",))):
        assert np.array_equal(want, _loop(r.S, members, mode))
        for s in standins:
            assert not gc.same_words(gc.group_words(r.S, members, mode, standin=s), want, mode), (mode, s)
    assert gc.same_words(gc.group_words(r.S, members, gc.MEAN), _loop(r.S, members, gc.MEAN), gc.MEAN)


def test_the_exclusion_standin_changes_the_exclusion_case():
    r, S = gc.normal_words()
    members = gc.list_members(r.U, nG=16)
    for mode in (gc.LEAST, gc.MEAN, gc.MOST):
        best = gc.group_lists(S, members, mode, 2)[1]
        lists = gc.exclusion_lists(r.I, len(members), best)
        assert [len(x) for x in lists[:4]] == [0, 1, 65, 300] and all(x == sorted(set(x)) for x in lists)
        edges = range(dc.RANGE_W, r.I, dc.RANGE_W)
        assert all(e - 2 in lists[2] and e + 1 in lists[2] for e in edges)       # excluded ids on both sides of every range edge
        want = gc.group_lists(S, members, mode, 300, lists)
        assert not dc.same(want, gc.group_lists(S, members, mode, 300))           # the exclusions matter
        # deep_chunk_pairs = 256: one group per block (g0 = g), so row g of the block is always list 0 -- the empty one
        assert not dc.same(want, gc.group_lists(S, members, mode, 300, lists, standin="excl_row", block=1)), mode


# ---- the conditions the GPU cases rely on --------------------------------------------------------------------------------------------
def test_least_misery_is_not_a_member_and_not_the_mean():
    r, S = gc.normal_words()
    members = gc.list_members(r.U)
    cnt = gc.counts(members)
    big = np.flatnonzero(cnt >= 2)
    assert big.size >= 6
    k = 10
    least = gc.group_lists(S, members, gc.LEAST, k)[1]
    mean = gc.group_lists(S, members, gc.MEAN, k)[1]
    own = dc.key_lists(S, k)[1]
    differs = [all(not np.array_equal(least[g], own[u]) for u in members[g, :cnt[g]]) for g in big]
    assert np.mean(differs) >= 0.5, differs
    assert np.mean([not np.array_equal(least[g], mean[g]) for g in big]) >= 0.5
    w = dc.words(S)
    other = []                                               # over those groups' columns: the worst member is not member 0
    for g in big:
        rows = gc.rank_half(w[members[g, :cnt[g]]])
        other.append(rows.argmax(0)[~np.isnan(S[members[g, 0]])] != 0)
    assert np.concatenate(other).mean() >= 1 / 3


@pytest.mark.parametrize("I", gc.LIST_SIZES)
def test_exact_list_recipes(I):
    r = dc.exact_recipe(64, I, U=3 if I > 2000 else 6)
    members = gc.list_members(r.U)
    assert set(gc.counts(members).tolist()) == {1, 2, 3, 4}
    S = r.S.astype(np.float32)
    assert gc.list_ks(I)[-1] == min(1024, I)
    w, i = gc.group_lists(S, members, gc.LEAST, min(1024, I))
    assert (i[:, -1] >= 0).all()
    tied = (w[:, :-1] == w[:, 1:]).sum()
    assert tied >= 10                                        # exact tables: equal group words, the lower id decides


def test_range_recipe_has_listed_and_excluded_dishes_on_both_sides_of_every_edge():
    r = dc.range_recipe("exact1300")
    S = r.S.astype(np.float32)
    members = gc.list_members(r.U)
    lists = dc.boundary_lists(r.I, dc.RANGE_W, len(members))[0]
    for mode in (gc.LEAST, gc.MEAN, gc.MOST):
        i = gc.group_lists(S, members, mode, 1024, lists)[1]
        assert dc.boundary_condition(i, lists, r.edges), mode
    assert dc.ranges(r.I, 256) == (256, 1) and 256 < 1024    # ranges narrower than k, one group per block
