"""CPU checks of menu retrieval (m2d_topk_menu; build-defined): the boundary (header, ctypes table, built
library, engine method, torch op), the numpy restatement of the greedy against a plain Python loop, THE IDENTITY THE DESIGN RESTS ON
(the greedy over the full order equals the greedy over the merge of each signature's own top-k), float32 against float64 on the exact
recipes, the conditions the GPU cases of tests/test_gpu_menu.py rely on, and the wrong-kernel stand-ins under the same comparisons:
each must change the answer of every case aimed at it.

Of these cases only the two boundary cases fail without the feature (with all of tests/test_gpu_menu.py); the others check the test
inputs, the restatement and the stand-ins, and import nothing of the engine."""
import inspect
import os
import re

import numpy as np
import pytest

import deep_cases as dc
import menu_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    return open(os.path.join(ROOT, *path)).read()


# ---- the boundary --------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_in_the_header_the_ctypes_table_and_the_library():
    import ctypes as c
    from foodrec_amd import _native
    header = _read("include", "m2d.h")
    assert "int m2d_topk_menu(m2d_engine *h, const int32_t *users /* device [nU] */, int64_t nU, int32_t k," in header
    assert re.search(r"#define M2D_MENU_MAX_CATEGORIES %d\b" % mc.MAX_C, header)
    assert "NO reference counterpart (DESIGN.md 4.13)" in header and "ONE STREAM SYNCHRONISATION" in header
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    assert _native.SIGNATURES["m2d_topk_menu"] == (c.c_int, [vp, vp, i64, i32, vp, vp, vp, vp])
    assert getattr(_native.lib(), "m2d_topk_menu") is not None        # the built library exports it
    assert _native.ABI_VERSION == 2
    assert re.search(r"^SRCS\s*:=.*\bm2d_menu\.hip\b", _read("foodrec_amd", "csrc", "Makefile"), flags=re.M)
    eng = _read("foodrec_amd", "csrc", "m2d_engine.h")
    assert "if (tables & M2D_TAB_MASKS) h->menu_valid = false;" in eng
    assert "M2D_TAB_PM | M2D_TAB_RE | M2D_TAB_CE | M2D_TAB_MASKS, M2D_BY_CALLER" in _read("foodrec_amd", "csrc", "m2d_abi.hip")


def test_python_surface():
    import torch
    from foodrec_amd import ops, recommender
    assert list(inspect.signature(ops.ScoringEngine._topk_menu).parameters) == ["self", "users", "k", "caps"]
    sig = inspect.signature(recommender.Model.topk_menu)
    assert list(sig.parameters) == ["self", "users", "k", "caps"]
    assert sig.parameters["k"].default == 10 and sig.parameters["caps"].default is None
    users = torch.empty(7, dtype=torch.int32, device="meta")
    for caps in (torch.empty((7, 4), dtype=torch.int32, device="meta"), torch.empty(4, dtype=torch.int32, device="meta")):
        s, i = torch.ops.m2d.topk_menu(1, users, caps, 10)                          # the fake implementation
        assert s.shape == i.shape == (7, 10) and s.dtype == torch.float32 and i.dtype == torch.int32


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
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
    return C, I, k, cats, s, caps


def test_the_restatement_agrees_with_a_plain_loop():
    rng = np.random.default_rng(1)
    for t in range(400):
        C, I, k, cats, s, caps = _random_case(rng, one_signature=t % 10 == 0)
        order = mc.order_of(dc.words(s))
        want = mc.plain_menu(order, mc.signatures(cats), list(caps) + [0] * (mc.MAX_C - C), k)
        w, i = mc.menu_lists(s[None], cats, caps[None], k)
        assert i[0, :len(want)].tolist() == want and (i[0, len(want):] == -1).all() and (w[0, len(want):] == mc.NAN_WORD).all(), t
        assert np.array_equal(w[0, :len(want)], dc.words(s)[want])
    # planted rows: -0 / +0 tie to the lower id, NaN last in id order, an empty mask is never capped
    cats = mc._bits([1, 1, 2, 0, 3, 0, 1], 2)
    s = np.asarray([1.0, 1.0, 0.0, np.nan, -0.0, np.nan, 5.0], np.float32)
    assert mc.menu_lists(s[None], cats, [[1, 1]], 5)[1].tolist() == [[6, 2, 3, 5, -1]]
    assert mc.menu_lists(s[None], cats, [[2, 1]], 5)[1].tolist() == [[6, 0, 2, 3, 5]]
    assert mc.menu_lists(s[None], cats, [[3, 2]], 7)[1].tolist() == [[6, 0, 1, 2, 3, 5, -1]]      # 4 = {0, 1}: category 0 is full
    assert mc.menu_lists(s[None], cats, [[0, 0]], 3)[1].tolist() == [[3, 5, -1]]
    assert mc.menu_lists(s[None], cats, [[7, 7]], 7)[1].tolist() == [[6, 0, 1, 2, 4, 3, 5]] == dc.key_lists(s[None], 7)[1].tolist()


def test_the_identity_the_design_rests_on():
    """The greedy over the full order equals the greedy over the merged per-signature top-k lists: 3 000 random cases, C from 1 to 6,
    I up to 400, k up to 64, integer scores with heavy ties and normal scores, one-signature catalogues, caps 0 .. k + 1 -- and the
    caps matter in most of them, and leave rows short in many."""
    rng = np.random.default_rng(2)
    changed = short = 0
    for t in range(3000):
        C, I, k, cats, s, caps = _random_case(rng, one_signature=t % 10 == 0)
        full = mc.menu_lists(s[None], cats, caps[None], k)
        merged = mc.merged_menu(s[None], cats, caps[None], k, W=None if t % 3 else int(rng.integers(1, 50)))
        assert dc.same(full, merged), (t, C, I, k, caps.tolist())
        changed += int(not dc.same(full, dc.key_lists(s[None], k)))
        short += int(mc.short_rows(full)[0])
    assert changed > 1500 and short > 500, (changed, short)


@pytest.mark.parametrize("C,E", ((4, 4), (4, 64), (4, 200), (3, 64), (5, 64), (6, 64)))
def test_float32_equals_float64_on_the_exact_recipes(C, E):
    r = mc.exact_recipe(C, E, 1300 if E == 64 else 257)
    s64 = mc.host_scores(r)
    s32 = mc.host_scores(r, np.float32)
    assert np.array_equal(np.isnan(s64), np.isnan(s32)) and np.array_equal(s64[~np.isnan(s64)], s32[~np.isnan(s32)].astype(np.float64))
    assert np.isnan(s64[:, dc.nan_dishes(r.I)]).all()
    if C == 4:
        assert np.array_equal(dc.words(s32), dc.words(dc.exact_recipe(E, r.I).S.astype(np.float32)))     # the deep cases' own words


def test_tie_recipes_score_bit_equal_words_across_segments():
    for group in mc.TIE_GROUPS:
        r = mc.tie_recipe(group)
        s64, s32 = mc.host_scores(r), mc.host_scores(r, np.float32)
        assert np.array_equal(s64[~np.isnan(s64)], s32[~np.isnan(s32)].astype(np.float64))
        w = dc.words(s32)
        assert (w[:, r.copies] == w[:, r.copies[:1]]).all() and sorted(set(r.sig[r.copies])) == [1, 2]
        zero = w[r.U - 1][~np.isnan(s32[r.U - 1])]
        assert (zero << 1 == 0).all()                        # the all-zero user: one tie group over every segment


# ---- visibility: no GPU case can pass vacuously ---------------------------------------------------------------------------------------
def _capped_recipes():
    return ([mc.exact_recipe(C, 64, 1300) for C in (3, 4, 5, 6)] + [mc.normal_recipe(6, 64, 1300, form=f) for f in ("multi", "weighted", "negative", "minus_zero")]
            + [mc.segment_recipe(), mc.tie_recipe(2), mc.tie_recipe(65), mc.edge_recipe()])


def test_caps_change_the_lists_and_leave_rows_short():
    for r in _capped_recipes():
        W32 = mc.host_scores(r, np.float32, r.users)
        n = len(r.users)
        free = dc.key_lists(W32, 10)
        any_short = False
        for name in mc.CAP_SETS:
            got = mc.menu_lists(W32, r.cats, mc.cap_set(name, n, r.C, 10, mc.busiest(W32, r.cats)), 10)
            assert mc.changed_rows(got, free).mean() >= 0.5, (r.C, name)
            any_short |= bool(mc.short_rows(got).any())
        assert any_short, r.C
        assert dc.same(mc.menu_lists(W32, r.cats, mc.caps_uncapped(n, r.C, 64), 64), dc.key_lists(W32, 64))


def test_a_tie_group_straddles_two_segments_and_position_k():
    for group in mc.TIE_GROUPS:
        r = mc.tie_recipe(group)
        W32 = mc.host_scores(r, np.float32, r.users)
        assert len(r.users) >= 3 and r.users[-1] == r.U - 1
        for j in range(len(r.users) - 1):
            k = r.k[j]
            w, i = mc.menu_lists(W32[j:j + 1], r.cats, mc.caps_uncapped(1, r.C, k), k + 1 if k < 64 else k)
            at = np.flatnonzero(np.isin(i[0], r.copies))
            assert len(at) >= 2 and len(set(r.sig[i[0, at]])) == 2 and len(set(w[0, at])) == 1, (group, j)
            if k < 64:
                assert dc.straddles(W32[j], k)
        w, i = mc.menu_lists(W32[-1:], r.cats, mc.caps_uncapped(1, r.C, 10), 10)       # the all-zero user: one word, several segments
        assert len(set(w[0])) == 1 and len(set(r.sig[i[0]])) >= 2
    r = mc.edge_recipe()
    W32 = mc.host_scores(r, np.float32, r.users)
    assert len(r.edges) >= 8 and mc.edge_condition(mc.menu_lists(W32, r.cats, mc.caps_uncapped(len(r.users), 4, 64), 64)[1], r)
    S = mc.host_scores(r, np.float32)
    _, seg_off = mc.index(r.sig)
    for p in r.edges:                                        # by construction: each planted dish heads its segment for its user
        for d in (r.perm[p - 1], r.perm[p]):
            seg = r.perm[seg_off[r.sig[d]]:seg_off[r.sig[d] + 1]]
            assert S[p % r.U][d] == S[p % r.U][seg].max()


# ---- the stand-ins --------------------------------------------------------------------------------------------------------------------
def _aimed(standin):
    """(W32, cats, caps, k) of every case aimed at `standin`"""
    out = []
    if standin == "per_signature":           # two signatures share a category: per-signature counts let both fill it
        for r in (mc.exact_recipe(4, 64, 1300), mc.normal_recipe(6, 64, 1300)):
            out.append((mc.host_scores(r, np.float32, r.users), r.cats, mc.caps_all(len(r.users), r.C, 1), 10))
    elif standin == "higher_id":
        for g in mc.TIE_GROUPS:
            r = mc.tie_recipe(g)
            W32 = mc.host_scores(r, np.float32, r.users)
            for j in range(len(r.users)):
                out.append((W32[j:j + 1], r.cats, mc.caps_uncapped(1, r.C, r.k[j]), r.k[j]))
    elif standin == "cap_empty":             # caps exhausted: the empty-mask dishes fill the tail
        r = mc.exact_recipe(4, 64, 1300)
        out.append((mc.host_scores(r, np.float32, r.users), r.cats, mc.caps_all(len(r.users), 4, 1), 10))
        out.append((mc.host_scores(r, np.float32, r.users), r.cats, mc.caps_all(len(r.users), 4, 0), 5))
    elif standin == "readmit":
        for r in (mc.exact_recipe(4, 64, 1300), mc.normal_recipe(6, 64, 1300)):
            out.append((mc.host_scores(r, np.float32, r.users), r.cats, mc.caps_all(len(r.users), r.C, 1), 10))
            out.append((mc.host_scores(r, np.float32, r.users), r.cats, mc.caps_all(len(r.users), r.C, 2), 10))
    elif standin == "first_cap_cut":
        for r in (mc.exact_recipe(4, 64, 1300), mc.normal_recipe(6, 64, 1300)):
            out.append((mc.host_scores(r, np.float32, r.users), r.cats, mc.caps_zero_on(len(r.users), r.C, 10, 0), 10))
    elif standin == "minus_zero_member":
        r = mc.normal_recipe(6, 64, 1300, form="minus_zero")
        for name in ("one", "two"):
            out.append((mc.host_scores(r, np.float32, r.users), r.cats, mc.cap_set(name, len(r.users), r.C, 10), 10))
    return out


@pytest.mark.parametrize("standin", mc.STANDINS)
def test_every_standin_changes_the_answer_of_every_case_aimed_at_it(standin):
    cases = _aimed(standin)
    assert cases
    for W32, cats, caps, k in cases:
        right = mc.menu_lists(W32, cats, caps, k)
        assert dc.same(right, mc.merged_menu(W32, cats, caps, k, W=mc.RANGE_W))
        assert not dc.same(right, mc.menu_lists(W32, cats, caps, k, standin)), (standin, k)


def test_the_host_workaround_is_wrong_where_the_caps_are_not_filled_within_its_depth():
    r = mc.one_signature_recipe()
    W32 = mc.host_scores(r, np.float32, r.users)
    caps = mc.caps_zero_on(len(r.users), 4, 10, 3)           # every dish is {0, 2}: nothing is capped, but depth 5 ends the walk
    assert mc.short_rows(mc.host_workaround(W32, r.cats, caps, 10, 5)).all() and not mc.short_rows(mc.menu_lists(W32, r.cats, caps, 10)).any()
    r = mc.exact_recipe(4, 64, 1300)
    W32 = mc.host_scores(r, np.float32, r.users)
    caps = mc.caps_zero_on(len(r.users), 4, 10, 0)
    assert dc.same(mc.host_workaround(W32, r.cats, caps, 10, r.I), mc.menu_lists(W32, r.cats, caps, 10))
    assert not dc.same(mc.host_workaround(W32, r.cats, caps, 10, 12), mc.menu_lists(W32, r.cats, caps, 10))
