"""GPU tests of retrieval and candidate ranking under the MLP head (m2d_topk_users_mlp, m2d_rank_candidates_mlp; DESIGN.md
section 8): the lists against the oracle's float64 head scores ordered by oracle.topk_catalogue's rule, through every head kernel
family, across the launcher's chunk edges, with ties and NaN scores, in the two-stage form, with the ingredient table, on a
user-range shard, after writers, and the argument checks.  Inputs, conditions and the comparison: tests/topk_mlp_cases.py."""
import functools
import types

import numpy as np
import pytest

import topk_mlp_cases as tc
from helpers import mlp_head

pytestmark = pytest.mark.gpu

DEFAULT_P = 1 << 22


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(r, head=True, masks=True, tables=None, user_base=0):
    from foodrec_amd import ScoringEngine
    PM, RE, CE = tables if tables is not None else (r.PM, r.RE, r.CE)
    eng = ScoringEngine(PM, RE, CE, coef=r.coef, user_base=user_base)
    if masks:
        eng.set_dish_categories(r.cats)
    if r.ing is not None:
        eng.set_ingredients(*r.ing)
    if head:
        eng.set_mlp_head(*(r.head if head is True else head))
    return eng


def _lists(eng, users, k, candidates=0, chunk=None):
    """(scores f32 [n, k], ids i32 [n, k]) as numpy, the id latch checked."""
    if chunk is not None:
        eng.set_option("topk_mlp_chunk_pairs", chunk)
    s, i = eng.topk_users_mlp(_dev(users), k, candidates)
    eng.check()
    return s.cpu().numpy(), i.cpu().numpy()


def _same(a, b):
    """Same ids, same score bits."""
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


@functools.lru_cache(maxsize=None)
def _exact(name):
    """The recipe's exact-mode lists at the default chunk, and the kernel that scored them (computed once, read-only)."""
    r = tc.recipe(name)
    eng = _engine(r)
    got = _lists(eng, r.users, r.k)
    kernel, launches = eng.last_kernel(), eng.get_option("topk_mlp_launches")
    eng.close()
    return got, kernel, launches


# ---- 1. exact mode against the oracle, one case per head kernel family ------------------------------------------------------
@pytest.mark.parametrize("name,kernel", [("pc", "m2d_mlp_pc_bf16x3"), ("gather", "m2d_mlp_mfma_bf16x3"),
                                         ("generic", "m2d_mlp_generic"), ("e128", "m2d_mlp_pc_bf16x3")])
def test_exact_mode_matches_the_oracle(name, kernel):
    r, ref = tc.recipe(name), tc.reference(name)
    differ, sharp = tc.assert_conditions(ref, tc.base_scores(r, r.users), tc.CONDITIONED[name], what=name)
    (s, i), ran, launches = _exact(name)
    assert ran == kernel
    assert launches == tc.chunk_geometry(len(r.users), r.I, DEFAULT_P)[2] == 1
    is_sharp = tc.compare_lists(s, i, ref, r.k, what=name)
    print("%s: lists differing from the base %.2f, sharp at k = %d: %.2f" % (name, differ, r.k, is_sharp.mean()))


# ---- 2. chunk edges -----------------------------------------------------------------------------------------------------------
def test_chunk_edges_give_the_same_lists_bit_for_bit():
    """16 384 pairs is where the head's launcher starts grouping pairs by mask pattern: chunks of 32 000 pairs are grouped, of
    4 000 and of 256 are not, the default takes all 37 000 in one launch.  The last user block is partial at 4 096 and 32 768."""
    r = tc.recipe("pc")
    want, _, _ = _exact("pc")
    eng = _engine(r)
    for P in (256, 4096, 32768, DEFAULT_P):
        got = _lists(eng, r.users, r.k, chunk=P)
        assert eng.get_option("topk_mlp_chunk_pairs") == P
        assert eng.get_option("topk_mlp_launches") == tc.chunk_geometry(len(r.users), r.I, P)[2], P
        assert _same(got, want), "chunk %d" % P
    for bad in (255, (1 << 24) + 1, 0, -1):
        with pytest.raises(ValueError):
            eng.set_option("topk_mlp_chunk_pairs", bad)
    assert eng.get_option("topk_mlp_chunk_pairs") == DEFAULT_P
    eng.close()


def test_running_list_merges_across_three_dish_ranges():
    r, ref = tc.recipe("pc5000"), tc.reference("pc5000")
    tc.assert_conditions(ref, tc.base_scores(r, r.users), tc.CONDITIONED["pc5000"], what="pc5000")
    want, _, _ = _exact("pc5000")
    tc.compare_lists(*want, ref, r.k, what="pc5000, one range")
    eng = _engine(r)
    got = _lists(eng, r.users, r.k, chunk=2048)
    assert eng.get_option("topk_mlp_launches") == 24 * 3 == tc.chunk_geometry(len(r.users), r.I, 2048)[2]
    assert _same(got, want)
    # every range holds some user's listed dishes, so the merge is what produced these lists
    assert all(((want[1] >= lo) & (want[1] < hi)).any() for lo, hi in ((0, 2048), (2048, 4096), (4096, 5000)))
    eng.close()


# ---- 3. ties and NaN, exact -----------------------------------------------------------------------------------------------------
def test_tied_copies_in_different_dish_ranges_go_to_the_lower_id():
    r, ref = tc.recipe("ties"), tc.reference("ties")
    eng = _engine(r)
    s, i = _lists(eng, r.users, r.k, chunk=2048)                    # ranges [0, 2048) and [2048, 2200): the copies sit in the second
    assert eng.get_option("topk_mlp_launches") == 2 * len(r.users)
    eng.close()
    tc.compare_lists(s, i, ref, r.k, what="ties")
    both = split = 0
    for j in range(len(r.users)):
        row = i[j].tolist()
        for a, d in enumerate(row):
            if d >= tc.TIE_SHIFT and d < tc.TIE_SHIFT + tc.TIE_COPIES:
                assert a > 0 and row[a - 1] == d - tc.TIE_SHIFT, "user %d: copy %d is not right behind its original: %s" % (j, d, row)
                assert s[j, a].view(np.int32) == s[j, a - 1].view(np.int32)
                both += 1
        _, ri = tc.ranked(ref[j:j + 1])
        if ri[0, r.k - 1] < tc.TIE_COPIES and ri[0, r.k] == ri[0, r.k - 1] + tc.TIE_SHIFT:
            assert row[-1] == ri[0, r.k - 1], "user %d: the pair split at position k keeps the lower id" % j
            split += 1
    assert both >= 5 and split >= 1, (both, split)


def test_empty_mask_dishes_come_last_in_id_order():
    r, ref = tc.recipe("nan40"), tc.reference("nan40")
    eng = _engine(r)
    s, i = _lists(eng, r.users, r.k)
    eng.close()
    tc.compare_lists(s, i, ref, r.k, what="nan40")
    empty = np.flatnonzero(r.cats.sum(1) == 0)
    for j in range(len(r.users)):
        assert not np.isnan(s[j, :10]).any() and np.isnan(s[j, 10:]).all()
        assert np.array_equal(i[j, 10:], empty[:6]), (j, i[j])
        assert set(i[j, :10].tolist()) == set(np.flatnonzero(r.cats.sum(1) > 0).tolist())


# ---- 4. two-stage mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K1,k", [("stage3000", 64, 10), ("stage3000", 16, 16), ("i33", 33, 10)])
def test_two_stage_reranks_the_retrieved_candidates(name, K1, k):
    r = tc.recipe(name)
    eng = _engine(r)
    _, cand = eng.topk_users(_dev(r.users), K1)                      # stage 1 on its own: covered by its own tests
    eng.check()
    cand = cand.cpu().numpy().astype(np.int64)
    s, i = _lists(eng, r.users, k, candidates=K1)
    assert eng.get_option("topk_mlp_launches") == 1
    ref = tc.head_scores(r, r.users, cand)
    if K1 > k:
        tc.assert_conditions(ref, tc.base_scores(r, r.users, cand), k, cand, what="%s K1 = %d" % (name, K1))
    else:
        assert tc.sharp_users(tc.ranked(ref, cand)[0], k).mean() >= tc.MIN_SHARE
    sharp = tc.compare_lists(s, i, ref, k, ids=cand, what="%s K1 = %d" % (name, K1))
    if K1 == r.I:                                                    # every dish is a candidate: the exact mode's lists
        es, ei = _lists(eng, r.users, k)
        assert np.array_equal(ei[sharp], i[sharp])
        tc.compare_lists(es, ei, tc.reference(name), k, what="i33 exact")
    # a smaller chunk cuts the users into blocks, stage 1 runs per block: the same lists
    if name == "stage3000" and K1 == 64:
        again = _lists(eng, r.users, k, candidates=K1, chunk=65536)
        assert eng.get_option("topk_mlp_launches") == tc.chunk_geometry(3000, r.I, 65536, K1)[2] == 3
        assert _same(again, (s, i))
    eng.close()


# ---- 5. ingredient table set ----------------------------------------------------------------------------------------------------
def test_exact_mode_with_the_ingredient_table():
    r, ref = tc.recipe("ing"), tc.reference("ing")                   # inference_mlp(..., dish_high=H)
    tc.assert_conditions(ref, tc.base_scores(r, r.users), tc.CONDITIONED["ing"], what="ing")
    (s, i), kernel, _ = _exact("ing")
    assert kernel == "m2d_mlp_pc_bf16x3"
    tc.compare_lists(s, i, ref, r.k, what="ing")
    # the table matters: without it the lists are others
    plain = types.SimpleNamespace(**{**vars(r), "ing": None, "H": None})
    eng = _engine(plain)
    assert not np.array_equal(_lists(eng, r.users, r.k)[1], i)
    eng.close()


# ---- 6. user_base ---------------------------------------------------------------------------------------------------------------
def test_user_base_keeps_ids_global_and_latches_the_id_below_it():
    r = tc.recipe("pc")
    want, _, _ = _exact("pc")
    eng = _engine(r, user_base=7000)
    for cand in (0, 64):
        ref_eng = _engine(r)
        plain = _lists(ref_eng, r.users, r.k, candidates=cand)
        ref_eng.close()
        assert _same(_lists(eng, r.users + 7000, r.k, candidates=cand), plain)
    assert _same(_lists(eng, r.users + 7000, r.k), want)
    bad = (r.users + 7000).copy()
    bad[5] = 6999
    eng.topk_users_mlp(_dev(bad), r.k)
    with pytest.raises(IndexError, match="user id 6999"):
        eng.check()
    assert _same(_lists(eng, r.users + 7000, r.k), want)            # the engine stays usable
    eng.close()


# ---- 7. readers after writers ---------------------------------------------------------------------------------------------------
def test_lists_follow_table_edits_and_a_new_head():
    import torch
    r = tc.recipe("pc")
    rng = np.random.default_rng(77)
    eng = _engine(r)
    modes = (0, 64)
    before = [_lists(eng, r.users, r.k, candidates=c) for c in modes]
    RE2 = (rng.standard_normal(r.RE.shape) * 0.5).astype(np.float32)
    eng.re.copy_(torch.as_tensor(RE2))                               # in place: the engine borrows this tensor
    eng.tables_updated()
    after = [_lists(eng, r.users, r.k, candidates=c) for c in modes]
    fresh = _engine(r, tables=(r.PM, RE2, r.CE))
    for c, b, a in zip(modes, before, after):
        assert _same(a, _lists(fresh, r.users, r.k, candidates=c)), "candidates %d after the table edit" % c
        assert not np.array_equal(a[1], b[1])
    head2 = mlp_head((r.C + 1) * r.E, r.H1, r.H2, rng, scale=4.0)
    eng.set_mlp_head(*head2)
    fresh.close()
    fresh = _engine(r, head=head2, tables=(r.PM, RE2, r.CE))
    for c, a in zip(modes, after):
        new = _lists(eng, r.users, r.k, candidates=c)
        assert _same(new, _lists(fresh, r.users, r.k, candidates=c)), "candidates %d after the new head" % c
        assert not np.array_equal(new[1], a[1])
    tc.compare_lists(*_lists(eng, r.users, r.k), tc.head_scores(r, r.users, tables=(r.PM, RE2, r.CE), head=head2), r.k, what="edited")
    eng.close()
    fresh.close()


# ---- 8. rank_candidates(head=True) ----------------------------------------------------------------------------------------------
def _segment_reference(items, lens, scores, k):
    """Per segment: (ids of oracle.rank_candidates on these scores, the collapsed table's scores in that order, sharp?)."""
    from oracle import m2d_oracle as oracle
    out = []
    for it, n, sc in zip(items, lens, scores):
        table = {}
        for d, v in zip(it[:n].tolist(), sc[:n].tolist()):
            table[d] = v
        ids = oracle.rank_candidates(it[:n].tolist(), sc[:n].tolist(), k)
        full = np.array(sorted(table.values(), reverse=True))[:k + 1]
        gap = full[:-1] - full[1:]
        out.append((ids, np.array([table[d] for d in ids]), bool(np.all(gap > 2 * np.maximum(tc.bound(full[:-1]), tc.bound(full[1:]))))))
    return out


def test_rank_candidates_under_the_head():
    r = tc.recipe("pc")
    rng = np.random.default_rng(8)
    nseg, L, k = 100, 51, 10
    users = rng.integers(0, r.U, nseg).astype(np.int32)
    items = np.stack([rng.choice(r.I, L, replace=False) for _ in range(nseg)]).astype(np.int32)
    items[5, 7] = items[5, 2]                                        # the dict collapse: first position, last score
    lens = np.full(nseg, L, np.int32)
    lens[[0, 11, 22, 33, 44]] = [1, 3, 10, 30, 50]
    head_sc = tc.head_scores(r, users, items)
    base_sc = tc.base_scores(r, users, items)
    ref_h, ref_b = _segment_reference(items, lens, head_sc, k), _segment_reference(items, lens, base_sc, k)
    assert np.mean([set(a[0]) != set(b[0]) for a, b in zip(ref_h, ref_b)]) >= tc.MIN_SHARE       # condition 1, per segment set
    assert np.mean([a[2] for a in ref_h]) >= tc.MIN_SHARE                                       # condition 2
    eng = _engine(r)
    ut, it, lt = _dev(users), _dev(items), _dev(lens)
    results = {}
    for head in (True, False):
        s, i, f = eng.rank_candidates(ut, it, k, lt, head=head)
        eng.check()
        results[head] = s, i, f = s.cpu().numpy(), i.cpu().numpy(), f.cpu().numpy()
        assert not f.any()
        for j, (ids, sc, sharp) in enumerate(ref_h if head else ref_b):
            n = len(ids)
            assert np.all(i[j, n:] == -1) and np.isnan(s[j, n:]).all(), "segment %d: padding" % j
            assert np.all(np.abs(s[j, :n] - sc) <= tc.bound(sc)), "segment %d (head %s): scores" % (j, head)        # comparison (a)
            if sharp:
                assert i[j, :n].tolist() == list(ids), "segment %d (head %s): ids" % (j, head)
    s0, i0, f0 = (t.cpu().numpy() for t in eng.rank_candidates(ut, it, k, lt))          # as it was called before
    assert np.array_equal(i0, results[False][1]) and np.array_equal(s0.view(np.int32), results[False][0].view(np.int32))
    assert not np.array_equal(results[True][1], results[False][1])
    eng.close()


# ---- 9. arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    import torch
    from foodrec_amd import _native
    lib = _native.lib()
    r = tc.recipe("i33")                                             # I = 33: I + 1 lies below 64
    k, nU = 10, len(r.users)
    ut = _dev(r.users)
    out_s = torch.empty((nU, 64), dtype=torch.float32, device="cuda")
    out_i = torch.empty((nU, 64), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(eng, users=ut.data_ptr(), n=nU, k=k, cand=0, s=out_s.data_ptr(), i=out_i.data_ptr()):
        return lib.m2d_topk_users_mlp(eng._h, users, n, k, cand, s, i, st)

    no_head = _engine(r, head=False)
    assert call(no_head) == _native.M2D_ERR_NOT_CONFIGURED == lib.m2d_score_pairs_mlp(no_head._h, ut.data_ptr(), ut.data_ptr(), nU, out_s.data_ptr(), st)
    assert "m2d_set_mlp_head" in _native.error_text(no_head._h)
    with pytest.raises(ValueError):
        no_head.topk_users_mlp(ut, k)
    with pytest.raises(ValueError):
        no_head.rank_candidates(ut[:4], _dev(np.zeros((4, 5), np.int32)), 3, head=True)
    no_head.close()
    no_masks = _engine(r, masks=False)
    assert call(no_masks) == _native.M2D_ERR_NOT_CONFIGURED
    assert "m2d_set_dish_categories" in _native.error_text(no_masks._h)
    no_masks.close()

    eng = _engine(r)
    for bad_k in (0, 65, r.I + 1):
        assert call(eng, k=bad_k) == _native.M2D_ERR_INVALID_ARG, bad_k
        assert call(eng, k=bad_k, cand=64) == _native.M2D_ERR_INVALID_ARG, bad_k
    for bad_c in (k - 1, 65, r.I + 1, -1):
        assert call(eng, cand=bad_c) == _native.M2D_ERR_INVALID_ARG, bad_c
    for kw in ({"users": None}, {"s": None}, {"i": None}):
        assert call(eng, **kw) == _native.M2D_ERR_INVALID_ARG, kw
    assert call(eng, n=-1) == _native.M2D_ERR_INVALID_ARG
    assert call(eng, n=0) == _native.M2D_OK == call(eng, n=0, users=None, s=None, i=None)
    assert call(eng, k=r.I, cand=r.I) == _native.M2D_OK and call(eng, k=r.I) == _native.M2D_OK           # the largest legal values
    eng.check()
    with pytest.raises(ValueError):
        eng.topk_users_mlp(ut, k, candidates=k - 1)
    with pytest.raises(TypeError):
        eng.topk_users_mlp(ut.to(torch.int64), k)
    s, i = eng.topk_users_mlp(ut[:0], k)
    assert tuple(s.shape) == (0, k)
    # duplicated users are allowed: the same rows
    dup = _lists(eng, np.concatenate([r.users[:3], r.users[:3]]), k)
    assert np.array_equal(dup[1][:3], dup[1][3:]) and np.array_equal(dup[0][:3].view(np.int32), dup[0][3:].view(np.int32))
    # the torch op is the method
    ts, ti = torch.ops.m2d.topk_users_mlp(eng.id, ut, k, 0)
    assert _same((ts.cpu().numpy(), ti.cpu().numpy()), _lists(eng, r.users, k))
    eng.close()


def test_model_topk_under_the_head():
    import torch
    import foodrec_amd
    r = tc.recipe("i33")
    args = types.SimpleNamespace(num_categories=r.C, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    model.set_mlp_head(*r.head)
    users = r.users.tolist()
    with pytest.raises(ValueError, match="head=True together with exclude"):
        model.topk(users, 5, exclude=[[1]] * len(users), head=True)
    s, i = model.topk(users, 10, head=True)
    tc.compare_lists(s, i, tc.reference("i33"), 10, what="Model.topk(head=True)")
    # the listed scores are predict_extended(head=True)'s for those pairs, within the bar (the launch shapes differ)
    pe = model.predict_extended(np.repeat(r.users, 10), i.reshape(-1), head=True).reshape(s.shape)
    assert np.all(np.abs(pe - s) <= tc.bound(s))
    s2, i2 = model.topk(users, 10, head=True, candidates=33)
    assert s2.shape == (len(users), 10)
    d0 = model.topk(users, 10)                                       # the defaults: the head is ignored, as before
    d1 = model.engine.topk_users(_dev(r.users), 10)
    assert np.array_equal(d0[1], d1[1].cpu().numpy()) and not np.array_equal(d0[1], i)
