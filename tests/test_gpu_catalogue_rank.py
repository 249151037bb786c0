"""Full-catalogue rank (m2d_catalogue_rank, ScoringEngine.catalogue_rank, evaluate_model_full) on the MI355X."""
import math

import numpy as np
import pytest
import torch

from helpers import COEFS
from seen_dish_cases import assert_rank_band, exact_tables as _exact_tables, host_rank as _host_rank, masks as _masks, \
    normal_tables as _normal_tables, oracle_scores as _oracle_scores

pytestmark = pytest.mark.gpu


def _engine(PM, RE, CE, cats, coef):
    import foodrec_amd
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=coef, device=torch.device("cuda", 0))
    eng.set_dish_categories(cats)
    return eng


def _rank(eng, users, items, exclude=None):
    r, s = eng.catalogue_rank(torch.as_tensor(np.asarray(users, np.int32)).cuda(), torch.as_tensor(np.asarray(items, np.int32)).cuda(),
                              exclude)
    eng.check()
    return r.cpu().numpy(), s.cpu().numpy()


# 1. agreement with retrieval, as exact integers ----------------------------------------------------------------------------------------
AGREE = [(32, 16, 33, 0.99), (32, 16, 1000, 0.99), (64, 16, 1000, 0.99), (128, 10, 1000, 0.99), (64, 16, 100003, 0.99),
         (128, 10, 100003, 0.99), (32, 16, 100003, 0.99)] + [(64, 16, 1000, c) for c in COEFS] + [(32, 16, 33, c) for c in COEFS] + \
        [(128, 10, 1000, c) for c in COEFS]


@pytest.mark.parametrize("E,k,I,coef", AGREE)
def test_rank_agrees_with_topk_lists(E, k, I, coef):
    rng = np.random.default_rng(E * 7 + I + int(coef * 100))
    U = 2048
    PM, RE, CE = _normal_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, _masks(rng, I), coef)
    users = torch.arange(U, dtype=torch.int32, device="cuda")
    for bf in (1, 0):
        eng.set_option("topk_bf16x3", bf)
        _, ids = eng.topk_users(users, k)
        eng.check()
        ids = ids.cpu().numpy()
        r, _ = _rank(eng, np.repeat(np.arange(U), k), ids.reshape(-1))
        want = np.tile(np.arange(k), U)
        bad = np.flatnonzero(r != want)
        assert bad.size == 0, (bf, bad[:8], r[bad[:8]], want[bad[:8]])


# 2. against the float64 oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [200, 64, 128])
def test_rank_within_oracle_band(E):
    rng = np.random.default_rng(E)
    U, I, coef = 64, 5000, 0.99
    PM, RE, CE = _normal_tables(rng, U, I, E)
    cats = _masks(rng, I)
    eng = _engine(PM, RE, CE, cats, coef)
    users = rng.integers(0, U, 48)
    items = rng.integers(0, I, 48)
    r, s = _rank(eng, users, items)
    for q in range(users.size):
        assert_rank_band(_oracle_scores(PM, RE, CE, cats, int(users[q]), coef), int(items[q]), r[q], s[q])


# 3. exact-arithmetic tables: exact ranks; the two protocols agree ----------------------------------------------------------------------
@pytest.mark.parametrize("E", [8, 32, 64])
def test_exact_tables_exact_ranks(E):
    rng = np.random.default_rng(100 + E)
    U, I = 16, 3000
    PM, RE, CE, cats = _exact_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, cats, 0.5)
    users = np.repeat(np.arange(U), 40)
    items = rng.integers(0, I, users.size)
    excl = [rng.choice(I, 30, replace=False).tolist() for _ in range(users.size)]
    r0, _ = _rank(eng, users, items)
    r1, _ = _rank(eng, users, items, excl)
    assert eng.get_option("rank_resolved") > 0
    for q in range(users.size):
        s64 = _oracle_scores(PM, RE, CE, cats, int(users[q]), 0.5)
        assert r0[q] == _host_rank(s64, int(items[q])), q
        assert r1[q] == _host_rank(s64, int(items[q]), excl[q]), q


def test_full_protocol_equals_sampled_protocol():
    import foodrec_amd
    rng = np.random.default_rng(7)
    U, I, E = 40, 600, 32
    PM, RE, CE, cats = _exact_tables(rng, U, I, E)
    import types
    args = types.SimpleNamespace(num_categories=4, num_users=U, embed_size=E, high_level_score_coefficient=0.5)
    model = foodrec_amd.Model(args, PM, RE, CE, None, device=torch.device("cuda", 0))
    d2c = {str(d): [[float(v)] for v in cats[d]] for d in range(I)}
    testRatings, testNegatives, train = {}, {}, {}
    for u in range(U):
        p = int(rng.integers(0, I - 60))
        negs = sorted(rng.choice(np.arange(p + 1, I), 50, replace=False).tolist())
        testRatings[str(u)] = [p]
        testNegatives[str(u)] = [0] * 50 + negs
        cand = set([p] + negs)
        train[str(u)] = [d for d in range(I) if d not in cand]
    for K in (1, 5, 10):
        h0, n0 = foodrec_amd.evaluate_model(None, model, testRatings, testNegatives, K, d2c)
        h1, n1 = foodrec_amd.evaluate_model_full(None, model, testRatings, train, K, d2c)
        assert h0 == h1 and n0 == n1, K


# 4. degenerate tables ---------------------------------------------------------------------------------------------------------------------
def _check_against_host(PM, RE, CE, cats, coef, users, items, need_resolved=False):
    eng = _engine(PM, RE, CE, cats, coef)
    r, _ = _rank(eng, users, items)
    if need_resolved:
        assert eng.get_option("rank_resolved") > 0
    for q in range(len(users)):
        s64 = _oracle_scores(PM, RE, CE, cats, int(users[q]), coef)
        assert r[q] == _host_rank(s64, int(items[q])), (q, r[q], _host_rank(s64, int(items[q])))
    return eng


def test_degenerate_zero_memory_and_coef_one():
    rng = np.random.default_rng(11)
    U, I, E = 8, 2000, 64
    PM, RE, CE, cats = _exact_tables(rng, U, I, E)
    PM[3] = 0.0
    users = np.repeat(np.arange(U), 16)
    items = rng.integers(0, I, users.size)
    _check_against_host(PM, RE, CE, cats, 0.5, users, items, need_resolved=True)
    _check_against_host(PM, RE, CE, cats, 1.0, users, items)


def test_degenerate_duplicates_empty_masks_and_tiny_catalogues():
    rng = np.random.default_rng(12)
    U, E = 6, 32
    for I in (1, 5, 31, 700):
        PM, RE, CE, cats = _exact_tables(rng, U, I, E)
        if I >= 5:
            RE[1::3] = RE[0]
            cats[1::3] = cats[0]
            cats[2::5] = 0.0                                  # empty masks: NaN scores
        users = np.repeat(np.arange(U), 4)
        items = rng.integers(0, I, users.size)
        if I >= 5:
            items[0] = 2                                      # an empty-mask held-out dish
        _check_against_host(PM, RE, CE, cats, 0.5, users, items)


# 5. exclusions -------------------------------------------------------------------------------------------------------------------------------
def test_exclusions_subtract_what_precedes():
    rng = np.random.default_rng(21)
    U, I, E = 64, 5000, 64
    PM, RE, CE = _normal_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, _masks(rng, I), 0.99)
    users = rng.integers(0, U, 64)
    items = rng.integers(0, I, 64)
    r0, _ = _rank(eng, users, items)
    excl = []
    for q in range(64):
        x = rng.integers(0, I, 500).tolist() + [int(items[q])]
        x = x + x[:20]                                        # unsorted, repeated, p itself inside
        excl.append(x)
    r1, _ = _rank(eng, users, items, excl)
    r_none, _ = _rank(eng, users, items, [[] for _ in range(64)])
    assert np.array_equal(r_none, r0)
    # rank_plain of each excluded x against the same user
    for q in range(64):
        xs = sorted(set(excl[q]) - {int(items[q])})
        rx, _ = _rank(eng, np.full(len(xs), users[q]), np.asarray(xs))
        before = int((rx < r0[q]).sum())
        assert r1[q] == r0[q] - before, q


def test_bad_ids_raise_and_engine_recovers():
    rng = np.random.default_rng(22)
    U, I, E = 16, 300, 32
    PM, RE, CE = _normal_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, _masks(rng, I), 0.99)
    for users, items, excl in (([0, U], [1, 2], None), ([0, 1], [1, I], None), ([0, 1], [1, 2], [[3, I + 5], []])):
        with pytest.raises(IndexError):
            _rank(eng, users, items, excl)
        r, _ = _rank(eng, [0, 1], [1, 2])
        assert r.shape == (2,)


# 6. refusals and plumbing ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    rng = np.random.default_rng(31)
    U, I, E = 8, 200, 32
    PM, RE, CE = _normal_tables(rng, U, I, E)
    import foodrec_amd
    q = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=torch.device("cuda", 0))
    with pytest.raises(ValueError):
        eng.catalogue_rank(*q)                                # no masks
    cats = _masks(rng, I)
    w = cats.copy()
    w[3, w[3].argmax()] = 0.5
    eng.set_dish_categories(w)
    with pytest.raises(ValueError, match="0/1"):
        eng.catalogue_rank(*q)
    eng.set_dish_categories(cats)
    eng.catalogue_rank(*q)
    eng.check()
    eng.re[5, 3] = float("inf")
    eng.tables_updated()
    with pytest.raises(ValueError, match="finite"):
        eng.catalogue_rank(*q)
    eng3 = foodrec_amd.ScoringEngine(PM[:, :4], RE, CE[:3], coef=0.99, device=torch.device("cuda", 0))
    eng3.set_dish_categories(cats[:, :3])
    with pytest.raises(ValueError, match="C = 4"):
        eng3.catalogue_rank(*q)
    engi = _engine(PM, RE, CE, cats, 0.99)
    engi.set_ingredients(rng.standard_normal((10, E)).astype(np.float32), np.arange(I + 1, dtype=np.int32), np.zeros(I, np.int32))
    with pytest.raises(ValueError, match="ingredient"):
        engi.catalogue_rank(*q)


def test_op_sharding_repeat_and_topk_diagnostics():
    rng = np.random.default_rng(41)
    U, I, E = 256, 4000, 64
    PM, RE, CE = _normal_tables(rng, U, I, E)
    cats = _masks(rng, I)
    eng = _engine(PM, RE, CE, cats, 0.99)
    users = torch.as_tensor(rng.integers(0, U, 300).astype(np.int32)).cuda()
    items = torch.as_tensor(rng.integers(0, I, 300).astype(np.int32)).cuda()
    eng.topk_users(torch.arange(U, dtype=torch.int32, device="cuda"), 10)
    names = ("topk_repaired", "topk_refined", "topk_tiles_scanned", "topk_tiles_full")
    before = [eng.get_option(n) for n in names]
    r1, s1 = eng.catalogue_rank(users, items)
    r2, s2 = eng.catalogue_rank(users, items)
    eng.check()
    assert torch.equal(r1, r2) and torch.equal(s1, s2)
    assert [eng.get_option(n) for n in names] == before
    ro, so = torch.ops.m2d.catalogue_rank(eng.id, users, items)
    assert torch.equal(ro, r1) and torch.equal(so, s1)
    # a shard holding users [128, 256) with global ids
    shard = _engine(PM[128:], RE, CE, cats, 0.99)
    shard.set_user_base(128)
    sel = users >= 128
    rs, _ = shard.catalogue_rank(users[sel].contiguous(), items[sel].contiguous())
    shard.check()
    assert torch.equal(rs, r1[sel])


# 7. reference sizes, end to end -----------------------------------------------------------------------------------------------------------------
def test_reference_split_end_to_end(tmp_path):
    import json
    import os
    import types

    import foodrec_amd
    from foodrec_amd import formats
    path = formats.write_synthetic_split(str(tmp_path), num_users=64657, num_dishes=4548, embed_size=32)
    ds = foodrec_amd.Dataset(path)
    PM, RE, CE = (np.load(os.path.join(str(tmp_path), n + ".npy")).astype(np.float32)
                  for n in ("Personal_Memory", "Recipe_Embedding", "Category_Embedding"))
    with open(os.path.join(str(tmp_path), "dish_to_category.json")) as f:
        d2c = json.load(f)
    U, E = PM.shape[0], PM.shape[2]
    args = types.SimpleNamespace(num_categories=4, num_users=U, embed_size=E, high_level_score_coefficient=0.99)
    model = foodrec_amd.Model(args, PM, RE, CE, None, device=torch.device("cuda", 0))
    rng = np.random.default_rng(5)
    keys = list(ds.testRatings.keys())
    sample = {keys[i]: ds.testRatings[keys[i]] for i in sorted(rng.choice(len(keys), 256, replace=False).tolist())}
    cats = model.set_dish_categories(d2c)
    checked = 0
    for K in (10, 100):
        hits, ndcgs = foodrec_amd.evaluate_model_full(None, model, sample, ds.trainMatrix, K, d2c)
        for i, u in enumerate(sample):
            s64 = _oracle_scores(PM, RE, CE, cats, int(u), 0.99)
            p = sample[u][0]
            keep = np.ones(s64.size, dtype=bool)
            keep[[x for x in ds.trainMatrix.get(u, []) if x != p]] = False
            keep[p] = False
            sp = s64[p]
            t = 1e-5 * max(1.0, abs(sp))
            lo = int(((s64 > sp + t) & keep).sum())
            hi = int(((s64 >= sp - t) & keep).sum())
            if (lo < K) == (hi < K):
                assert hits[i] == int(lo < K), (u, lo, hi, hits[i])
                checked += 1
            if lo == hi:
                assert ndcgs[i] == (math.log(2) / math.log(lo + 2) if lo < K else 0), (u, lo, ndcgs[i])
    assert checked > 400
