"""Full-catalogue top-k that leaves out each user's seen dishes (m2d_topk_users_excluding, ScoringEngine.topk_users_excluding,
Model.topk(exclude=...)) on the MI355X."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import COEFS
from seen_dish_cases import assert_list_band, exact_tables as _exact_tables, host_topk, masks as _masks, normal_tables as _normal_tables, \
    oracle_scores as _oracle_scores, per_query_csr as _per_query_csr

pytestmark = pytest.mark.gpu


def _engine(PM, RE, CE, cats, coef):
    import foodrec_amd
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=coef, device=torch.device("cuda", 0))
    eng.set_dish_categories(cats)
    return eng


def _users(U):
    return torch.arange(U, dtype=torch.int32, device="cuda")


def _topk_excl(eng, users, k, exclude):
    s, i = eng.topk_users_excluding(users, k, exclude)
    eng.check()
    return s.cpu().numpy(), i.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# 1. exact tables, exact lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("E", [8, 32, 64, 128, 200])
def test_exact_tables_exact_lists(E, k):
    rng = np.random.default_rng(300 + E)
    U, I = 16, 3000
    PM, RE, CE, cats = _exact_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, cats, 0.5)
    cycle = (0, 3, 6, 7, 16, 40)
    s64 = [_oracle_scores(PM, RE, CE, cats, u, 0.5) for u in range(U)]
    excl = []
    for u in range(U):
        own = host_topk(s64[u], 64, [])[:cycle[u % len(cycle)]].tolist()
        excl.append(own + rng.choice(I, 30, replace=False).tolist())
    _, ids = _topk_excl(eng, _users(U), k, excl)
    short = eng.get_option("topk_excl_short")
    for u in range(U):
        want = host_topk(s64[u], k, excl[u])
        assert ids[u].tolist() == want.tolist(), (u, ids[u], want)
    if k == 10 and E in (32, 64):
        assert 0 < short < U, short                           # both tiers ran


# 2. agreement with the rank call, as integers and bits ------------------------------------------------------------------------------
def _own_top_plus_random(eng, rng, U, I, jmod, nrand):
    """per user: its own unfiltered top (user index mod jmod) plus nrand random ids -> (offsets, ids) ascending, distinct"""
    from foodrec_amd.ops import exclusion_csr
    _, top = eng.topk_users(_users(U), min(jmod, I))
    eng.check()
    top = top.cpu().numpy()
    rnd = rng.integers(0, I, (U, nrand))
    lists = [top[u, :u % jmod].tolist() + rnd[u].tolist() for u in range(U)]
    return exclusion_csr(lists, U)


def _assert_rank_equals_position(eng, U, I, k, off, ids):
    dev = torch.device("cuda", 0)
    excl_dev = (torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev))
    sc, li = _topk_excl(eng, _users(U), k, excl_dev)
    assert li.min() >= 0                                      # enough dishes remain: no -1 entries
    qoff, qids = _per_query_csr(off, ids, k)
    r, s = eng.catalogue_rank(torch.from_numpy(np.repeat(np.arange(U, dtype=np.int32), k)).to(dev),
                              torch.from_numpy(li.reshape(-1).astype(np.int32)).to(dev),
                              (qoff, qids))
    eng.check()
    r, s = r.cpu().numpy().reshape(U, k), s.cpu().numpy().reshape(U, k)
    bad = np.argwhere(r != np.arange(k)[None, :])
    assert bad.size == 0, (bad[:8], r[bad[:8, 0]], li[bad[:8, 0]])
    assert np.array_equal(_bits(s), _bits(sc)), np.argwhere(_bits(s) != _bits(sc))[:8]
    srt = np.sort(li, axis=1)
    assert (np.diff(srt, axis=1) != 0).all()                 # no id repeats
    keys = np.repeat(np.arange(U, dtype=np.int64), np.diff(off)) * I + ids
    assert not np.isin(np.arange(U, dtype=np.int64)[:, None] * I + li, keys).any()      # no excluded id is listed
    return sc, li


SHAPES = [(32, 16), (64, 16), (64, 10), (128, 10), (200, 10)]


@pytest.mark.parametrize("coef", COEFS)
@pytest.mark.parametrize("I", [33, 1000, 100003])
@pytest.mark.parametrize("E,k", SHAPES)
def test_rank_of_listed_dish_is_its_position(E, k, I, coef):
    rng = np.random.default_rng(E * 11 + I + k + int(coef * 100))
    U = 2048
    PM, RE, CE = _normal_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, _masks(rng, I), coef)
    for bf in (1, 0):
        eng.set_option("topk_bf16x3", bf)
        off, ids = _own_top_plus_random(eng, rng, U, I, 5 if I == 33 else 20, 5 if I == 33 else 20)
        _assert_rank_equals_position(eng, U, I, k, off, ids)


# 3. both tiers, same answer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [1000, 100003])
@pytest.mark.parametrize("E,k", [(64, 16), (64, 10), (128, 10)])
def test_both_tiers_same_ids_and_bits(E, k, I):
    rng = np.random.default_rng(E * 13 + I + k)
    U = 2048
    PM, RE, CE = _normal_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, _masks(rng, I), 0.99)
    off, ids = _own_top_plus_random(eng, rng, U, I, 20, 20)
    dev = torch.device("cuda", 0)
    excl = (torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev))
    s0, i0 = _topk_excl(eng, _users(U), k, excl)
    short0 = eng.get_option("topk_excl_short")
    assert 0 < short0 < U                                     # users with j close to 20 are short, users with j = 0 are not
    eng.set_option("topk_excl_tier", 2)
    s2, i2 = _topk_excl(eng, _users(U), k, excl)
    assert eng.get_option("topk_excl_short") == U and eng.get_option("topk_excl_tiles_scanned") > 0
    assert np.array_equal(i0, i2), np.argwhere(i0 != i2)[:8]
    assert np.array_equal(_bits(s0), _bits(s2))
    # an unrelated call of 3 users in between: scratch of another size must not leak into the next call
    _topk_excl(eng, torch.tensor([5, 1, 9], dtype=torch.int32, device="cuda"), 3, [[1, 2], [], [7]])
    s2b, i2b = _topk_excl(eng, _users(U), k, excl)
    eng.set_option("topk_excl_tier", 0)
    _topk_excl(eng, torch.tensor([5, 1, 9], dtype=torch.int32, device="cuda"), 3, [[1, 2], [], [7]])
    s0b, i0b = _topk_excl(eng, _users(U), k, excl)
    assert eng.get_option("topk_excl_short") == short0
    for s, i in ((s2b, i2b), (s0b, i0b)):
        assert np.array_equal(i0, i) and np.array_equal(_bits(s0), _bits(s))


# 4. float64 band on normal tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 128, 200])
def test_lists_within_oracle_band(E):
    rng = np.random.default_rng(400 + E)
    U, I, coef, k = 64, 5000, 0.99, 10
    PM, RE, CE = _normal_tables(rng, U, I, E)
    cats = _masks(rng, I)
    eng = _engine(PM, RE, CE, cats, coef)
    off, ids = _own_top_plus_random(eng, rng, U, I, 20, 20)
    sc, li = _topk_excl(eng, _users(U), k, (off, ids))
    for u in range(U):
        assert_list_band(_oracle_scores(PM, RE, CE, cats, u, coef), ids[off[u]:off[u + 1]], li[u], sc[u])


# 5. with no exclusions it is topk_users ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,k", [(32, 16), (64, 16), (128, 10)])
def test_no_exclusions_is_topk_users(E, k):
    rng = np.random.default_rng(500 + E)
    U, I = 512, 20000
    PM, RE, CE = _normal_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, _masks(rng, I), 0.99)
    _, want = eng.topk_users(_users(U), k)
    eng.check()
    want = want.cpu().numpy()
    _, a = _topk_excl(eng, _users(U), k, None)
    _, b = _topk_excl(eng, _users(U), k, [[] for _ in range(U)])
    assert eng.get_option("topk_excl_short") == 0
    assert np.array_equal(a, want) and np.array_equal(b, want)
    eng.set_option("topk_excl_tier", 2)
    _, c = _topk_excl(eng, _users(U), k, None)
    assert np.array_equal(c, want)


# 6. edges -----------------------------------------------------------------------------------------------------------------------------------
def test_short_catalogue_pads_with_minus_one_and_nan():
    rng = np.random.default_rng(61)
    U, I, E, k = 8, 33, 32, 10
    PM, RE, CE, cats = _exact_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, cats, 0.5)
    excl = [rng.choice(I, 30, replace=False).tolist() for _ in range(U)]
    for tier in (0, 2):
        eng.set_option("topk_excl_tier", tier)
        sc, li = _topk_excl(eng, _users(U), k, excl)
        for u in range(U):
            want = host_topk(_oracle_scores(PM, RE, CE, cats, u, 0.5), k, excl[u])
            assert want.size == 3
            assert li[u].tolist() == want.tolist() + [-1] * 7, (tier, u, li[u])
            assert np.isnan(sc[u, 3:]).all() and not np.isnan(sc[u, :3]).any()


def test_empty_mask_dishes_come_last_in_id_order_and_can_be_excluded():
    rng = np.random.default_rng(62)
    U, I, E, k = 8, 40, 32, 16
    PM, RE, CE, cats = _exact_tables(rng, U, I, E)
    cats[2::3] = 0.0                                          # 13 empty masks: NaN scores
    eng = _engine(PM, RE, CE, cats, 0.5)
    masked = np.flatnonzero(cats.sum(1) > 0)
    excl = [masked[u:u + 20].tolist() + [2, 8 + 3 * u] for u in range(U)]         # 7 masked dishes remain; two empty ones excluded
    for tier in (0, 2):
        eng.set_option("topk_excl_tier", tier)
        sc, li = _topk_excl(eng, _users(U), k, excl)
        for u in range(U):
            want = host_topk(_oracle_scores(PM, RE, CE, cats, u, 0.5), k, excl[u])
            assert li[u].tolist() == want.tolist(), (tier, u, li[u], want)
            assert np.isnan(sc[u, 7:]).all() and not np.isnan(sc[u, :7]).any()


def test_coef_one_lowest_ids_not_excluded_win():
    rng = np.random.default_rng(63)
    U, I, E, k = 16, 3000, 64, 10
    PM, RE, CE, cats = _exact_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, cats, 1.0)
    s64 = [_oracle_scores(PM, RE, CE, cats, u, 1.0) for u in range(U)]
    excl = [host_topk(s64[u], 64, [])[:3 * (u % 6)].tolist() + rng.choice(I, 30, replace=False).tolist() for u in range(U)]
    for tier in (0, 2):
        eng.set_option("topk_excl_tier", tier)
        _, li = _topk_excl(eng, _users(U), k, excl)
        for u in range(U):
            assert li[u].tolist() == host_topk(s64[u], k, excl[u]).tolist(), (tier, u)


def test_whole_catalogue_excluded_no_users_and_user_base():
    rng = np.random.default_rng(64)
    U, I, E, k = 64, 500, 64, 10
    PM, RE, CE = _normal_tables(rng, U, I, E)
    cats = _masks(rng, I)
    eng = _engine(PM, RE, CE, cats, 0.99)
    excl = [list(range(I)) if u == 5 else [u, u + 1] for u in range(U)]
    sc, li = _topk_excl(eng, _users(U), k, excl)
    assert (li[5] == -1).all() and np.isnan(sc[5]).all()
    assert (li[np.arange(U) != 5] >= 0).all()
    s0, i0 = eng.topk_users_excluding(torch.zeros(0, dtype=torch.int32, device="cuda"), k, None)
    assert tuple(s0.shape) == (0, k) and tuple(i0.shape) == (0, k)
    # a shard holding users [32, 64) with global ids
    shard = _engine(PM[32:], RE, CE, cats, 0.99)
    shard.set_user_base(32)
    ss, si = _topk_excl(shard, torch.arange(32, 64, dtype=torch.int32, device="cuda"), k, excl[32:])
    assert np.array_equal(si, li[32:]) and np.array_equal(_bits(ss), _bits(sc[32:]))


# 7. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_reported_with_their_positions_and_the_engine_recovers():
    rng = np.random.default_rng(71)
    U, I, E = 16, 300, 32
    PM, RE, CE = _normal_tables(rng, U, I, E)
    eng = _engine(PM, RE, CE, _masks(rng, I), 0.99)
    dev = torch.device("cuda", 0)

    def works():
        _, li = _topk_excl(eng, [0, 1], 5, [[3], []])
        assert li.shape == (2, 5) and (li >= 0).all()

    for tier in (0, 2):
        eng.set_option("topk_excl_tier", tier)
        with pytest.raises(IndexError, match=r"item id %d at position 1 " % (I + 5)):
            _topk_excl(eng, [0, 1], 5, [[3, I + 5], []])
        works()
        raw = (torch.tensor([0, 3, 4], dtype=torch.int64, device=dev), torch.tensor([4, 9, 7, 2], dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match=r"not ascending: value 7 at position 2 "):
            _topk_excl(eng, [0, 1], 5, raw)
        works()
        with pytest.raises(IndexError, match=r"user id %d at position 1 " % U):
            _topk_excl(eng, [0, U], 5, [[3], []])
        works()
    with pytest.raises(ValueError):
        eng.topk_users_excluding([0], 17, None)
    with pytest.raises(ValueError):
        eng.topk_users_excluding([0], 0, None)
    tiny = _engine(PM, RE[:7], CE, _masks(rng, 7), 0.99)
    with pytest.raises(ValueError, match="min\\(16, I\\)"):
        tiny.topk_users_excluding([0], 8, None)               # k > I, as in m2d_topk_users


def test_refusals_name_the_condition():
    rng = np.random.default_rng(72)
    U, I, E = 8, 200, 32
    PM, RE, CE = _normal_tables(rng, U, I, E)
    import foodrec_amd
    q = (torch.zeros(1, dtype=torch.int32, device="cuda"), 5)
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=torch.device("cuda", 0))
    with pytest.raises(ValueError, match="m2d_set_dish_categories"):
        eng.topk_users_excluding(*q)                          # no masks
    cats = _masks(rng, I)
    w = cats.copy()
    w[3, w[3].argmax()] = 0.5
    eng.set_dish_categories(w)
    with pytest.raises(ValueError, match="0/1"):
        eng.topk_users_excluding(*q)
    eng.set_dish_categories(cats)
    eng.topk_users_excluding(*q)
    eng.check()
    engi = _engine(PM, RE, CE, cats, 0.99)
    engi.set_ingredients(rng.standard_normal((10, E)).astype(np.float32), np.arange(I + 1, dtype=np.int32), np.zeros(I, np.int32))
    with pytest.raises(ValueError, match="ingredient"):
        engi.topk_users_excluding(*q)
    engm = _engine(PM, RE, CE, cats, 0.99)
    K = 5 * E
    engm.set_mlp_head(rng.standard_normal((K, 256)).astype(np.float32), np.zeros(256, np.float32),
                      rng.standard_normal((256, 64)).astype(np.float32), np.zeros(64, np.float32), np.zeros(64, np.float32), 0.0)
    with pytest.raises(ValueError, match="MLP"):
        engm.topk_users_excluding(*q)


# 8. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_model_full_measures_the_lists_model_topk_serves(tmp_path):
    import foodrec_amd
    from foodrec_amd import formats
    path = formats.write_synthetic_split(str(tmp_path), num_users=300, num_dishes=60, embed_size=32, train_per_user=12)
    ds = foodrec_amd.Dataset(path)
    PM, RE, CE = (np.load(os.path.join(str(tmp_path), n + ".npy")).astype(np.float32)
                  for n in ("Personal_Memory", "Recipe_Embedding", "Category_Embedding"))
    with open(os.path.join(str(tmp_path), "dish_to_category.json")) as f:
        d2c = json.load(f)
    args = types.SimpleNamespace(num_categories=4, num_users=PM.shape[0], embed_size=PM.shape[2], high_level_score_coefficient=0.99)
    model = foodrec_amd.Model(args, PM, RE, CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(d2c)
    users = list(ds.testRatings.keys())
    n_hits = 0
    for K in (5, 16):
        hits, ndcgs = foodrec_amd.evaluate_model_full(None, model, ds.testRatings, ds.trainMatrix, K, d2c)
        seen = {u: [x for x in ds.trainMatrix.get(u, []) if x != ds.testRatings[u][0]] for u in users}
        _, ids = model.topk(users, K, exclude=seen)
        _, ids_list = model.topk(users, K, exclude=[seen[u] for u in users])
        assert np.array_equal(ids, ids_list)
        for i, u in enumerate(users):
            pos = np.flatnonzero(ids[i] == ds.testRatings[u][0])
            assert hits[i] == int(pos.size == 1), (K, u, hits[i], ids[i])
            assert ndcgs[i] == (math.log(2) / math.log(int(pos[0]) + 2) if pos.size else 0), (K, u)
        n_hits += sum(hits)
    assert n_hits > 20                                        # the catalogue is small enough for hits to occur
    s_plain, i_plain = model.topk(users, 10)
    assert i_plain.shape == (len(users), 10)


# 9. existing behaviour ---------------------------------------------------------------------------------------------------------------------
def test_topk_users_bits_and_the_diagnostics_rule():
    rng = np.random.default_rng(91)
    U, I, E = 256, 4000, 64
    PM, RE, CE = _normal_tables(rng, U, I, E)
    cats = _masks(rng, I)
    eng = _engine(PM, RE, CE, cats, 0.99)
    users = _users(U)
    s_before, i_before = eng.topk_users(users, 10)
    eng.check()
    q_u = torch.as_tensor(rng.integers(0, U, 300).astype(np.int32)).cuda()
    q_i = torch.as_tensor(rng.integers(0, I, 300).astype(np.int32)).cuda()
    eng.catalogue_rank(q_u, q_i)
    rank_names, topk_names = ("rank_tiles_scanned", "rank_resolved"), ("topk_repaired", "topk_refined", "topk_tiles_scanned", "topk_tiles_full")
    rank_before = [eng.get_option(n) for n in rank_names]
    topk_before = [eng.get_option(n) for n in topk_names]
    excl = [rng.integers(0, I, 20).tolist() for _ in range(U)]
    # the exact scan alone: neither family of diagnostics moves
    eng.set_option("topk_excl_tier", 2)
    _topk_excl(eng, users, 10, excl)
    assert [eng.get_option(n) for n in rank_names] == rank_before
    assert [eng.get_option(n) for n in topk_names] == topk_before
    # the first tier: the rank call's stay, the topk_* ones describe the internal retrieval of 16 entries (include/m2d.h)
    eng.set_option("topk_excl_tier", 0)
    _topk_excl(eng, users, 10, excl)
    assert [eng.get_option(n) for n in rank_names] == rank_before
    stable = ("topk_repaired", "topk_refined", "topk_tiles_full")       # (tiles stepped through depend on how the blocks' thresholds met)
    inner = [eng.get_option(n) for n in stable]
    eng.topk_users(users, 16)
    eng.check()
    assert [eng.get_option(n) for n in stable] == inner
    s_after, i_after = eng.topk_users(users, 10)
    eng.check()
    assert torch.equal(i_before, i_after) and torch.equal(s_before.view(torch.int32), s_after.view(torch.int32))
    so, io = torch.ops.m2d.topk_users_excluding(eng.id, users, 10)
    sd, idd = eng.topk_users_excluding(users, 10, None)
    eng.check()
    assert torch.equal(io, idd) and torch.equal(so.view(torch.int32), sd.view(torch.int32))
