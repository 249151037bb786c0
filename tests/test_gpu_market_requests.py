"""GPU tests of market requests (m2d_topk_markets): one (user, market) per request, filtered, scored and listed
in one call.  Ids and counts are compared as integers and scores as float32 words against the numpy restatement, into poisoned
[nQ, k] buffers with a guard row on either side: catalogue and bitmap edges, 51 different markets in one call, every share setting,
another category count, normal and non-finite tables against the pair kernel's words, errors, and the calls around it.  Requests,
restatement and stand-ins: tests/market_request_cases.py.

Slowest case: see README.md (status row "market requests")."""
import ctypes

import numpy as np
import pytest

import market_cases as mc
import market_request_cases as mq
import seen_dish_cases as sd
import slate_cases as sc

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN word no kernel writes; no dish id, no count


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(c, user_base=0, recipes=True):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(c.PM, c.RE, c.CE, coef=getattr(c, "coef", sd.COEF), user_base=user_base)
    eng.set_dish_categories(c.cats)
    if recipes:
        eng.set_recipes(c.off, c.ids, c.R)
    return eng


@pytest.fixture(scope="module")
def engines():
    """one engine per case, built on first use and shared by the tests of this file"""
    made = {}

    def get(key, case):
        if key not in made:
            made[key] = _engine(case)
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def _call(eng, users, markets, k, max_missing=0, counts=True, csr=None):
    """m2d_topk_markets through the C ABI into poisoned buffers: [nQ + 2, k] scores and ids and [nQ + 2] counts, the call's rows in the
    middle.  Returns (score words i32[nQ, k], ids i32[nQ, k], counts i32[nQ] or None) after checking that the guard rows were not
    written and every word of the call's rows was."""
    import torch
    from foodrec_amd import _native
    nQ = len(users)
    off, ids = csr if csr is not None else mq.csr(markets)
    u, o, m = _dev(np.asarray(users, np.int32)), _dev(np.asarray(off, np.int64)), _dev(np.asarray(ids, np.int32))
    s = torch.full((nQ + 2, k), POISON, dtype=torch.int32, device="cuda")
    i = torch.full((nQ + 2, k), POISON, dtype=torch.int32, device="cuda")
    n = torch.full((nQ + 2,), POISON, dtype=torch.int32, device="cuda")
    rc = _native.lib().m2d_topk_markets(eng._h, u.data_ptr(), nQ, o.data_ptr(), m.data_ptr() if m.numel() else None, m.numel(), k, max_missing,
                                        s[1:].data_ptr(), i[1:].data_ptr(), n[1:].data_ptr() if counts else None,
                                        torch.cuda.current_stream().cuda_stream)
    _native.raise_for(rc, eng._h)
    torch.cuda.synchronize()
    s, i, n = s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()
    for buf in (s, i, n):
        assert (buf[0] == POISON).all() and (buf[-1] == POISON).all(), "a guard row was written"
    assert (s[1:-1] != POISON).all() and (i[1:-1] != POISON).all(), "words of the call's rows were not written"
    assert (n[1:-1] != POISON).all() if counts else (n == POISON).all()
    return s[1:-1], i[1:-1], (n[1:-1] if counts else None)


def _assert_equal(got, want, what):
    """got: (words, ids, counts) of _call; want: (scores f64, ids, counts) of the restatement"""
    ws, wi, wn = want
    assert np.array_equal(got[2], wn), "%s: counts %s, restated %s" % (what, got[2], wn)
    assert np.array_equal(got[1], wi), "%s: ids of %d rows differ" % (what, int((got[1] != wi).any(1).sum()))
    s = got[0].view(np.float32)
    assert mq.same_answer((s, got[1], got[2]), want), "%s: score words differ" % what
    listed = np.minimum(wn, got[1].shape[1])
    for q in range(len(wn)):
        assert (got[1][q, listed[q]:] == -1).all() and np.isnan(s[q, listed[q]:]).all(), "%s: row %d past its count" % (what, q)


def _restated(eng, c, k, mm=0, what="", **kw):
    got = _call(eng, c.users, c.markets, k, mm, **kw)
    _assert_equal(got, mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, mm, k), "%s k = %d, max_missing = %d" % (what, k, mm))
    return got


# ---- 1. catalogue edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mq.CATALOGUES)
def test_catalogue_edges_equal_the_restatement(engines, n):
    c = mq.catalogue_case(n)
    eng = engines(("catalogue", n), c)
    for mm in c.tolerances:
        for k in mq.KS:
            _restated(eng, c, k, mm, "I = %d" % n)
            assert eng.last_kernel() == mq.TOPK_LDS


# ---- 2. bitmap edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", mc.BITMAP_ROWS)
def test_bitmap_edges_six_markets_in_one_call(engines, R):
    c = mq.bitmap_case(R)
    eng = engines(("bitmap", R), c)
    for k in (10, 64):
        _restated(eng, c, k, 0, "R = %d" % R)
        assert eng.last_kernel() == (mq.TOPK_LDS if R <= mq.LB else mq.TOPK_L2)
    _restated(eng, c, 10, 1, "R = %d, one missing" % R)


# ---- 3. 51 different markets in one call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", mq.COMPOSED_WIDTHS)
def test_fifty_one_markets_in_one_call(engines, E):
    c = mq.composed_case(E)
    eng = engines(("composed", E), c)
    rows = {}
    for k in mq.COMPOSED_KS:
        rows[k] = _restated(eng, c, k, 0, "E = %d" % E)
        assert np.array_equal(rows[k][2], c.counts)
        nocount = _call(eng, c.users, c.markets, k, 0, counts=False)              # out_counts null: the same lists
        assert np.array_equal(nocount[0], rows[k][0]) and np.array_equal(nocount[1], rows[k][1])
    # each row equals topk_market for that single request, ids and words
    for k in (7, 64):
        for q in range(len(c.users)):
            s, i, count = eng.topk_market(_dev(c.users[q:q + 1]), _dev(c.markets[q]), k)
            assert count == rows[k][2][q]
            nan = np.isnan(s.cpu().numpy()[0])
            assert np.array_equal(i.cpu().numpy()[0], rows[k][1][q]), "request %d, k = %d: ids differ from topk_market" % (q, k)
            assert np.array_equal(np.isnan(rows[k][0][q].view(np.float32)), nan)
            assert np.array_equal(sc.bits(np.where(nan, 0, s.cpu().numpy()[0])), sc.bits(np.where(nan, 0, rows[k][0][q].view(np.float32))))
    eng.check()
    # permuting the requests permutes the rows
    p = np.random.default_rng(E).permutation(len(c.users))
    got = _call(eng, c.users[p], [c.markets[j] for j in p], 10)
    assert all(np.array_equal(a, b[p]) for a, b in zip(got, rows[10]))
    # a request alone returns its row of the batch
    for q in (0, 3, 17, 50):
        one = _call(eng, c.users[q:q + 1], c.markets[q:q + 1], 10)
        assert all(np.array_equal(a[0], b[q]) for a, b in zip(one, rows[10]))
    eng.check()


# ---- 4. shares ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("773", "600", "hollow", "last wave"))
def test_every_share_setting_returns_the_one_share_words(engines, which):
    c = mq.share_case(which)
    eng = engines(("share", which), c)
    num_cu = eng.get_option("num_cu")
    try:
        for k in (10, 64):
            eng.set_option("market_shares", 1)
            one = _restated(eng, c, k, c.max_missing, which)
            assert eng.get_option("market_shares_used") == 1
            for S in mq.SHARES[1:]:
                eng.set_option("market_shares", S)
                for counts in (True, False):
                    got = _call(eng, c.users, c.markets, k, c.max_missing, counts=counts)
                    assert eng.get_option("market_shares_used") == mq.shares_used(S, len(c.users), num_cu, c.I) == len(mq.share_bounds(c.I, S))
                    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]), "%s, %d shares, k = %d" % (which, S, k)
                    assert not counts or np.array_equal(got[2], one[2])
    finally:
        eng.set_option("market_shares", 0)
    eng.check()


def test_the_share_rule_spreads_a_lone_request_and_gives_many_one_block_each(engines):
    c = mq.share_case("773")
    eng = engines(("share", "773"), c)
    num_cu = eng.get_option("num_cu")
    assert eng.get_option("market_shares") == 0
    one = _call(eng, c.users[:1], c.markets[:1], 10)
    assert eng.get_option("market_shares_used") == mq.shares_used(0, 1, num_cu, c.I) > 1
    nQ = 4 * num_cu + 1
    many = _call(eng, np.resize(c.users, nQ), [c.markets[0]] * nQ, 10)
    assert eng.get_option("market_shares_used") == 1
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[0], b[len(c.users)]) for a, b in zip(one, many))
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="market_shares"):
            eng.set_option("market_shares", bad)
    eng.check()


# ---- 5. another category count ---------------------------------------------------------------------------------------------------------
def test_three_categories_forty_columns(engines):
    c = mq.other_shape_case()
    eng = engines("other shape", c)
    for k in (10, 64):
        for mm in (0, 2):
            _restated(eng, c, k, mm, "C = 3, E = 40")
    eng.check()


# ---- 6. / 7. normal and non-finite tables: the pair kernel's words -------------------------------------------------------------------------
def _pair_words(eng, user, dishes):
    """score_pairs_bydish under variant = 9 for (user, d), d in dishes: the words the lists are defined by"""
    if len(dishes) == 0:
        return np.zeros(0, np.int32)
    eng.set_option("variant", 9)
    try:
        out = eng.score_pairs_bydish(_dev(np.full(len(dishes), user, np.int32)), _dev(np.asarray(dishes, np.int32)))
        return np.ascontiguousarray(out.cpu().numpy()).view(np.int32)
    finally:
        eng.set_option("variant", 0)


def _assert_rows_are_the_pair_kernels(eng, c, got, k, rows=None, what=""):
    for q in (range(len(c.users)) if rows is None else rows):
        cook = mc.restate(c.off, c.ids, c.R, c.markets[q], 0)[0]
        assert got[2][q] == len(cook)
        words = _pair_words(eng, c.users[q], cook)
        o = mq.key_order(words, cook)[:k]
        kk = len(o)
        assert np.array_equal(got[1][q, :kk], cook[o]) and (got[1][q, kk:] == -1).all(), "%s request %d: ids" % (what, q)
        mine, theirs = got[0][q, :kk], words[o]
        nan = np.isnan(theirs.view(np.float32))
        assert np.array_equal(np.isnan(mine.view(np.float32)), nan) and np.array_equal(mine[~nan], theirs[~nan]), "%s request %d: words" % (what, q)


@pytest.mark.parametrize("coef", mq.NORMAL_COEFS)
def test_normal_tables_list_the_pair_kernels_words(coef):
    from foodrec_amd import ScoringEngine
    from helpers import TOL
    c = mq.normal_case()
    eng = ScoringEngine(c.PM, c.RE, c.CE, coef=coef)
    eng.set_dish_categories(c.cats)
    eng.set_recipes(c.off, c.ids, c.R)
    k = 10
    got = _call(eng, c.users, c.markets, k)
    _assert_rows_are_the_pair_kernels(eng, c, got, k, what="coef %g" % coef)
    S = sd.score_matrix(c.PM, c.RE, c.CE, c.cats, coef, users=np.unique(c.users))
    row = {int(u): j for j, u in enumerate(np.unique(c.users))}
    worst = 0.0
    for q in range(len(c.users)):
        n = min(k, got[2][q])
        ref, s = S[row[int(c.users[q])]][got[1][q, :n]], got[0][q, :n].view(np.float32).astype(np.float64)
        assert np.array_equal(np.isnan(s), np.isnan(ref))
        ok = ~np.isnan(ref)
        worst = max(worst, float(np.abs(s[ok] - ref[ok]).max(initial=0.0)))
    print("coef %g: largest |listed - float64| = %.3e (bar %.0e)" % (coef, worst, TOL))
    assert worst <= TOL
    # skip_masked does not change the bits on finite tables
    eng.set_option("skip_masked", 0)
    again = _call(eng, c.users, c.markets, k)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    eng.check()
    eng.close()


def test_non_finite_tables_return_the_graphs_answer():
    """+inf in one low-level row of user u: a dish with that category scores +inf or -inf (the sign of its own row's element), a dish
    without it NaN (0 * inf, Model_Recommender.py:82) -- the whole order is visible in a market that leaves fewer than k dishes"""
    from foodrec_amd import ScoringEngine
    c = mq.normal_case()
    u, k = int(c.users[0]), 64
    m = next(m for m in range(c.R) if len(mc.restate(c.off, c.ids, c.R, np.arange(m), 0)[0]) >= 24)
    markets = [np.arange(m, dtype=np.int32)] + list(c.markets[1:])
    cook = mc.restate(c.off, c.ids, c.R, markets[0], 0)[0]
    assert 24 <= len(cook) <= k and (c.cats[cook, 1] == 1).any() and (c.cats[cook, 1] == 0).any()
    case = mq._case(users=c.users, markets=markets, off=c.off, ids=c.ids, R=c.R)
    clean = ScoringEngine(c.PM, c.RE, c.CE, coef=0.5)
    clean.set_dish_categories(c.cats)
    clean.set_recipes(c.off, c.ids, c.R)
    want = _call(clean, c.users, markets, k)
    clean.close()
    PM = c.PM.copy()
    PM[u, 2, 5] = np.inf                                     # the low-level row of category 1
    eng = ScoringEngine(PM, c.RE, c.CE, coef=0.5)
    eng.set_dish_categories(c.cats)
    eng.set_recipes(c.off, c.ids, c.R)
    got = _call(eng, c.users, markets, k)
    hit = [q for q in range(len(c.users)) if c.users[q] == u]
    _assert_rows_are_the_pair_kernels(eng, case, got, k, rows=hit, what="inf")
    n0 = got[2][0]
    s0 = got[0][0].view(np.float32)[:n0]
    kinds = np.where(np.isposinf(s0), 0, np.where(np.isneginf(s0), 2, np.where(np.isnan(s0), 3, 1)))
    assert np.all(np.diff(kinds) >= 0) and kinds[0] == 0 and kinds[-1] == 3 and (kinds == 2).any(), "+inf, finite, -inf, NaN: %s" % kinds
    for q in range(len(c.users)):
        if q not in hit:
            assert all(np.array_equal(a[q], b[q]) for a, b in zip(got, want)), "request %d changed with another user's inf" % q
    eng.check()
    eng.close()


# ---- 8. errors and refusals ------------------------------------------------------------------------------------------------------------
def test_errors_are_latched_and_the_other_rows_are_right(engines):
    c = mq.composed_case(64)
    eng = engines(("composed", 64), c)
    k = 10
    want = mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, k)
    off, ids = mq.csr(c.markets)
    # a bad market id: value and global index named, that id ignored, every row right
    for pos in (int(off[20]) + 3, len(ids) - 1):
        for bad_id in (-1, c.R):
            bad = ids.copy()
            bad[pos] = bad_id
            markets = [bad[off[q]:off[q + 1]] for q in range(len(c.users))]
            got = _call(eng, c.users, markets, k)
            with pytest.raises(IndexError, match=r"ingredient id %d at position %d " % (bad_id, pos)):
                eng.check()
            _assert_equal(got, mq.restate(c.S, c.users, c.off, c.ids, c.R, markets, 0, k), "bad market id")
            eng.check()                                           # the latch is clear again
    # a bad user id: that row empty, its count right, the other rows right
    for q, bad_user in ((0, -1), (30, c.U), (52, 2 ** 31 - 1)):
        users = c.users.copy()
        users[q] = bad_user
        got = _call(eng, users, c.markets, k)
        with pytest.raises(IndexError, match=r"user id %d at position %d " % (bad_user, q)):
            eng.check()
        _assert_equal(got, mq.restate(c.S, users, c.off, c.ids, c.R, c.markets, 0, k), "bad user id")
        assert (got[1][q] == -1).all() and got[2][q] == c.counts[q]
    # decreasing offsets, offsets outside [0, nnzM]: latched with the request, clamped before anything is read
    for q, value in ((10, int(off[10]) - 5), (25, len(ids) + 1000), (40, -7)):
        o = off.copy()
        o[q + 1] = value
        got = _call(eng, c.users, c.markets, k, csr=(o, ids))
        # (the request after a bad end offset starts outside as well: whichever of the two is latched first)
        with pytest.raises(ValueError, match=r"at position (%d|%d) .*m2d_topk_markets" % (q, q + 1)):
            eng.check()
        lo = np.clip(o[:-1], 0, len(ids))
        hi = np.clip(np.maximum(o[1:], lo), 0, len(ids))
        markets = [ids[lo[j]:hi[j]] for j in range(len(c.users))]
        _assert_equal(got, mq.restate(c.S, c.users, c.off, c.ids, c.R, markets, 0, k), "offsets, request %d" % q)
    _assert_equal(_call(eng, c.users, c.markets, k), want, "after the errors")
    eng.check()


def test_bad_arguments_and_refusals():
    import torch
    from foodrec_amd import _native
    from helpers import mlp_head
    c = mq.composed_case(64)
    eng = _engine(c, recipes=False)
    lib = _native.lib()
    users, markets = _dev(c.users), [m for m in c.markets]
    with pytest.raises(ValueError, match="m2d_set_recipes first"):
        eng.topk_markets(users, markets, 10)
    eng.set_recipes(c.off, c.ids, c.R)
    for k in (0, 65):
        with pytest.raises(ValueError, match="1 <= k <= 64"):
            eng.topk_markets(users, markets, k)
    with pytest.raises(ValueError, match="max_missing >= 0"):
        eng.topk_markets(users, markets, 10, max_missing=-1)
    with pytest.raises(ValueError, match="54 markets for 53 users"):
        eng.topk_markets(users, markets + [[1]], 10)
    s, i, n = eng.topk_markets(users[:0], [], 10, return_counts=True)           # nQ = 0: nothing launched
    assert tuple(s.shape) == (0, 10) and tuple(i.shape) == (0, 10) and tuple(n.shape) == (0,)
    off, ids = (_dev(a) for a in mq.csr(c.markets))
    out_s, out_i = torch.empty((53, 10), device="cuda"), torch.empty((53, 10), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = lambda **kw: [kw.get("h", eng._h), kw.get("users", users.data_ptr()), kw.get("nQ", 53), kw.get("off", off.data_ptr()),
                         kw.get("ids", ids.data_ptr()), kw.get("nnz", ids.numel()), 10, 0, kw.get("s", out_s.data_ptr()), out_i.data_ptr(), None, st]
    for kw in ({"nQ": -1}, {"nnz": -1}, {"users": None}, {"off": None}, {"ids": None}, {"s": None}):
        assert lib.m2d_topk_markets(*args(**kw)) == _native.M2D_ERR_INVALID_ARG, kw
    assert lib.m2d_topk_markets(*args(nQ=0, users=None)) == _native.M2D_OK
    assert lib.m2d_topk_markets(*args(ids=None, nnz=0, off=_dev(np.zeros(54, np.int64)).data_ptr())) == _native.M2D_OK
    eng.check()
    assert (out_i.cpu().numpy() == -1).all()                                     # every market empty
    rng = np.random.default_rng(3)
    eng.set_ingredients((rng.integers(-4, 5, (7, 64)) / 4).astype(np.float32), np.arange(c.I + 1, dtype=np.int32), rng.integers(0, 7, c.I).astype(np.int32))
    with pytest.raises(ValueError, match="m2d_topk_markets: the ingredient table is set"):
        eng.topk_markets(users, markets, 10)
    eng.clear_ingredients()
    eng.set_mlp_head(*mlp_head(320, 256, 64, rng))
    with pytest.raises(ValueError, match="m2d_topk_markets: the MLP head is set"):
        eng.topk_markets(users, markets, 10)
    eng.clear_mlp_head()
    _restated(eng, c, 10, 0, "after the refusals")                               # the engine answers correctly afterwards
    eng.close()
    from foodrec_amd import ScoringEngine
    bare = ScoringEngine(c.PM, c.RE, c.CE, coef=c.coef)
    bare.set_recipes(c.off, c.ids, c.R)
    with pytest.raises(ValueError, match="m2d_set_dish_categories first"):
        bare.topk_markets(users, markets, 10)
    bare.close()


def test_a_user_base_shard():
    c = mq.composed_case(64)
    eng = _engine(c, user_base=1000)
    got = _call(eng, c.users + 1000, c.markets, 10)
    _assert_equal(got, mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, 10), "user_base 1000")
    got = _call(eng, c.users, c.markets, 10)                                      # ids below the shard: every row empty, counts kept
    with pytest.raises(IndexError, match="user id"):
        eng.check()
    assert (got[1] == -1).all() and np.array_equal(got[2], c.counts)
    eng.close()


# ---- 9. around it ------------------------------------------------------------------------------------------------------------------------
def test_repeatable_and_follows_new_recipes():
    c, b = mq.composed_case(64), mc.extreme_recipe("hollow")
    eng = _engine(c)
    first = _restated(eng, c, 10, 0, "first")
    for _ in range(2):
        assert all(np.array_equal(x, y) for x, y in zip(first, _call(eng, c.users, c.markets, 10)))
    off = np.concatenate([b.off[:c.I + 1], np.full(max(0, c.I - b.I), b.off[-1], np.int32)])[:c.I + 1]
    eng.set_recipes(off, b.ids[:off[-1]], b.R)
    markets = [np.arange(j % (b.R + 1), dtype=np.int32) for j in range(len(c.users))]
    second = _call(eng, c.users, markets, 10)
    _assert_equal(second, mq.restate(c.S, c.users, off, b.ids[:off[-1]], b.R, markets, 0, 10), "replaced recipes")
    assert not np.array_equal(first[1], second[1])
    eng.check()
    eng.close()


def test_independent_of_the_shared_market_calls_in_between(engines):
    c = mq.composed_case(64)
    eng = engines(("composed", 64), c)
    before = _call(eng, c.users, c.markets, 10, 1)
    shared = mc.composed_recipe().market
    cook = eng.cookable_dishes(_dev(shared), 0).cpu().numpy()
    s, i, count = eng.topk_market(_dev(c.users), _dev(shared), 10)
    after = _call(eng, c.users, c.markets, 10, 1)
    assert all(np.array_equal(x, y) for x, y in zip(before, after)), "topk_markets changed after cookable_dishes / topk_market"
    assert np.array_equal(eng.cookable_dishes(_dev(shared), 0).cpu().numpy(), cook) and np.array_equal(cook, mc.composed_recipe().cookable)
    s2, i2, count2 = eng.topk_market(_dev(c.users), _dev(shared), 10)
    assert count2 == count and np.array_equal(i2.cpu().numpy(), i.cpu().numpy()) and np.array_equal(
        s2.cpu().numpy().view(np.int32), s.cpu().numpy().view(np.int32)), "topk_market changed after topk_markets"
    eng.check()


def test_lists_follow_the_engines_writers():
    """topk_markets after write_memory and after a train_step equals a fresh engine built from the written tables, ids and score words"""
    import torch
    from foodrec_amd import ScoringEngine
    c = mq.normal_case()
    rng = np.random.default_rng(6)
    t = lambda a: torch.as_tensor(a, device="cuda")

    def engine(PM, RE, CE):
        e = ScoringEngine(PM, RE, CE, coef=0.5)
        e.set_dish_categories(c.cats)
        e.set_recipes(c.off, c.ids, c.R)
        return e

    def lists(e):
        out = _call(e, c.users, c.markets, 10)
        e.check()
        return out

    def fresh():
        f = engine(eng.pm.cpu().numpy(), eng.re.cpu().numpy(), eng.ce.cpu().numpy())
        out = lists(f)
        f.close()
        return out

    eng = engine(c.PM.copy(), c.RE.copy(), c.CE.copy())
    before = lists(eng)
    B, L = 600, 7
    wu = (np.arange(B) % c.U).astype(np.int32)
    masked = np.flatnonzero(c.cats.sum(1) > 0)
    wi = rng.choice(masked, B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, c.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(c.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    after_write, f = lists(eng), fresh()
    assert (after_write[0] != before[0]).mean() > 0.5, "write_memory changed nothing"
    assert all(np.array_equal(x, y_) for x, y_ in zip(after_write, f)), "after write_memory"
    eng.train_begin("sgd", 200.0)
    tu = (rng.permutation(256) % c.U).astype(np.int32)
    ti = rng.choice(masked, 256).astype(np.int32)
    eng.train_step(t(tu), t(ti), t(c.cats[ti]), t(rng.integers(0, 2, 256).astype(np.float32))); eng.check()
    after_step, f = lists(eng), fresh()
    assert (after_step[0] != after_write[0]).mean() > 0.5, "train_step changed nothing"
    assert all(np.array_equal(x, y_) for x, y_ in zip(after_step, f)), "after train_step"
    eng.train_end()
    eng.close()


def test_python_surface_returns_the_engines_words(engines):
    import types

    import torch

    import foodrec_amd
    c = mq.composed_case(64)
    eng = engines(("composed", 64), c)
    want = _call(eng, c.users, c.markets, 10, 1)
    raw = lambda x: np.ascontiguousarray(x.cpu().numpy()).view(np.int32)
    off, ids = mq.csr(c.markets)
    for markets in ([m.tolist() for m in c.markets], (off, ids), (_dev(off), _dev(ids))):
        s, i, n = eng.topk_markets(_dev(c.users), markets, 10, max_missing=1, return_counts=True)
        assert s.dtype == torch.float32 and i.dtype == torch.int32 and n.dtype == torch.int32
        assert all(np.array_equal(raw(x), y) for x, y in zip((s, i, n), want))
    pair = eng.topk_markets(c.users, c.markets, 10, max_missing=1)
    assert len(pair) == 2 and np.array_equal(raw(pair[1]), want[1])
    s, i, n = torch.ops.m2d.topk_markets(eng.id, _dev(c.users), _dev(off), _dev(ids), 10, 1)
    assert all(np.array_equal(raw(x), y) for x, y in zip((s, i, n), want))
    eng.check()
    args = types.SimpleNamespace(num_categories=4, num_users=c.U, embed_size=c.E, high_level_score_coefficient=c.coef)
    model = foodrec_amd.Model(args, c.PM, c.RE, c.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(c.cats)
    model.set_recipes((c.off, c.ids), c.R)
    plain = model.topk([4, 0, 31], 10)
    s, i, n = model.topk_markets([str(u) for u in c.users], [[str(v) for v in m] for m in c.markets], 10, max_missing=1)
    assert s.dtype == np.float32 and i.dtype == np.int32 and n.dtype == np.int32
    assert np.array_equal(s.view(np.int32), want[0]) and np.array_equal(i, want[1]) and np.array_equal(n, want[2])
    with pytest.raises(ValueError, match="2 markets for 3 users"):
        model.topk_markets([1, 2, 3], [[1], [2]])
    with pytest.raises(IndexError, match=r"ingredient id %d at position 1 " % c.R):
        model.topk_markets([1], [[0, c.R]])
    again = model.topk([4, 0, 31], 10)
    assert np.array_equal(again[1], plain[1]) and np.array_equal(again[0].view(np.int32), plain[0].view(np.int32))
