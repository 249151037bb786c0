"""GPU tests of the excluding market requests (m2d_topk_markets_excluding): m2d_topk_markets that leaves out
each request's excluded dishes and names the list entries a listed dish's market lacks.  Ids, counts and missing entries are compared as
integers and scores as float32 words against the numpy restatement, into poisoned buffers with a guard row on either side.  Requests,
restatement and stand-ins: tests/market_excluding_cases.py (on tests/market_request_cases.py).

Slowest case: see README.md (status row "market requests, excluding")."""
import re

import numpy as np
import pytest

import market_cases as mc
import market_excluding_cases as mx
import market_request_cases as mq
import seen_dish_cases as sd

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN word no kernel writes; no dish id, no count, no ingredient id


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(c, user_base=0, coef=None):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(c.PM, c.RE, c.CE, coef=coef if coef is not None else getattr(c, "coef", sd.COEF), user_base=user_base)
    eng.set_dish_categories(c.cats)
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


def _old(eng, users, markets, k, max_missing=0):
    """m2d_topk_markets into poisoned buffers: (score words, ids, counts)"""
    import torch
    from foodrec_amd import _native
    nQ = len(users)
    off, ids = mq.csr(markets)
    u, o, m = _dev(np.asarray(users, np.int32)), _dev(off), _dev(ids)
    s = torch.full((nQ, k), POISON, dtype=torch.int32, device="cuda")
    i = torch.full((nQ, k), POISON, dtype=torch.int32, device="cuda")
    n = torch.full((nQ,), POISON, dtype=torch.int32, device="cuda")
    rc = _native.lib().m2d_topk_markets(eng._h, u.data_ptr(), nQ, o.data_ptr(), m.data_ptr() if m.numel() else None, m.numel(), k, max_missing,
                                        s.data_ptr(), i.data_ptr(), n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _native.raise_for(rc, eng._h)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()


def _call(eng, users, markets, excl, k, max_missing=0, counts=True, missing=False, xcsr=None, repeats=False):
    """m2d_topk_markets_excluding through the C ABI into poisoned buffers with a guard row on either side: [nQ + 2, k] scores and ids,
    [nQ + 2] counts, [nQ + 2, k, max_missing] missing entries.  `excl`: None (excl_off = NULL) or nQ id sequences, made ascending
    (`repeats`: with repeated ids); `xcsr`: the (offsets, ids) arrays as they are.  Returns (score words, ids, counts or None, missing or
    None) after checking that no guard row was written and every word of the call's rows was."""
    import torch
    from foodrec_amd import _native
    nQ = len(users)
    off, ids = mq.csr(markets)
    u, o, m = _dev(np.asarray(users, np.int32)), _dev(np.asarray(off, np.int64)), _dev(np.asarray(ids, np.int32))
    xo = xi = None
    if xcsr is not None or excl is not None:
        a, b = xcsr if xcsr is not None else mx.csr(excl, repeats)
        xo, xi = _dev(np.asarray(a, np.int64)), _dev(np.asarray(b, np.int32))
    mm = max(max_missing, 1)
    s = torch.full((nQ + 2, k), POISON, dtype=torch.int32, device="cuda")
    i = torch.full((nQ + 2, k), POISON, dtype=torch.int32, device="cuda")
    n = torch.full((nQ + 2,), POISON, dtype=torch.int32, device="cuda")
    w = torch.full((nQ + 2, k, mm), POISON, dtype=torch.int32, device="cuda")
    rc = _native.lib().m2d_topk_markets_excluding(
        eng._h, u.data_ptr(), nQ, o.data_ptr(), m.data_ptr() if m.numel() else None, m.numel(),
        xo.data_ptr() if xo is not None else None, xi.data_ptr() if xi is not None and xi.numel() else None, k, max_missing,
        s[1:].data_ptr(), i[1:].data_ptr(), n[1:].data_ptr() if counts else None, w[1:].data_ptr() if missing else None,
        torch.cuda.current_stream().cuda_stream)
    _native.raise_for(rc, eng._h)
    torch.cuda.synchronize()
    s, i, n, w = s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy(), w.cpu().numpy()
    for buf in (s, i, n, w):
        assert (buf[0] == POISON).all() and (buf[-1] == POISON).all(), "a guard row was written"
    assert (s[1:-1] != POISON).all() and (i[1:-1] != POISON).all(), "words of the call's rows were not written"
    assert (n[1:-1] != POISON).all() if counts else (n == POISON).all()
    written = missing and max_missing > 0
    assert (w[1:-1] != POISON).all() if written else (w == POISON).all(), "out_missing: %s" % ("words not written" if written else "written")
    return s[1:-1], i[1:-1], (n[1:-1] if counts else None), (w[1:-1] if written else None)


def _assert_equal(got, want, what):
    """got: _call's tuple; want: (scores f64, ids, counts) of the restatement"""
    ws, wi, wn = want
    assert np.array_equal(got[2], wn), "%s: counts %s, restated %s" % (what, got[2], wn)
    assert np.array_equal(got[1], wi), "%s: ids of %d rows differ" % (what, int((got[1] != wi).any(1).sum()))
    s = got[0].view(np.float32)
    assert mq.same_answer((s, got[1], got[2]), want), "%s: score words differ" % what
    listed = np.minimum(wn, got[1].shape[1])
    for q in range(len(wn)):
        assert (got[1][q, listed[q]:] == -1).all() and np.isnan(s[q, listed[q]:]).all(), "%s: row %d past its count" % (what, q)


def _restated(eng, c, excl, k, mm=0, what="", **kw):
    got = _call(eng, c.users, c.markets, excl, k, mm, **kw)
    _assert_equal(got, mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, excl, mm, k), "%s k = %d, max_missing = %d" % (what, k, mm))
    if got[3] is not None:
        assert mx.same_missing(got[3], mx.restate_missing(c.off, c.ids, c.R, c.markets, got[1], mm)), "%s k = %d, max_missing = %d: missing entries" % (what, k, mm)
    return got


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. no exclusions, no missing entries: m2d_topk_markets' words ------------------------------------------------------------------------
@pytest.mark.parametrize("n", mq.CATALOGUES)
def test_null_exclusions_and_null_missing_return_topk_markets_words(engines, n):
    c = mq.catalogue_case(n)
    eng = engines(("catalogue", n), c)
    for k in mq.KS:
        for mm in (0, 2):
            old = _old(eng, c.users, c.markets, k, mm)
            kernel = eng.last_kernel()
            new = _call(eng, c.users, c.markets, None, k, mm)
            assert eng.last_kernel() == kernel == mq.TOPK_LDS                       # the same instantiation
            assert _same(new[:3], old), "I = %d, k = %d, max_missing = %d" % (n, k, mm)
            # an empty list for every request: the exclusion form, the same words
            empty = _call(eng, c.users, c.markets, [()] * len(c.users), k, mm)
            assert eng.last_kernel() == "m2d_markets_topk_excl_lds" and _same(empty[:3], old)
    eng.check()


# ---- 2. exclusion edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mq.CATALOGUES)
def test_exclusion_kinds_on_the_catalogue_cases(engines, n):
    c = mq.catalogue_case(n)
    eng = engines(("catalogue", n), c)
    for kind in mx.KINDS:
        excl = mx.exclusions(n, kind)
        for k in mq.KS:
            for mm in (0, 2):
                got = _restated(eng, c, excl, k, mm, "I = %d, %s" % (n, kind), repeats=(kind == "mixed"))
                if kind == "all":
                    assert (got[2] == 0).all() and (got[1] == -1).all() and np.isnan(got[0].view(np.float32)).all()
        nocount = _call(eng, c.users, c.markets, excl, 10, 0, counts=False)          # out_counts null: the same lists
        assert _same(nocount[:2], _call(eng, c.users, c.markets, excl, 10, 0)[:2])
    eng.check()


@pytest.mark.parametrize("n", mq.CATALOGUES)
def test_excluded_ids_at_the_group_and_block_edges(engines, n):
    c = mx.edge_case(n)
    eng = engines(("edge", n), c)
    try:
        for S in (1, 4):
            eng.set_option("market_shares", S)
            for k in mq.KS:
                _restated(eng, c, c.excl, k, 0, "edge ids, I = %d, %d shares" % (n, S), repeats=(S == 4))
            _restated(eng, c, c.excl, 10, 1, "edge ids, I = %d, %d shares" % (n, S), missing=True)
    finally:
        eng.set_option("market_shares", 0)
    eng.check()


def test_exclusions_on_both_sides_of_every_share_boundary(engines):
    c, excl = mq.share_case("773"), mx.share_exclusions()
    eng = engines(("share", "773"), c)
    try:
        for k in (10, 64):
            eng.set_option("market_shares", 1)
            one = _restated(eng, c, excl, k, 0, "one share")
            assert eng.get_option("market_shares_used") == 1
            for S in mq.SHARES[1:]:
                eng.set_option("market_shares", S)
                for counts in (True, False):
                    got = _call(eng, c.users, c.markets, excl, k, 0, counts=counts)
                    assert eng.get_option("market_shares_used") == len(mq.share_bounds(c.I, S))
                    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]), "%d shares, k = %d" % (S, k)
                    assert not counts or np.array_equal(got[2], one[2])
    finally:
        eng.set_option("market_shares", 0)
    eng.check()


@pytest.mark.parametrize("E", mq.COMPOSED_WIDTHS)
def test_fifty_one_requests_each_with_its_own_list(engines, E):
    c, excl = mq.composed_case(E), mx.composed_exclusions(E)
    eng = engines(("composed", E), c)
    rows = {k: _restated(eng, c, excl, k, 0, "E = %d" % E) for k in (10, 64)}
    assert eng.last_kernel() == "m2d_markets_topk_excl_lds"
    if E == 64:                                              # every row equals the one-request call (which spreads over many shares)
        for q in range(len(c.users)):
            one = _call(eng, c.users[q:q + 1], c.markets[q:q + 1], excl[q:q + 1], 10)
            assert all(np.array_equal(a[0], b[q]) for a, b in zip(one[:3], rows[10][:3])), "request %d alone" % q
        assert eng.get_option("market_shares_used") > 1
        p = np.random.default_rng(E).permutation(len(c.users))                      # permuting the requests permutes the rows
        got = _call(eng, c.users[p], [c.markets[j] for j in p], [excl[j] for j in p], 10)
        assert all(np.array_equal(a, b[p]) for a, b in zip(got[:3], rows[10][:3]))
    eng.check()


def test_a_history_longer_than_the_workarounds_slack(engines):
    """every request has had its 59 best dishes: topk_markets at k = 64 filtered on the host can list 5, the call lists 10"""
    c, excl, k = mq.composed_case(64), mx.history_exclusions(), mx.HISTORY_K
    eng = engines(("composed", 64), c)
    got = _restated(eng, c, excl, k, 0, "history")
    old = _old(eng, c.users, c.markets, 64)
    wrong = 0
    for q in range(len(c.users)):
        keep = [d for d in old[1][q] if d >= 0 and d not in set(excl[q].tolist())][:k]
        wrong += list(got[1][q][got[1][q] >= 0]) != keep
    assert wrong >= 30 and (got[1][50] >= 0).all()
    eng.check()


# ---- 3. missing entries --------------------------------------------------------------------------------------------------------------------
def _assert_missing_counts(eng, c, got, mm, what):
    """the non-negative entries of out_missing[q, j] number m2d_cookable_dishes' out_missing of that dish for the same market"""
    for q in range(len(c.users)):
        ids, miss = eng.cookable_dishes(_dev(np.asarray(c.markets[q], np.int32)), mm, return_missing=True)
        miss = miss.cpu().numpy().reshape(-1)
        for j, d in enumerate(got[1][q]):
            assert (got[3][q, j] >= 0).sum() == (miss[d] if d >= 0 else 0), "%s: request %d, dish %d" % (what, q, d)


def test_missing_entries_of_the_fixed_layout(engines):
    c = mx.missing_case()
    eng = engines("missing", c)
    try:
        for S in (1, 2):                                     # 70 dishes: one 256-dish block, so one share whatever is asked
            eng.set_option("market_shares", S)
            for mm in mx.TOLERANCES:
                for k in mq.KS:
                    for excl in (None, c.excl):
                        got = _restated(eng, c, excl, k, mm, "layout, %d shares" % S, missing=True)
                    nomiss = _call(eng, c.users, c.markets, c.excl, k, mm)           # out_missing null: the same lists
                    assert _same(nomiss[:3], got[:3])
                _assert_missing_counts(eng, c, got, mm, "layout, max_missing = %d" % mm)
    finally:
        eng.set_option("market_shares", 0)
    got = _call(eng, c.users, c.markets, c.excl, 64, 3, missing=True)
    row = {int(d): got[3][0, j].tolist() for j, d in enumerate(got[1][0]) if d >= 0}
    assert row[4] == [11, 1, 3] and row[5] == [13, 5, 1] and row[6] == [21, 21, -1] and row[7] == [15, 15, -1] and row[8] == [-1, -1, -1]
    assert 0 < got[2][4] < 64 and (got[3][4][got[1][4] < 0] == -1).all()            # a row shorter than k
    _call(eng, c.users, c.markets, c.excl, 10, 0, missing=True)                     # max_missing = 0: the pointer is ignored
    eng.check()


def test_missing_entries_with_more_than_one_share(engines):
    """catalogue_case(773): lists of 63 / 64 / 65 / 193 entries whose last entry is absent, the rows merged from 1 - 4 shares.  Every
    request has had all dishes but every twelfth and the four long lists, so fewer than 64 are left and all of them are listed."""
    c = mq.catalogue_case(773)
    eng = engines(("catalogue", 773), c)
    long_lists = [2 * mq.DW + j for j in range(4)]
    excl = [np.asarray([d for d in range(c.I) if d % 12 and d not in long_lists])] * len(c.users)
    try:
        eng.set_option("market_shares", 1)
        one = {mm: _restated(eng, c, excl, 64, mm, "one share", missing=True) for mm in mx.TOLERANCES}
        assert one[1][2].max() < 64 and set(long_lists) <= set(one[1][1][0].tolist()) and all((one[1][3][0][one[1][1][0] == d] >= 0).sum() == 1 for d in long_lists)
        for S in mq.SHARES[1:]:
            eng.set_option("market_shares", S)
            for mm in mx.TOLERANCES:
                got = _call(eng, c.users, c.markets, excl, 64, mm, missing=True)
                assert eng.get_option("market_shares_used") == len(mq.share_bounds(c.I, S)) and _same(got, one[mm]), "%d shares, max_missing = %d" % (S, mm)
        _assert_missing_counts(eng, c, got, 3, "773 dishes, 64 shares")
    finally:
        eng.set_option("market_shares", 0)
    eng.check()


@pytest.mark.parametrize("R", mc.BITMAP_ROWS)
def test_both_bitmap_forms(engines, R):
    c, excl = mq.bitmap_case(R), mx.bitmap_exclusions(R)
    eng = engines(("bitmap", R), c)
    lds = R <= mq.LB
    for mm in (1, 2):
        got = _restated(eng, c, excl, 10, mm, "R = %d" % R, missing=True)
        assert eng.last_kernel() == ("m2d_markets_topk_excl_lds" if lds else "m2d_markets_topk_excl_l2")
        _assert_missing_counts(eng, c, got, mm, "R = %d" % R)
    _restated(eng, c, None, 64, 1, "R = %d, no exclusions" % R, missing=True)
    assert eng.last_kernel() == (mq.TOPK_LDS if lds else mq.TOPK_L2)
    try:
        eng.set_option("market_shares", 2)                   # 300 dishes: two shares, the bitmap still where the first launch left it
        _restated(eng, c, excl, 10, 2, "R = %d, two shares" % R, missing=True)
        assert eng.get_option("market_shares_used") == 2
    finally:
        eng.set_option("market_shares", 0)
    eng.check()


# ---- 4. with the rest of the engine --------------------------------------------------------------------------------------------------------
def test_three_categories_forty_columns(engines):
    c, excl = mq.other_shape_case(), mx.random_exclusions("other shape")
    eng = engines("other shape", c)
    for k in (10, 64):
        for mm in (0, 2):
            _restated(eng, c, excl, k, mm, "C = 3, E = 40", missing=True)
    eng.check()


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


@pytest.mark.parametrize("coef", mq.NORMAL_COEFS)
def test_normal_tables_list_the_pair_kernels_words(coef):
    c, excl = mq.normal_case(), mx.random_exclusions("normal")
    eng = _engine(c, coef=coef)
    k, mm = 10, 1
    got = _call(eng, c.users, c.markets, excl, k, mm, missing=True)
    for q in range(len(c.users)):
        cook = mc.restate(c.off, c.ids, c.R, c.markets[q], mm)[0]
        cook = cook[~np.isin(cook, excl[q])]
        assert got[2][q] == len(cook)
        words = _pair_words(eng, c.users[q], cook)
        o = mq.key_order(words, cook)[:k]
        kk = len(o)
        assert np.array_equal(got[1][q, :kk], cook[o]) and (got[1][q, kk:] == -1).all(), "coef %g request %d: ids" % (coef, q)
        mine, theirs = got[0][q, :kk], words[o]
        nan = np.isnan(theirs.view(np.float32))
        assert np.array_equal(np.isnan(mine.view(np.float32)), nan) and np.array_equal(mine[~nan], theirs[~nan]), "coef %g request %d: words" % (coef, q)
    assert mx.same_missing(got[3], mx.restate_missing(c.off, c.ids, c.R, c.markets, got[1], mm))
    eng.check()
    eng.close()


def test_a_user_base_shard():
    c, excl = mq.composed_case(64), mx.composed_exclusions(64)
    eng = _engine(c, user_base=1000)
    got = _call(eng, c.users + 1000, c.markets, excl, 10, 1, missing=True)
    want = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, excl, 1, 10)
    _assert_equal(got, want, "user_base 1000")
    assert mx.same_missing(got[3], mx.restate_missing(c.off, c.ids, c.R, c.markets, got[1], 1))
    got = _call(eng, c.users, c.markets, excl, 10, 1, missing=True)                 # ids below the shard: every row empty, counts kept
    with pytest.raises(IndexError, match="user id"):
        eng.check()
    assert (got[1] == -1).all() and np.array_equal(got[2], want[2]) and (got[3] == -1).all()
    eng.close()


def test_repeatable_and_follows_new_recipes_and_writers():
    import torch
    c, b = mq.composed_case(64), mc.extreme_recipe("hollow")
    excl = mx.composed_exclusions(64)
    eng = _engine(c)
    first = _restated(eng, c, excl, 10, 1, "first", missing=True)
    for _ in range(2):
        assert _same(first, _call(eng, c.users, c.markets, excl, 10, 1, missing=True))
    # write_memory: the lists equal a fresh engine's on the written tables
    rng = np.random.default_rng(6)
    t = lambda a: torch.as_tensor(a, device="cuda")
    B, L = 600, 7
    wu = (np.arange(B) % c.U).astype(np.int32)
    wi = rng.choice(np.flatnonzero(c.cats.sum(1) > 0), B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, c.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(c.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    written = _call(eng, c.users, c.markets, excl, 10, 1, missing=True)
    assert (written[0] != first[0]).mean() > 0.3, "write_memory changed nothing"
    from foodrec_amd import ScoringEngine
    fresh = ScoringEngine(eng.pm.cpu().numpy(), eng.re.cpu().numpy(), eng.ce.cpu().numpy(), coef=c.coef)
    fresh.set_dish_categories(c.cats)
    fresh.set_recipes(c.off, c.ids, c.R)
    assert _same(written, _call(fresh, c.users, c.markets, excl, 10, 1, missing=True)), "after write_memory"
    fresh.close()
    # replaced recipes
    off = np.concatenate([b.off[:c.I + 1], np.full(max(0, c.I - b.I), b.off[-1], np.int32)])[:c.I + 1]
    eng.set_recipes(off, b.ids[:off[-1]], b.R)
    markets = [np.arange(j % (b.R + 1), dtype=np.int32) for j in range(len(c.users))]
    second = _call(eng, c.users, markets, excl, 10, 1, missing=True)
    want = mx.restate(c.S, c.users, off, b.ids[:off[-1]], b.R, markets, excl, 1, 10)
    assert np.array_equal(second[2], want[2]) and mx.same_missing(second[3], mx.restate_missing(off, b.ids[:off[-1]], b.R, markets, second[1], 1))
    for q in range(len(c.users)):                                                    # (written tables are not exact: the sets, not the order)
        assert set(second[1][q][second[1][q] >= 0].tolist()) <= set(mc.restate(off, b.ids[:off[-1]], b.R, markets[q], 1)[0].tolist()) - set(excl[q].tolist())
    eng.check()
    eng.close()


def test_independent_of_the_other_market_calls_in_between(engines):
    c, excl = mq.composed_case(64), mx.composed_exclusions(64)
    eng = engines(("composed", 64), c)
    before = _call(eng, c.users, c.markets, excl, 10, 1, missing=True)
    shared = mc.composed_recipe().market
    old = _old(eng, c.users, c.markets, 10, 1)
    cook = eng.cookable_dishes(_dev(shared), 0).cpu().numpy()
    after = _call(eng, c.users, c.markets, excl, 10, 1, missing=True)
    assert _same(before, after), "topk_markets_excluding changed after topk_markets / cookable_dishes"
    assert _same(old, _old(eng, c.users, c.markets, 10, 1)), "topk_markets changed after topk_markets_excluding"
    assert np.array_equal(eng.cookable_dishes(_dev(shared), 0).cpu().numpy(), cook) and np.array_equal(cook, mc.composed_recipe().cookable)
    eng.check()


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors_are_latched_and_the_other_rows_are_right(engines):
    c, excl = mq.composed_case(64), mx.composed_exclusions(64)
    eng = engines(("composed", 64), c)
    k, nQ = 10, len(c.users)
    want = mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, excl, 1, k)
    wantm = lambda ids: mx.restate_missing(c.off, c.ids, c.R, c.markets, ids, 1)
    off, ids = mx.csr(excl)

    def others_right(got, rows, what):
        keep = np.setdiff1d(np.arange(nQ), rows)
        assert all(np.array_equal(a[keep], np.asarray(b)[keep]) for a, b in ((got[1], want[1]), (got[2], want[2]))), what
        assert mq.same_answer((got[0].view(np.float32)[keep], got[1][keep], got[2][keep]), tuple(w[keep] for w in want)), what
        assert mx.same_missing(got[3][keep], wantm(got[1])[keep]), what

    # an excluded id outside the catalogue: value and index in excl_ids named
    for pos, bad_id in ((int(off[20]), -1), (int(off[31]) - 1, c.I), (len(ids) - 1, 2 ** 31 - 1)):
        bad = ids.copy()
        bad[pos] = bad_id
        q = int(np.searchsorted(off, pos, side="right")) - 1
        got = _call(eng, c.users, c.markets, None, k, 1, missing=True, xcsr=(off, bad))
        with pytest.raises(IndexError, match=r"item id %d at position %d " % (bad_id, pos)):
            eng.check()
        others_right(got, [q], "bad excluded id at %d" % pos)
        eng.check()                                          # the latch is clear again
    # a segment that is not ascending: the id below its predecessor, by value and index
    q = 25
    pos = int(off[q]) + 100
    bad = ids.copy()
    bad[pos] = bad[pos - 1] - 1
    assert off[q] < pos - 1 and pos < off[q + 1] and bad[pos] >= 0
    got = _call(eng, c.users, c.markets, None, k, 1, missing=True, xcsr=(off, bad))
    with pytest.raises(ValueError, match=r"value %d at position %d " % (bad[pos], pos)):
        eng.check()
    others_right(got, [q], "segment not ascending")
    # a decreasing offset, an offset outside the array: latched, clamped before anything is read
    for q, value in ((10, int(off[10]) - 5), (40, len(ids) + 1000), (30, -7)):
        o = off.copy()
        o[q + 1] = value
        got = _call(eng, c.users, c.markets, None, k, 1, missing=True, xcsr=(o, ids))
        # (the request after a bad end offset starts outside as well: whichever of the two is latched first)
        # or an id of the segment that now starts in its neighbours' and is not ascending where they meet)
        with pytest.raises(ValueError, match="not ascending") as e:
            eng.check()
        assert int(re.search(r"at position (\d+) ", str(e.value)).group(1)) in {q + 1, q + 2} | set(off.tolist())
        others_right(got, [q, q + 1], "offsets, request %d" % q)
    # a bad user in one row: that row empty, its count right
    users = c.users.copy()
    users[30] = c.U
    got = _call(eng, users, c.markets, excl, k, 1, missing=True)
    with pytest.raises(IndexError, match=r"user id %d at position 30 " % c.U):
        eng.check()
    others_right(got, [30], "bad user")
    assert (got[1][30] == -1).all() and got[2][30] == want[2][30] and (got[3][30] == -1).all()
    # a bad market id: it contributes nothing
    moff, mids = mq.csr(c.markets)
    mids = mids.copy()
    mids[int(moff[20]) + 3] = c.R
    markets = [mids[moff[j]:moff[j + 1]] for j in range(nQ)]
    got = _call(eng, c.users, markets, excl, k, 1, missing=True)
    with pytest.raises(IndexError, match=r"ingredient id %d at position %d " % (c.R, int(moff[20]) + 3)):
        eng.check()
    _assert_equal(got, mx.restate(c.S, c.users, c.off, c.ids, c.R, markets, excl, 1, k), "bad market id")
    assert mx.same_missing(got[3], mx.restate_missing(c.off, c.ids, c.R, markets, got[1], 1))
    # the engine is usable afterwards
    _assert_equal(_call(eng, c.users, c.markets, excl, k, 1), want, "after the errors")
    eng.check()


def test_bad_arguments_and_refusals():
    import torch
    from foodrec_amd import ScoringEngine, _native
    from helpers import mlp_head
    c, excl = mq.composed_case(64), list(mx.composed_exclusions(64))
    eng = ScoringEngine(c.PM, c.RE, c.CE, coef=c.coef)
    eng.set_dish_categories(c.cats)
    lib = _native.lib()
    users, markets = _dev(c.users), [m for m in c.markets]
    with pytest.raises(ValueError, match="m2d_set_recipes first"):
        eng.topk_markets_excluding(users, markets, excl)
    eng.set_recipes(c.off, c.ids, c.R)
    for k in (0, 65):
        with pytest.raises(ValueError, match="1 <= k <= 64"):
            eng.topk_markets_excluding(users, markets, excl, k)
    with pytest.raises(ValueError, match="max_missing >= 0"):
        eng.topk_markets_excluding(users, markets, excl, 10, max_missing=-1)
    with pytest.raises(ValueError, match="54 markets for 53 users"):
        eng.topk_markets_excluding(users, markets + [[1]], excl)
    with pytest.raises(ValueError, match="52 lists for 53 queries"):
        eng.topk_markets_excluding(users, markets, list(excl[:52]))
    s, i, n, m = eng.topk_markets_excluding(users[:0], [], [], 10, 2, return_counts=True, return_missing=True)     # nQ = 0: nothing launched
    assert tuple(s.shape) == (0, 10) and tuple(i.shape) == (0, 10) and tuple(n.shape) == (0,) and tuple(m.shape) == (0, 10, 2)
    off, ids = (_dev(a) for a in mq.csr(c.markets))
    xoff, xids = (_dev(a) for a in mx.csr(excl))
    out_s, out_i = torch.empty((53, 10), device="cuda"), torch.empty((53, 10), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = lambda **kw: [kw.get("h", eng._h), kw.get("users", users.data_ptr()), kw.get("nQ", 53), kw.get("off", off.data_ptr()),
                         kw.get("ids", ids.data_ptr()), kw.get("nnz", ids.numel()), kw.get("xoff", xoff.data_ptr()), kw.get("xids", xids.data_ptr()),
                         kw.get("k", 10), kw.get("mm", 0), kw.get("s", out_s.data_ptr()), kw.get("i", out_i.data_ptr()), None, None, st]
    for kw in ({"nQ": -1}, {"nnz": -1}, {"users": None}, {"off": None}, {"ids": None}, {"s": None}, {"i": None}, {"k": 0}, {"k": 65}, {"mm": -1}):
        assert lib.m2d_topk_markets_excluding(*args(**kw)) == _native.M2D_ERR_INVALID_ARG, kw
    assert lib.m2d_topk_markets_excluding(*args(nQ=0, users=None)) == _native.M2D_OK
    # excl_ids null under offsets that are all zero: no exclusions; under offsets with a total: the segments reach outside an array of
    # length 0 -- latched (the total is on the device and the call never synchronises), nothing read, nothing excluded
    assert lib.m2d_topk_markets_excluding(*args(xoff=_dev(np.zeros(54, np.int64)).data_ptr(), xids=None)) == _native.M2D_OK
    eng.check()
    plain = out_i.cpu().numpy().copy()
    assert np.array_equal(plain, mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, 0, 10)[1])
    assert lib.m2d_topk_markets_excluding(*args(xids=None)) == _native.M2D_OK
    with pytest.raises(ValueError, match="at position"):
        eng.check()
    assert np.array_equal(out_i.cpu().numpy(), plain)
    rng = np.random.default_rng(3)
    eng.set_ingredients((rng.integers(-4, 5, (7, 64)) / 4).astype(np.float32), np.arange(c.I + 1, dtype=np.int32), rng.integers(0, 7, c.I).astype(np.int32))
    with pytest.raises(ValueError, match="m2d_topk_markets_excluding: the ingredient table is set"):
        eng.topk_markets_excluding(users, markets, excl)
    eng.clear_ingredients()
    eng.set_mlp_head(*mlp_head(320, 256, 64, rng))
    with pytest.raises(ValueError, match="m2d_topk_markets_excluding: the MLP head is set"):
        eng.topk_markets_excluding(users, markets, excl)
    eng.clear_mlp_head()
    _restated(eng, c, excl, 10, 1, "after the refusals", missing=True)              # the engine answers correctly afterwards
    eng.close()
    bare = ScoringEngine(c.PM, c.RE, c.CE, coef=c.coef)
    bare.set_recipes(c.off, c.ids, c.R)
    with pytest.raises(ValueError, match="m2d_set_dish_categories first"):
        bare.topk_markets_excluding(users, markets, excl)
    bare.close()


# ---- 6. the Python surface and the torch op ------------------------------------------------------------------------------------------------
def test_python_surface_returns_the_engines_words(engines):
    import types

    import torch

    import foodrec_amd
    c, excl = mq.composed_case(64), list(mx.composed_exclusions(64))
    eng = engines(("composed", 64), c)
    want = _call(eng, c.users, c.markets, excl, 10, 2, missing=True)
    raw = lambda x: np.ascontiguousarray(x.cpu().numpy()).view(np.int32)
    xoff, xids = mx.csr(excl)
    shuffled = [np.random.default_rng(q).permutation(np.concatenate([x, x[:5]])) for q, x in enumerate(excl)]     # any order, repeats
    for exclude in ([x.tolist() for x in excl], shuffled, (xoff, xids), (_dev(xoff), _dev(xids))):
        s, i, n, m = eng.topk_markets_excluding(_dev(c.users), c.markets, exclude, 10, 2, return_counts=True, return_missing=True)
        assert s.dtype == torch.float32 and i.dtype == n.dtype == m.dtype == torch.int32 and tuple(m.shape) == (53, 10, 2)
        assert all(np.array_equal(raw(x), y) for x, y in zip((s, i, n, m), want))
    pair = eng.topk_markets_excluding(c.users, c.markets, excl, max_missing=2)
    assert len(pair) == 2 and np.array_equal(raw(pair[1]), want[1])
    s, i, m = eng.topk_markets_excluding(c.users, c.markets, excl, max_missing=2, return_missing=True)
    assert np.array_equal(raw(m), want[3])
    off, ids = mq.csr(c.markets)
    out = torch.ops.m2d.topk_markets_excluding(eng.id, _dev(c.users), _dev(off), _dev(ids), _dev(xoff), _dev(xids), 10, 2)
    assert all(np.array_equal(raw(x), y) for x, y in zip(out, want))
    s, i, n, m = torch.ops.m2d.topk_markets_excluding(eng.id, _dev(c.users), _dev(off), _dev(ids), None, None, 10, 0)
    assert tuple(m.shape) == (53, 10, 0) and _same([raw(x) for x in (s, i, n)], _old(eng, c.users, c.markets, 10, 0))
    eng.check()
    args = types.SimpleNamespace(num_categories=4, num_users=c.U, embed_size=c.E, high_level_score_coefficient=c.coef)
    model = foodrec_amd.Model(args, c.PM, c.RE, c.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(c.cats)
    model.set_recipes((c.off, c.ids), c.R)
    users = [str(u) for u in c.users]
    s, i, n, m = model.topk_markets_excluding(users, [[str(v) for v in mk] for mk in c.markets], [[str(d) for d in x] for x in shuffled], 10, 2, missing=True)
    assert s.dtype == np.float32 and i.dtype == np.int32 and n.dtype == np.int32 and m.dtype == np.int32
    assert np.array_equal(s.view(np.int32), want[0]) and np.array_equal(i, want[1]) and np.array_equal(n, want[2]) and np.array_equal(m, want[3])
    three = model.topk_markets_excluding(users, c.markets, None, 10, 2)
    assert len(three) == 3 and _same([three[0].view(np.int32), three[1], three[2]], _old(eng, c.users, c.markets, 10, 2))
    # a dict keyed by the user as given: users 3 and 9 appear twice in the batch, under different markets
    had = {"3": [int(d) for d in mx.ranked(c, 3)[:2]] + [int(d) for d in mx.ranked(c, 51)[:2]], "9": [int(mx.ranked(c, 52)[0])]}
    lists = [had.get(u, ()) for u in users]
    s, i, n = model.topk_markets_excluding(users, c.markets, had, 10)
    _assert_equal((s.view(np.int32), i, n), mx.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, lists, 0, 10), "dict")
    with pytest.raises(ValueError, match="2 exclusion lists for 3 users"):
        model.topk_markets_excluding([1, 2, 3], [[1], [2], [3]], [[1], [2]])
    with pytest.raises(IndexError, match=r"item id %d at position 1 " % c.I):
        model.topk_markets_excluding([1], [[0, 1]], [[0, c.I]])
    with pytest.raises(ValueError, match="market together with exclude"):
        model.topk([1], 10, exclude=[[0]], market=[0, 1])
