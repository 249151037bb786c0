"""Requests, the numpy restatement and the stand-ins of the excluding market-request tests (tests/test_market_excluding_cases_cpu.py,
tests/test_gpu_market_excluding.py): m2d_topk_markets_excluding, m2d_topk_markets that leaves out each request's excluded dishes and
names, for every listed dish, the list entries its market lacks.

The restatement of the lists is market_request_cases.restate on recipe lists from which X_q's columns have been removed: an excluded
dish gets an empty list, and an empty list is never cookable, so it is neither counted nor ranked.  The missing entries are restated
straight from the definition.  Nothing here imports the engine.  Cases are computed once and shared (lru_cache); callers do not write
into them."""
import functools

import numpy as np

import market_cases as mc
import market_request_cases as mq
import seen_dish_cases as sd

STANDINS = ("first_for_all", "last_share_unfiltered", "excluded_counted", "window_last_missed")
MISSING_STANDINS = ("sorted", "repeat_once", "position_64_lost")
EDGE_IDS = (0, 63, 64, 65, 255, 256, 257)                    # and I - 1: both sides of a 64-dish group and of a 256-dish block
SEGMENT_LENGTHS = (0, 1, 63, 64, 65, 300)
KINDS = ("best", "all", "few", "mixed")
TOLERANCES = (1, 2, 3)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def without(off, ids, X):
    """the recipe lists with the lists of the dishes in X emptied: (offsets int32[I + 1], ids)"""
    off, ids = np.asarray(off, np.int64), np.asarray(ids)
    lens = np.diff(off)
    X = np.unique(np.asarray(X, np.int64))
    X = X[(X >= 0) & (X < len(lens))]
    keep = np.ones(len(ids), bool)
    for d in X:
        keep[off[d]:off[d + 1]] = False
    lens = lens.copy()
    lens[X] = 0
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), ids[keep]


def restate(S64, users, off, ids, R, markets, excl, max_missing, k, standin=None, shares=1):
    """(scores f64[nQ, k], ids i64[nQ, k], counts i64[nQ]) of the call; `excl`: nQ id sequences (any order, repeats allowed) or None.
    `standin`: what a subtly wrong kernel would return --
      "first_for_all"           request 0's exclusions are used for every request;
      "last_share_unfiltered"   the last of `shares` shares ignores the exclusions;
      "excluded_counted"        excluded dishes are left out of the list but still counted;
      "window_last_missed"      of the excluded ids inside one 64-dish group the last one is missed (a window one short)."""
    assert standin is None or standin in STANDINS
    nQ, I = len(users), len(off) - 1
    out_s, out_i, counts = np.full((nQ, k), np.nan), np.full((nQ, k), -1, np.int64), np.zeros(nQ, np.int64)
    share = mq.share_of(I, shares) if standin == "last_share_unfiltered" else None
    for q in range(nQ):
        X = np.zeros(0, np.int64) if excl is None else np.unique(np.asarray(excl[0 if standin == "first_for_all" else q], np.int64))
        X = X[(X >= 0) & (X < I)]
        if standin == "last_share_unfiltered" and share.max() > 0:
            X = X[share[X] != share.max()]
        if standin == "window_last_missed" and len(X):
            group = X // mq.DW
            X = X[np.concatenate([group[1:] == group[:-1], [False]])]
        o, i_ = without(off, ids, X)
        s, i, c = mq.restate(S64, users[q:q + 1], o, i_, R, markets[q:q + 1], max_missing, k)
        out_s[q], out_i[q], counts[q] = s[0], i[0], c[0]
        if standin == "excluded_counted":
            counts[q] = mq.restate(S64, users[q:q + 1], off, ids, R, markets[q:q + 1], max_missing, k)[2][0]
    return out_s, out_i, counts


def restate_missing(off, ids, R, markets, listed, max_missing, standin=None):
    """int64 [nQ, k, max_missing]: for listed[q, j] the ids of its list entries absent from markets[q], in list order, every occurrence,
    -1 from the number missing on and where listed[q, j] is -1.  `standin` --
      "sorted"             the absent ids come out ascending instead of in list order;
      "repeat_once"        an absent id that the list names twice is given once;
      "position_64_lost"   the entry at position 64 of a list (the first of its second batch) is never looked at."""
    assert standin is None or standin in MISSING_STANDINS
    off, ids = np.asarray(off, np.int64), np.asarray(ids, np.int64)
    nQ, k = listed.shape
    out = np.full((nQ, k, max_missing), -1, np.int64)
    for q in range(nQ):
        present = np.zeros(R, bool)
        m = np.asarray(markets[q], np.int64).reshape(-1)
        present[m[(m >= 0) & (m < R)]] = True
        for j in range(k):
            d = int(listed[q, j])
            if d < 0:
                continue
            seg = ids[off[d]:off[d + 1]]
            if standin == "position_64_lost":
                seg = np.delete(seg, 64) if len(seg) > 64 else seg
            absent = [int(v) for v in seg if not present[v]]
            if standin == "sorted":
                absent = sorted(absent)
            if standin == "repeat_once":
                absent = list(dict.fromkeys(absent))
            absent = absent[:max_missing]
            out[q, j, :len(absent)] = absent
    return out


def same_missing(a, b):
    return np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64))


def csr(excl, repeats=False):
    """(offsets int64[nQ + 1], ids int32) as the C ABI takes them: ascending within a segment; `repeats`: every third id twice"""
    lists = []
    for x in excl:
        x = np.unique(np.asarray(x, np.int64))
        lists.append(np.sort(np.concatenate([x, x[::3]])) if repeats else x)
    return mq.csr(lists)


def ranked(c, q, max_missing=0, X=()):
    """every cookable dish of request q that is not in X, in the order"""
    o, i_ = without(c.off, c.ids, X)
    cook = mc.restate(o, i_, c.R, c.markets[q], max_missing)[0]
    return mq._ranked(c.S[c.users[q]], cook, len(cook))[1]


# ---- 1. exclusion edges on the catalogue cases ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exclusions(n, kind):
    """eight exclusion lists for market_request_cases.catalogue_case(n)'s eight requests --
      "best"    the request's best cookable dish and the lowest dish it cannot cook (no effect);
      "all"     every dish cookable at max_missing = 2: count 0 at 0, 1 and 2;
      "few"     all but the three LAST of the order at max_missing = 0: fewer than k left, the best ones gone;
      "mixed"   an empty first and an empty last segment, between them SEGMENT_LENGTHS[1:] and a random 40 ids, drawn without order."""
    c = mq.catalogue_case(n)
    rng = np.random.default_rng(41000 + n)
    out = []
    for q in range(len(c.users)):
        if kind == "best":
            order = ranked(c, q)
            cook = set(mc.restate(c.off, c.ids, c.R, c.markets[q], 2)[0].tolist())
            x = list(order[:1]) + [d for d in range(n) if d not in cook][:1]
        elif kind == "all":
            x = mc.restate(c.off, c.ids, c.R, c.markets[q], 2)[0]
        elif kind == "few":
            x = ranked(c, q)[:-3]
        else:
            length = ((0,) + SEGMENT_LENGTHS[1:] + (40, 0))[q]
            x = rng.permutation(n)[:length]
        out.append(np.asarray(x, np.int64))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_case(n):
    """n dishes with lists of 1 - 3 entries over 20 ingredients, none empty (in market_cases.catalogue_recipe the dishes at the group
    edges have empty lists and are never cookable); four requests: the full market twice -- every dish cookable --, ids 0 .. 9 and
    0 .. 14.  Exclusions: EDGE_IDS and I - 1; those and their neighbours; EDGE_IDS and I - 1 again; none."""
    rng = np.random.default_rng(45000 + n)
    off, ids = mc._csr([[int(v) for v in rng.integers(0, 20, int(rng.integers(1, 4)))] for _ in range(n)])
    PM, RE, CE, cats = sd.exact_tables(rng, 8, n, 4)
    edges = sorted({d for d in EDGE_IDS + (n - 1,) if d < n})
    near = sorted({e for d in edges for e in (d - 1, d, d + 1) if 0 <= e < n})
    markets = [np.arange(20, dtype=np.int32), np.arange(20, dtype=np.int32), np.arange(10, dtype=np.int32), np.arange(15, dtype=np.int32)]
    return mq._case(I=n, R=20, off=off, ids=ids, PM=PM, RE=RE, CE=CE, cats=cats, coef=sd.COEF, S=sd.score_matrix(PM, RE, CE, cats),
                    users=np.arange(4, dtype=np.int32), markets=markets,
                    excl=(np.asarray(edges, np.int64), np.asarray(near, np.int64), np.asarray(edges, np.int64), np.zeros(0, np.int64)))


# ---- 2. share boundaries ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def share_exclusions():
    """for market_request_cases.share_case("773") (the full market, equal scores straddling every boundary): the dishes on both sides
    of every boundary of 2, 3 and 4 shares, and each request's three best dishes"""
    c = mq.share_case("773")
    edge = sorted({d for S in (2, 3, 4) for b, e in mq.share_bounds(c.I, S) for d in (b - 1, b, e - 1, e) if 0 <= d < c.I})
    return tuple(np.asarray(edge + list(ranked(c, q)[:3]), np.int64) for q in range(len(c.users)))


# ---- 3. 51 requests, each with its own list; a history longer than the workaround's slack -------------------------------------------------
@functools.lru_cache(maxsize=None)
def composed_exclusions(E):
    """for market_request_cases.composed_case(E): request q leaves out 200 random dishes and its own best q mod 4 cookable ones"""
    c = mq.composed_case(E)
    rng = np.random.default_rng(42000)
    return tuple(np.concatenate([rng.permutation(c.I)[:200], ranked(c, q)[:q % 4]]).astype(np.int64) for q in range(len(c.users)))


HISTORY_K = 10
HISTORY = 64 - HISTORY_K + 5                                 # more than 64 - k of the best: asking for 64 and filtering cannot fill k


@functools.lru_cache(maxsize=None)
def history_exclusions():
    """for composed_case(64): every request has had its HISTORY best cookable dishes"""
    c = mq.composed_case(64)
    return tuple(ranked(c, q)[:HISTORY].astype(np.int64) for q in range(len(c.users)))


def host_workaround(c, excl, k, max_missing=0):
    """today's way: topk_markets at k = 64, then drop the excluded ids on the host and keep k"""
    s, i, n = mq.restate(c.S, c.users, c.off, c.ids, c.R, c.markets, max_missing, 64)
    out_s, out_i = np.full((len(c.users), k), np.nan), np.full((len(c.users), k), -1, np.int64)
    for q in range(len(c.users)):
        keep = [j for j in range(64) if i[q, j] >= 0 and i[q, j] not in set(np.asarray(excl[q]).tolist())][:k]
        out_s[q, :len(keep)], out_i[q, :len(keep)] = s[q, keep], i[q, keep]
    return out_s, out_i


# ---- 4. missing entries: the fixed layout ----------------------------------------------------------------------------------------------
MISSING_DISHES = 70
LAYOUT = {                                                   # dish: (list length, {position: absent id})
    2: (63, {0: 9, 62: 3}),                                  # first and last of a list one short of a batch
    3: (64, {0: 7, 63: 5}),                                  # first and last of exactly one batch
    4: (65, {0: 11, 63: 1, 64: 3}),                          # the last of the first batch, the first (and last) of the second
    5: (193, {0: 13, 64: 5, 192: 1}),                        # four batches: first, position 64, last
    6: (193, {63: 21, 64: 21}),                              # ONE id twice and absent, on both sides of the batch edge
    7: (3, {0: 15, 2: 15}),                                  # one id twice in a short list
    8: (2, {}),
}


@functools.lru_cache(maxsize=None)
def missing_case():
    """70 dishes (two groups) over 100 ingredients, the even ids at the main market: LAYOUT's lists, the rest 1 - 6 entries with 0 - 3
    odd ones in random places, dish 69 empty.  Six requests: the even market (users 0, 1), the even market without ids 0 and 2, the
    full market, the empty market (only lists of at most max_missing entries are cookable: rows shorter than k) and ids 0 .. 49.  Request 0
    has had dishes 20 .. 39, so at k = 64 every other cookable dish of its market is listed, LAYOUT's among them."""
    rng = np.random.default_rng(43000)
    even, odd = np.arange(0, 100, 2), np.arange(1, 100, 2)
    lists = []
    for d in range(MISSING_DISHES):
        if d in LAYOUT:
            n, absent = LAYOUT[d]
            l = rng.choice(even[2:], n)
            for pos, v in absent.items():
                l[pos] = v
        elif d == MISSING_DISHES - 1:
            l = np.zeros(0, np.int64)
        else:
            n = int(rng.integers(1, 7))
            bad = min(n, int(rng.integers(0, 4)))
            l = rng.permutation(np.concatenate([rng.choice(odd, bad), rng.choice(even, n - bad)]))
        lists.append([int(v) for v in l])
    off, ids = mc._csr(lists)
    PM, RE, CE, cats = sd.exact_tables(rng, 8, MISSING_DISHES, 4)
    markets = [even.astype(np.int32), even.astype(np.int32), even[2:].astype(np.int32), np.arange(100, dtype=np.int32), np.zeros(0, np.int32),
               np.arange(50, dtype=np.int32)]
    excl = [np.arange(20, 40), np.asarray([3, 8, 40]), np.zeros(0, np.int64), np.asarray([0, 69]), np.asarray([1]), np.zeros(0, np.int64)]
    return mq._case(I=MISSING_DISHES, R=100, off=off, ids=ids, PM=PM, RE=RE, CE=CE, cats=cats, coef=sd.COEF,
                    S=sd.score_matrix(PM, RE, CE, cats), users=np.arange(6, dtype=np.int32), markets=markets, excl=tuple(excl))


# ---- 5. bitmap forms ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bitmap_exclusions(R):
    """for market_request_cases.bitmap_case(R)'s six requests: the best dish of each at max_missing = 1, and dishes 0 .. 3 (one list per
    named id) for the last two"""
    c = mq.bitmap_case(R)
    return tuple(np.concatenate([ranked(c, q, 1)[:1], np.arange(4) if q >= 4 else np.zeros(0, np.int64)]).astype(np.int64)
                 for q in range(len(c.users)))


# ---- 6. other shapes, normal tables -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_exclusions(which):
    """"other shape" / "normal": a random 0 - 30 dishes per request of market_request_cases.other_shape_case() / normal_case()"""
    c = mq.other_shape_case() if which == "other shape" else mq.normal_case()
    rng = np.random.default_rng(44000)
    return tuple(rng.permutation(c.I)[:int(rng.integers(0, 31))].astype(np.int64) for _ in range(len(c.users)))
