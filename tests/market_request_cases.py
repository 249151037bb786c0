"""Requests, the numpy restatement and the stand-ins of the market-request tests (tests/test_market_request_cases_cpu.py,
tests/test_gpu_market_requests.py): m2d_topk_markets, one (user, market) per request, filtered, scored and listed in one call.

The restatement of a request: market_cases.restate gives the cookable ids and their count, slate_cases.exact_lists ranks the request's
row of the float64 score matrix over those columns, and the row is padded with NaN / -1.  Nothing here imports the engine.  Cases are
computed once and shared (lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

import dense_topk_cases as dk
import market_cases as mc
import seen_dish_cases as sd
import slate_cases as sc

# the kernel's constants, restated (tests/test_market_request_cases_cpu.py holds each against its source line)
DW = 64             # m2d_market_requests.hip: constexpr int MQ_DW = 64 (dishes per group, one per lane)
WAVES = 4           # m2d_market_requests.hip: constexpr int MQ_WAVES = 4
DB = DW * WAVES     # m2d_market_requests.hip: constexpr int MQ_DB = MQ_DW * MQ_WAVES (dishes per catalogue block: a share's unit)
EB = 64             # m2d_market_requests.hip: constexpr int MQ_EB = 64 (entries per batch)
BF = 4              # m2d_market_requests.hip: constexpr int MQ_BF = 4 (batches in flight: lists of 63 / 64 / 65 / 193 entries and a group's run of
                    # 256 entries and more cross the edges of a batch and of four)
LB = 1 << 16        # m2d_market_requests.hip: constexpr int MQ_LDS_BITS = 1 << 16
KMAX = 64           # m2d_market_requests.hip: constexpr int MQ_KMAX = 64
MAX_SHARES = 64     # m2d_market_requests.hip: constexpr int MQ_MAX_SHARES = 64

TOPK_LDS, TOPK_L2 = "m2d_markets_topk_lds", "m2d_markets_topk_l2"
CATALOGUES = (1, 63, 64, 65, 255, 256, 257, 773)
KS = (1, 10, 64)
SHARES = (1, 2, 3, 4, 64)
STANDINS = ("shared_bitmap", "count_listed", "tie_to_higher_share", "drop_last_share", "nan_ranked_first")


# ---- the launcher's share rule ------------------------------------------------------------------------------------------------------
def shares_used(option, nQ, num_cu, n_dishes):
    """S = clamp(option or 4 num_cu / nQ, 1, min(64, ceil(I / 256)))"""
    nb = -(-n_dishes // DB)
    S = option if option > 0 else 4 * num_cu // nQ
    return max(1, min(S, MAX_SHARES, nb))


def share_bounds(n_dishes, S):
    """[(first dish, end dish)] of the S shares: catalogue blocks [s nb / S, (s + 1) nb / S) of 256 dishes"""
    nb = -(-n_dishes // DB)
    S = max(1, min(S, MAX_SHARES, nb))
    return [(s * nb // S * DB, min(n_dishes, (s + 1) * nb // S * DB)) for s in range(S)]


def share_of(n_dishes, S):
    """share index of every dish"""
    out = np.empty(n_dishes, np.int64)
    for s, (b, e) in enumerate(share_bounds(n_dishes, S)):
        out[b:e] = s
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _ranked(row, cook, k, share=None, nan_first=False):
    """the first k of `cook` by the order: score descending, equal scores to the lower id, NaN last in id order.  Stand-ins: `share`
    (an int array) sends equal scores in different shares to the higher share; `nan_first` lists NaN ahead of every number."""
    cook = np.asarray(cook, np.int64)
    s = row[cook]
    nan = np.isnan(s)
    tie = np.where(nan, 0, -share[cook]) if share is not None else np.zeros(len(cook), np.int64)
    o = np.lexsort((cook, tie, -np.where(nan, -np.inf, s), ~nan if nan_first else nan))[:k]
    return s[o], cook[o]


def restate(S64, users, off, ids, R, markets, max_missing, k, standin=None, shares=1):
    """(scores f64[nQ, k], ids i64[nQ, k], counts i64[nQ]) of the call.  S64: [U, I] float64 scores, users index its rows; a user
    outside [0, U) gives an empty row with the market's count.  `standin`: what a subtly wrong kernel would return --
      "shared_bitmap"         every request is answered from request 0's market;
      "count_listed"          counts are min(count, k);
      "tie_to_higher_share"   equal scores on two sides of a share boundary (`shares` shares) go to the higher id;
      "drop_last_share"       the last of `shares` shares is never ranked (it is still counted);
      "nan_ranked_first"      empty-mask dishes come ahead of the finite ones."""
    assert standin is None or standin in STANDINS
    nQ, I = len(users), len(off) - 1
    out_s, out_i, counts = np.full((nQ, k), np.nan), np.full((nQ, k), -1, np.int64), np.zeros(nQ, np.int64)
    share = share_of(I, shares) if standin in ("tie_to_higher_share", "drop_last_share") else None
    for q in range(nQ):
        market = markets[0] if standin == "shared_bitmap" else markets[q]
        cook = mc.restate(off, ids, R, market, max_missing)[0]
        counts[q] = min(len(cook), k) if standin == "count_listed" else len(cook)
        if not 0 <= users[q] < S64.shape[0]:
            continue
        if standin == "drop_last_share":
            cook = cook[share[cook] != share.max()] if share.max() > 0 else cook[:0]
        s, i = _ranked(S64[users[q]], cook, k, share if standin == "tie_to_higher_share" else None, standin == "nan_ranked_first")
        out_s[q, :len(i)], out_i[q, :len(i)] = s, i
    return out_s, out_i, counts


def restate_with_exact_lists(S64, users, off, ids, R, markets, max_missing, k):
    """the same through slate_cases.exact_lists, the ranking the slate tests use: a second statement of the order"""
    nQ = len(users)
    out_s, out_i, counts = np.full((nQ, k), np.nan), np.full((nQ, k), -1, np.int64), np.zeros(nQ, np.int64)
    for q in range(nQ):
        cook = mc.restate(off, ids, R, markets[q], max_missing)[0]
        counts[q] = len(cook)
        kk = min(k, len(cook))
        if kk:
            s, i = sc.exact_lists(S64[[users[q]]][:, cook], cook, kk)
            out_s[q, :kk], out_i[q, :kk] = s[0], i[0]
    return out_s, out_i, counts


def same_answer(a, b):
    """the GPU file's comparison: ids and counts as integers, scores as float32 words (-0 folded onto +0, NaN equal to NaN)"""
    (sa, ia, ca), (sb, ib, cb) = a, b
    nan = np.isnan(np.asarray(sb, np.float64))
    return (np.array_equal(np.asarray(ia, np.int64), np.asarray(ib, np.int64)) and np.array_equal(np.asarray(ca, np.int64), np.asarray(cb, np.int64))
            and np.array_equal(np.isnan(np.asarray(sa, np.float64)), nan)
            and np.array_equal(sc.bits(np.where(nan, 0, sa)), sc.bits(np.where(nan, 0, sb))))


def csr(markets):
    """(offsets int64[nQ + 1], ids int32) of a list of markets"""
    off = np.zeros(len(markets) + 1, np.int64)
    np.cumsum([len(m) for m in markets], out=off[1:])
    ids = np.concatenate([np.asarray(m, np.int32) for m in markets]).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return off, ids


def _case(**kw):
    r = types.SimpleNamespace(**kw)
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---- 1. catalogue edges ---------------------------------------------------------------------------------------------------------------
CAT_PREFIXES = (1, 2, 7, 40, 99)


@functools.lru_cache(maxsize=None)
def catalogue_case(n):
    """market_cases.catalogue_recipe(n) on seen_dish_cases.exact_tables (E = 4, 8 users); eight requests: the even-id market, the full
    market, the empty market and five prefix markets, one user each"""
    r = mc.catalogue_recipe(n)
    PM, RE, CE, cats = sd.exact_tables(np.random.default_rng(n), 8, n, 4)
    markets = [r.market, np.arange(r.R, dtype=np.int32), np.zeros(0, np.int32)] + [np.arange(m, dtype=np.int32) for m in CAT_PREFIXES]
    return _case(I=n, R=r.R, off=r.off, ids=r.ids, longest=r.longest, PM=PM, RE=RE, CE=CE, cats=cats, coef=sd.COEF,
                 S=sd.score_matrix(PM, RE, CE, cats), users=np.arange(8, dtype=np.int32), markets=markets,
                 tolerances=(0, 1, 2, r.longest))


# ---- 2. bitmap edges ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bitmap_case(R):
    """market_cases.bitmap_recipe(R): the six MARKETS as six requests of ONE call, users 0 .. 5"""
    r = mc.bitmap_recipe(R)
    PM, RE, CE, cats = sd.exact_tables(np.random.default_rng(R % 9973), 8, r.I, 4)
    return _case(I=r.I, R=R, off=r.off, ids=r.ids, PM=PM, RE=RE, CE=CE, cats=cats, coef=sd.COEF, S=sd.score_matrix(PM, RE, CE, cats),
                 users=np.arange(6, dtype=np.int32), markets=[mc.market_ids(name, R) for name in mc.MARKETS])


# ---- 3. 51 different markets in one call ---------------------------------------------------------------------------------------------
COMPOSED_KS = (1, 7, 10, 64)
COMPOSED_WIDTHS = (4, 64, 200)


@functools.lru_cache(maxsize=None)
def composed_case(E):
    """market_cases.composed_recipe() over slate_cases.exact_recipe(E)'s 600 dishes: request m has market range(m), m = 0 .. 50, and
    user m mod U; two more requests repeat user 3 under market range(40) and market range(3) under user 9"""
    x, m = sc.exact_recipe(E), mc.composed_recipe()
    markets = [np.arange(j, dtype=np.int32) for j in range(51)] + [np.arange(40, dtype=np.int32), np.arange(3, dtype=np.int32)]
    users = np.asarray([j % x.U for j in range(51)] + [3, 9], np.int32)
    counts = np.asarray([len(mc.restate(m.off, m.ids, m.R, mk, 0)[0]) for mk in markets])
    return _case(E=E, U=x.U, I=x.I, R=m.R, off=m.off, ids=m.ids, PM=x.PM, RE=x.RE, CE=x.CE, cats=x.cats, coef=x.coef, S=x.S, users=users,
                 markets=markets, counts=counts)


# ---- 4. shares ------------------------------------------------------------------------------------------------------------------------
def straddling_ties(S64, user, cook, k, shares, n_dishes):
    """pairs (a, b) of cookable dishes with equal scores for `user`, in different shares, at least one of them inside the first k"""
    share = share_of(n_dishes, shares)
    s, i = _ranked(S64[user], cook, len(cook))
    place = {int(d): p for p, d in enumerate(i)}
    out = []
    for p in range(len(i) - 1):
        j = p + 1
        while j < len(i) and s[j] == s[p]:
            if share[i[p]] != share[i[j]] and min(place[int(i[p])], place[int(i[j])]) < k:
                out.append((int(i[p]), int(i[j])))
            j += 1
    return out


@functools.lru_cache(maxsize=None)
def share_case(which):
    """"773": catalogue_case(773) with dishes 600 .. 772 given the rows and masks of dishes 0 .. 172, so equal scores straddle
    every boundary of 2, 3 and 4 shares; "600": composed_case(64) with the same edit on dishes 300 .. 599 <- 0 .. 299 (empty masks
    kept where they were); "hollow" / "last wave": market_cases.extreme_recipe, a share without a cookable dish and the last share alone"""
    if which in ("hollow", "last wave"):
        r = mc.extreme_recipe(which)
        PM, RE, CE, cats = sd.exact_tables(np.random.default_rng(77), 8, r.I, 4)
        return _case(I=r.I, R=r.R, off=r.off, ids=r.ids, PM=PM, RE=RE, CE=CE, cats=cats, coef=sd.COEF, S=sd.score_matrix(PM, RE, CE, cats),
                     users=np.arange(8, dtype=np.int32), markets=[r.market] * 8, max_missing=0)
    if which == "773":
        c = catalogue_case(773)
        RE, cats = c.RE.copy(), c.cats.copy()
        RE[600:773], cats[600:773] = RE[0:173], cats[0:173]
        markets = [np.arange(c.R, dtype=np.int32)] * 8                       # the full market: every non-empty list is cookable
        return _case(I=c.I, R=c.R, off=c.off, ids=c.ids, PM=c.PM, RE=RE, CE=c.CE, cats=cats, coef=c.coef,
                     S=sd.score_matrix(c.PM, RE, c.CE, cats), users=c.users, markets=markets, max_missing=0)
    c = composed_case(64)
    RE, cats = c.RE.copy(), c.cats.copy()
    keep = cats[300:600].sum(1) > 0
    RE[300:600][keep], cats[300:600][keep] = RE[0:300][keep], cats[0:300][keep]
    users = np.arange(16, dtype=np.int32)
    return _case(I=c.I, R=c.R, off=c.off, ids=c.ids, PM=c.PM, RE=RE, CE=c.CE, cats=cats, coef=c.coef,
                 S=sd.score_matrix(c.PM, RE, c.CE, cats, users=users), users=users, markets=[np.arange(c.R, dtype=np.int32)] * 16, max_missing=8)


# ---- 5. another category count --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def other_shape_case():
    """dense_topk_cases.exact_recipe(3, 40) -- C = 3, E = 40, ten empty-mask dishes, copies -- with recipe lists of 0 - 6 entries over
    12 ingredients drawn for its dishes; 24 requests with markets of 0 - 12 ids, repeats included"""
    x = dk.exact_recipe(3, 40)
    rng = np.random.default_rng(36000)
    lens = rng.integers(0, 7, x.I)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(0, 12, int(off[-1])).astype(np.int32)
    markets = [rng.integers(0, 12, int(rng.integers(0, 13))).astype(np.int32) for _ in range(24)]
    return _case(I=x.I, R=12, off=off, ids=ids, PM=x.PM, RE=x.RE, CE=x.CE, cats=x.cats, coef=x.coef, S=x.S,
                 users=rng.integers(0, x.U, 24).astype(np.int32), markets=markets)


# ---- 6. normal tables -----------------------------------------------------------------------------------------------------------------
NORMAL_COEFS = (0.5, 0.99)


@functools.lru_cache(maxsize=None)
def normal_case():
    """N(0, 1 / E) tables at E = 64, U = 48, I = 700, 0/1 masks, three empty-mask dishes; lists of 1 - 6 over 20 ingredients; 64 requests
    with markets of 4 - 16 ids"""
    rng = np.random.default_rng(37000)
    U, I, E, R = 48, 700, 64, 20
    PM, RE, CE = sd.normal_tables(rng, U, I, E)
    cats = sd.masks(rng, I)
    cats[[3, 333, 699]] = 0.0
    lens = rng.integers(1, 7, I)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(0, R, int(off[-1])).astype(np.int32)
    markets = [rng.permutation(R)[:int(rng.integers(4, 17))].astype(np.int32) for _ in range(64)]
    markets[0] = np.arange(R, dtype=np.int32)                                 # everything: the empty-mask dishes are listed last
    return _case(U=U, I=I, E=E, R=R, off=off, ids=ids, PM=PM, RE=RE, CE=CE, cats=cats, users=rng.integers(0, U, 64).astype(np.int32),
                 markets=markets)


def key_order(words, ids):
    """tkm_key's rule restated in numpy on float32 WORDS: the order of (score word, id) pairs -- NaN last, otherwise descending by
    value with -0 folded onto +0, equal values to the lower id"""
    s = np.asarray(words, np.int32).view(np.float32).astype(np.float64)
    nan = np.isnan(s)
    return np.lexsort((np.asarray(ids, np.int64), -np.where(nan, -np.inf, s), nan))
