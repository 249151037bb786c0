"""Inputs, references and stand-ins of the seen-dish filtering tests (tests/test_seen_dish_cases_cpu.py,
tests/test_gpu_seen_dish_edges.py; the helpers also serve tests/test_gpu_catalogue_rank.py and tests/test_gpu_topk_excluding.py).

Everything here is the oracle's: oracle.inference_f64 over the whole catalogue, the ranking order (score descending, NaN last, equal
scores to the lower id), and the launchers' share-count formulas restated on the host.  Nothing here imports the engine.  Recipes and
their references are computed once and shared (lru_cache); callers do not write into them."""
import functools
import math
import types

import numpy as np

from helpers import TOL

COEF = 0.5
EXACT_PATTERNS = (1, 2, 4, 8, 3, 5, 6, 9, 10, 12, 15)      # no popcount 3: no division by 3
EXCL_XS = 60                                                # m2d_catalogue_excl.hip: ids per user the one-lane scan keeps in LDS

# ---- the helpers the two older GPU files shared -------------------------------------------------------------------------------------


def masks(rng, I, C=4, allowed=None):
    if allowed is None:
        m = rng.integers(0, 2, (I, C)).astype(np.float32)
        z = m.sum(1) == 0
        m[z, rng.integers(0, C, int(z.sum()))] = 1.0
        return m
    pats = np.asarray(allowed)
    bits = pats[rng.integers(0, len(pats), I)]
    return ((bits[:, None] >> np.arange(C)[None, :]) & 1).astype(np.float32)


def normal_tables(rng, U, I, E, C=4):
    s = 1.0 / math.sqrt(E)
    PM = (rng.standard_normal((U, C + 1, E)) * s).astype(np.float32)
    RE = (rng.standard_normal((I, E)) * s).astype(np.float32)
    CE = (rng.standard_normal((C, E)) * s).astype(np.float32)
    return PM, RE, CE


def exact_tables(rng, U, I, E):
    """Entries k / 16, k in -16 .. 16, masks from EXACT_PATTERNS: at coef 0.5 every float32 operation of a score is exact."""
    f = lambda shape: (rng.integers(-16, 17, shape) / 16.0).astype(np.float32)      # noqa: E731
    return f((U, 5, E)), f((I, E)), f((4, E)), masks(rng, I, allowed=list(EXACT_PATTERNS))


def oracle_scores(PM, RE, CE, cats, u, coef, dtype=np.float64):
    from oracle import m2d_oracle as oracle
    I = RE.shape[0]
    return oracle.inference(PM, RE, CE, np.full(I, u, np.int32), np.arange(I, dtype=np.int32), cats, coef, dtype)


def host_rank(s64, p, excl=()):
    """rank of p over d != p, d not in excl: score desc, NaN last, equal scores to the lower id"""
    I = s64.size
    d = np.arange(I)
    keep = d != p
    if len(excl):
        keep[np.asarray(list(excl), dtype=np.int64)] = False
        keep[p] = False
    sp = s64[p]
    if np.isnan(sp):
        prec = ~np.isnan(s64) | (d < p)
    else:
        prec = (s64 > sp) | ((s64 == sp) & (d < p))
    return int((prec & keep).sum())


def host_topk(s64, k, excl):          # s64: oracle.inference_f64 over the whole catalogue for one user
    keep = np.ones(s64.size, bool); keep[list(excl)] = False
    d = np.flatnonzero(keep); key = np.where(np.isnan(s64[d]), -np.inf, s64[d])
    return d[np.lexsort((d, -key))[:k]]


def gather_csr(off, ids, rows):
    """the CSR whose row r is row rows[r] of (off, ids)"""
    rows = np.asarray(rows, np.int64)
    lens = np.diff(off)[rows]
    starts = np.asarray(off)[:-1][rows]
    qoff = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=qoff[1:])
    idx = np.repeat(starts - qoff[:-1], lens) + np.arange(qoff[-1])
    return qoff, ids[idx]


def per_query_csr(off, ids, k):
    """the CSR of U users -> the CSR of U k queries, user u's segment repeated for its k queries"""
    return gather_csr(off, ids, np.repeat(np.arange(len(off) - 1), k))


def lists_csr(lists):
    """ascending, distinct id lists -> (offsets int64, ids int32), as foodrec_amd.ops.exclusion_csr lays them out"""
    lists = [np.unique(np.asarray(x, np.int64)) for x in lists]
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([x.size for x in lists], out=off[1:])
    return off, (np.concatenate(lists) if off[-1] else np.zeros(0)).astype(np.int32)


def assert_rank_band(s64, p, rank, score):
    """test_rank_within_oracle_band's check of one query: the rank between the counts at s* +- 1e-5 max(1, |s*|), the score within TOL"""
    sp = s64[p]
    t = 1e-5 * max(1.0, abs(sp))
    d = np.arange(s64.size) != p
    lo = int(((s64 > sp + t) & d).sum())
    hi = int(((s64 >= sp - t) & d).sum())
    assert lo <= rank <= hi, (p, lo, rank, hi)
    assert abs(float(score) - sp) <= TOL * max(1.0, abs(sp)), (p, score, sp)


def assert_list_band(s64, excl, ids, scores):
    """test_lists_within_oracle_band's check of one user's list"""
    ls = s64[ids]
    t = 1e-5 * np.maximum(1.0, np.abs(ls))
    assert (ls[1:] <= ls[:-1] + t[:-1]).all(), ls             # non-increasing within t
    rest = np.ones(s64.size, bool)
    rest[excl] = False
    rest[ids] = False
    assert (s64[rest] <= ls[-1] + t[-1]).all(), (s64[rest].max(), ls[-1])
    assert (np.abs(scores - ls) <= TOL * np.maximum(1.0, np.abs(ls))).all(), (scores, ls)


# ---- whole-catalogue references -----------------------------------------------------------------------------------------------------
def score_matrix(PM, RE, CE, cats, coef=COEF, dtype=np.float64, users=None):
    """[len(users), I] oracle.inference scores, a user at a time"""
    users = range(PM.shape[0]) if users is None else users
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([oracle_scores(PM, RE, CE, cats, int(u), coef, dtype) for u in users])


def positions(S, higher_id=False):
    """pos[u, d]: the place of dish d in user u's order over the whole catalogue (== host_rank(S[u], d)); `higher_id`: the
    stand-in that resolves equal scores (NaN included) to the HIGHER id"""
    U, I = S.shape
    ids = np.arange(I)
    pos = np.empty((U, I), np.int64)
    for u in range(U):
        nan = np.isnan(S[u])
        o = np.lexsort((-ids if higher_id else ids, -np.where(nan, -np.inf, S[u]), nan))
        pos[u, o] = ids
    return pos


def ranks_excluding(pos, users, items, off=None, ids=None):
    """host_rank for queries (users[q], items[q]) with query q's exclusions row q of (off, ids): pos[u, p] less the excluded ids,
    p itself apart, that precede p"""
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    r = pos[users, items].copy()
    if off is not None and off[-1]:
        q = np.repeat(np.arange(users.size), np.diff(off))
        x = np.asarray(ids, np.int64)
        before = (pos[users[q], x] < r[q]) & (x != items[q])
        r -= np.bincount(q[before], minlength=users.size)
    return r


def topk_lists(S, users, k, lists, higher_id=False):
    """[len(users), k] host_topk ids (-1 where fewer than k dishes remain)"""
    out = np.full((len(users), k), -1, np.int64)
    for j, u in enumerate(users):
        if higher_id:
            keep = np.ones(S.shape[1], bool); keep[list(lists[j])] = False
            d = np.flatnonzero(keep); key = np.where(np.isnan(S[u][d]), -np.inf, S[u][d])
            w = d[np.lexsort((-d, -key))[:k]]
        else:
            w = host_topk(S[u], k, lists[j])
        out[j, :w.size] = w
    return out


# ---- 1. widths -----------------------------------------------------------------------------------------------------------------------
WIDTHS = (4, 12, 20, 48, 100, 128, 132, 200, 256)
WIDTH_U, WIDTH_I, WIDTH_HELD = 24, 700, 40
EMPTY_DISHES = (5, 300, 600)                                # (655 copies 5: empty too)
COPY_TO, COPIES = 650, 50                                   # dishes 650 .. 699 copy dishes 0 .. 49
OWN_CYCLE = (0, 3, 7, 16, 40)
NORMAL_WIDTHS = (48, 100, 132, 256)


def row_width(E):
    """grouped_row_width (m2d_catalogue_plan.hip): the sorted dish table's row stride"""
    return E if E in (32, 64, 128) else (32 if E < 32 else 64 if E < 64 else 128 if E < 128 else 256)


def one_lane_width(E):
    """the E4MAX of the one-lane kernels' instantiation, None for the 16-lane forms (E > 128)"""
    return 8 if E <= 32 else 16 if E <= 64 else 32 if E <= 128 else None


def _catalogue_edits(RE, cats):
    cats[list(EMPTY_DISHES)] = 0.0
    RE[COPY_TO:COPY_TO + COPIES] = RE[:COPIES]
    cats[COPY_TO:COPY_TO + COPIES] = cats[:COPIES]


@functools.lru_cache(maxsize=None)
def width_recipe(E):
    """Exact tables at U = 24, I = 700 with the empty-mask and copied dishes, the rank queries (every user x 40 held-out dishes,
    among them the three empty-mask dishes and the copied pair 7 / 657), 30 random exclusions per query plus the held-out dish
    itself and the empty-mask dishes next below and next above it, and the per-user lists of the top-k cases."""
    rng = np.random.default_rng(7000 + E)
    U, I = WIDTH_U, WIDTH_I
    r = types.SimpleNamespace(E=E, U=U, I=I, coef=COEF)
    r.PM, r.RE, r.CE, r.cats = exact_tables(rng, U, I, E)
    _catalogue_edits(r.RE, r.cats)
    r.S = score_matrix(r.PM, r.RE, r.CE, r.cats)
    r.pos = positions(r.S)
    empt = np.flatnonzero(r.cats.sum(1) == 0)
    r.q_users = np.repeat(np.arange(U), WIDTH_HELD)
    items, excl = [], []
    for u in range(U):
        held = list(EMPTY_DISHES) + [7, COPY_TO + 7] + rng.integers(0, I, WIDTH_HELD - 5).tolist()
        for p in held:
            x = rng.choice(I, 30, replace=False).tolist() + [p]
            x += empt[empt < p][-1:].tolist() + empt[empt > p][:1].tolist()
            excl.append(x)
        items += held
    r.q_items = np.asarray(items)
    r.q_excl = excl
    r.q_off, r.q_ids = lists_csr(excl)
    r.rank0 = ranks_excluding(r.pos, r.q_users, r.q_items)
    r.rank1 = ranks_excluding(r.pos, r.q_users, r.q_items, r.q_off, r.q_ids)
    r.lists = [host_topk(r.S[u], 64, [])[:OWN_CYCLE[u % len(OWN_CYCLE)]].tolist() + rng.choice(I, 30, replace=False).tolist()
               for u in range(U)]
    for a in (r.PM, r.RE, r.CE, r.cats, r.S, r.pos, r.rank0, r.rank1):
        a.setflags(write=False)
    return r


def width_ks(E):
    return (1, 10, 16) if E == 128 else (1, 16)


# ---- 2. / 3. launch edges ------------------------------------------------------------------------------------------------------------
LAUNCH_U, LAUNCH_I = 32, 600
LAUNCH_EMPTY = (5, 300, 500, 599)                           # two of them past the first 256-dish block
VARIANTS = 4                                                # exclusion sets per user in the calls whose users repeat


@functools.lru_cache(maxsize=None)
def launch_recipe(E):
    """The small tables of the launch-edge cases: exact recipe, U = 32, I = 600, four empty-mask dishes; S [U, I] float64, pos."""
    rng = np.random.default_rng(9000 + E)
    r = types.SimpleNamespace(E=E, U=LAUNCH_U, I=LAUNCH_I, coef=COEF)
    r.PM, r.RE, r.CE, r.cats = exact_tables(rng, r.U, r.I, E)
    r.cats[list(LAUNCH_EMPTY)] = 0.0
    r.S = score_matrix(r.PM, r.RE, r.CE, r.cats)
    r.pos = positions(r.S)
    for a in (r.PM, r.RE, r.CE, r.cats, r.S, r.pos):
        a.setflags(write=False)
    return r


def user_sets(r, size, seed=0):
    """One fixed exclusion set per user: `size` ids, among them the user's own best one, an empty-mask dish and -- where size
    allows -- dishes of its top 8.  Returns (offsets, ids)."""
    rng = np.random.default_rng(seed + 31 * r.E + size)
    out = []
    for u in range(r.U):
        own = host_topk(r.S[u], 8, [])
        x = [int(own[0]), LAUNCH_EMPTY[u % len(LAUNCH_EMPTY)]] + own[2:2 + max(0, (size - 2) // 2)].tolist()
        pool = np.setdiff1d(np.arange(r.I), x)
        x += rng.choice(pool, size - len(x), replace=False).tolist()
        out.append(x[:size])
    return lists_csr(out)


def random_queries(r, n, seed):
    """n queries in random order with repeats"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, r.U, n), rng.integers(0, r.I, n)


def rank_nsplit(E, n, num_cu):
    """m2d_launch_catalogue_rank's share count"""
    want = 32 * num_cu
    ns = -(-want // -(-n // 64)) if E <= 128 else -(-(want * 4) // n)
    return min(512, max(1, ns))


def excl_nsplit(E, live, num_cu):
    """excl_shape (m2d_catalogue_excl.hip) for `live` records with users"""
    want = 32 * num_cu * (1 if E <= 128 else 4)
    units = -(-live // 64) if E <= 128 else live
    return min(512, max(1, -(-want // units)))


def share_counts(E, num_cu):
    """{intended nsplit: n (queries / tier-2 users)} -- the same counts serve both launchers"""
    if E <= 128:
        return {1: 64 * 32 * num_cu, 2: 64 * 32 * num_cu - 64, 3: 64 * 11 * num_cu}
    return {1: 128 * num_cu, 2: 128 * num_cu - 1, 512: min(50, 128 * num_cu // 512)}      # 50 at 200 units and more: clamped


def pattern_tiles(cats):
    """per pattern 1 .. 15: the 32-row tiles of the sorted table (rows of a pattern start at a tile boundary)"""
    pt = (np.asarray(cats) != 0).astype(np.int64) @ (1 << np.arange(4))
    rows = np.bincount(pt, minlength=16)
    return pt, (rows + 31) // 32


def last_tile_of_first_share(cats, nsplit):
    """Stand-in (c): the dishes of the last tile of share 0 when every pattern is scanned in pattern order -- share 0 holds tiles
    [0, ceil(T / nsplit)).  Rows inside a pattern taken in id order (the table orders them by norm bucket; any 32 of them serve)."""
    pt, tiles = pattern_tiles(cats)
    T = int(tiles[1:].sum())
    t = -(-T // nsplit) - 1                                   # that tile, counted over the patterns in order
    for q in range(1, 16):
        if t < tiles[q]:
            return np.flatnonzero(pt == q)[32 * t:32 * (t + 1)]
        t -= tiles[q]
    raise AssertionError("no tile")


def variant_sets(r, size, seed=0):
    """VARIANTS exclusion sets per user -> (offsets, ids) of U * VARIANTS rows, row u * VARIANTS + v"""
    rng = np.random.default_rng(seed + 17 * r.E + size)
    out = []
    for u in range(r.U):
        own = host_topk(r.S[u], 6, [])
        for v in range(VARIANTS):
            x = own[:v].tolist()                              # none, the best, the best two, the best three
            pool = np.setdiff1d(np.arange(r.I), x)
            out.append(x + rng.choice(pool, size - len(x), replace=False).tolist())
    return lists_csr(out)


@functools.lru_cache(maxsize=None)
def variant_lists(E, size, k):
    """(offsets, ids, want [U * VARIANTS, k]) of variant_sets: the expected list of every (user, exclusion set)"""
    r = launch_recipe(E)
    off, ids = variant_sets(r, size)
    lists = [ids[off[j]:off[j + 1]] for j in range(r.U * VARIANTS)]
    want = topk_lists(r.S, np.repeat(np.arange(r.U), VARIANTS), k, lists)
    want.setflags(write=False)
    return off, ids, want


def xs_segments(r, seed=3):
    """The EXCL_XS case: 64 users (ids repeat past 32) whose segment lengths cycle through 0, 1, 59, 60, 61, 200.  Each segment
    holds the user's own best min(20, length) dishes; the rest are ids BELOW the largest of those, so that the segment's last
    position -- the one a lookup that stops at 60 would miss at length 61 -- is a dish of the user's own top."""
    rng = np.random.default_rng(seed + r.E)
    users = np.arange(64) % r.U
    lens = np.asarray((0, 1, EXCL_XS - 1, EXCL_XS, EXCL_XS + 1, 200))[np.arange(64) % 6]
    out = []
    for u, n in zip(users, lens):
        own = host_topk(r.S[u], 20, [])[:n]
        pool = np.setdiff1d(np.arange(int(own.max()) if n else 0), own)
        if pool.size < n - own.size:
            pool = np.setdiff1d(np.arange(r.I), own)
        out.append(own.tolist() + rng.choice(pool, n - own.size, replace=False).tolist())
    return users, lens, out


def boundary_sets(r, k=10, K1=16, seed=5):
    """Tier 1's exact boundary: 64 users (ids repeat), position 2 i excludes K1 - k of its own unfiltered top K1 (k survive: not
    short), position 2 i + 1 one more (short); each also 10 ids outside its top K1."""
    rng = np.random.default_rng(seed + r.E)
    users = np.arange(64) % r.U
    out = []
    for j, u in enumerate(users):
        top = host_topk(r.S[u], K1, [])
        drop = rng.choice(top, K1 - k + (j & 1), replace=False).tolist()
        out.append(drop + rng.choice(np.setdiff1d(np.arange(r.I), top), 10, replace=False).tolist())
    return users, out


def survivors(r, users, lists, K1=16):
    """dishes of each user's float64 top K1 that its list leaves"""
    return np.asarray([np.setdiff1d(host_topk(r.S[u], K1, []), x).size for u, x in zip(users, lists)])


def odd_one_sets(r, odd_short, odd_at, k=10, K1=16, n=65, seed=6):
    """65 users of which exactly one (at position odd_at) is short (`odd_short`) / is the only one that is not"""
    rng = np.random.default_rng(seed + r.E + odd_at + 2 * odd_short)
    users = (np.arange(n) * 7) % r.U
    out = []
    for j, u in enumerate(users):
        top = host_topk(r.S[u], K1, [])
        short = odd_short == (j == odd_at)
        cut = int(rng.integers(K1 - k + 1, K1 + 1)) if short else int(rng.integers(0, K1 - k + 1))
        out.append(rng.choice(top, cut, replace=False).tolist() + rng.choice(np.setdiff1d(np.arange(r.I), top), 5, replace=False).tolist())
    return users, out


def too_few_sets(r, left=7):
    """Per user every masked dish but `left` of them, and two empty-mask dishes: k + |X| exceeds the rows of every pattern, fewer
    than k = 16 masked dishes remain, the list ends in the two remaining empty-mask dishes and then -1 / NaN."""
    masked = np.flatnonzero(r.cats.sum(1) > 0)
    users = np.arange(16) % r.U
    out = []
    for j in range(users.size):
        keep = masked[(np.arange(left) * 37 + 11 * j) % masked.size]
        out.append(np.setdiff1d(masked, keep).tolist() + [LAUNCH_EMPTY[j % 4], LAUNCH_EMPTY[(j + 1) % 4]])
    return users, out


# ---- stand-ins: what a subtly wrong kernel would return ------------------------------------------------------------------------------
def standin_no_last_column(r):
    """(a) the low-level product without its last float4 column"""
    RE = r.RE.copy()
    RE[:, r.E - 4:] = 0.0
    return score_matrix(r.PM, RE, r.CE, r.cats)


def standin_stride_E(r):
    """(b) the padded table's rows read at stride E instead of ew: row d then holds floats [d E, d E + E) of the [I, ew] table
    (rows in id order here; the table's own order moves which wrong values a row gets, not that it gets them)"""
    ew = row_width(r.E)
    flat = np.zeros((r.I + 1, ew), np.float32)
    flat[:r.I, :r.E] = r.RE
    flat = flat.reshape(-1)
    RE = np.stack([flat[d * r.E:(d + 1) * r.E] for d in range(r.I)])
    return score_matrix(r.PM, RE, r.CE, r.cats)


def changed_share(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float((a != b).reshape(len(a), -1).any(axis=1).mean())
