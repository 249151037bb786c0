"""Inputs, references, launcher rules and stand-ins of the dense-retrieval tests (tests/test_dense_topk_cases_cpu.py,
tests/test_gpu_dense_topk.py): the kernels of foodrec_amd/csrc/m2d_catalogue_dense.hip behind m2d_topk_users -- m2d_build_dish_vectors,
m2d_topk_mfma<NB, WAVES, KR>, m2d_topk_generic -- with the plain merge of dish ranges and m2d_topk_fill_absent.

Everything here is the oracle's, in float64: the tables of a recipe, the score of every (user, dish), the whole ranking of
oracle.topk_catalogue's rule (score descending, equal scores to the lower id, NaN last in id order), the launcher's rules restated on
the host, and the comparisons the GPU file applies.  The exact recipes follow seen_dish_cases.exact_tables / launch_recipe -- entries
n / 16, blend 0.5, U = 32, I = 600, seen_dish_cases.masks over the allowed patterns -- but draw their tables in _tables below, not through
exact_tables: that function is C = 4 and signed only, and these recipes need any C, weighted masks, positive Recipe_Embedding /
Category_Embedding (users whose every score is negative), copied dishes and empty masks placed by range boundary.  Nothing here imports
the engine.  Recipes and references are computed once and shared (lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

import derived_table_cases as dt
import seen_dish_cases as sd
import slate_cases as sc

MFMA, GENERIC, GROUPED = "m2d_topk_mfma", "m2d_topk_generic", "m2d_topk_grouped"
COEF = sd.COEF
U, I = sd.LAUNCH_U, sd.LAUNCH_I                              # 32 users, 600 dishes: 19 tiles, the last one of 24 dishes
TILE = 32                                                   # dishes of a tile (m2d_topk_mfma: "Dish tiles of 32 rows")


# ---- the launcher's rules, restated (m2d_catalogue_dense.hip; the CPU file holds each against its source line) -----------------------
def mfma_form(C, E, k):
    """(NB, WAVES, KR) of m2d_topk_dense_launch's dispatch -- M2D_TOPK(20, 8) M2D_TOPK(40, 8) M2D_TOPK(80, 4), lds_lists = k > 16 ->
    launch_mfma<NBV, 2, 0>, k <= 10 ? <NBV, WV, 10> : <NBV, WV, 16> -- or None where m2d_topk_generic serves"""
    K = (C + 1) * E
    if K % 8 or K // 8 not in (20, 40, 80):
        return None
    NB = K // 8
    if k > 16:
        return NB, 2, 0
    return NB, 4 if NB == 80 else 8, 10 if k <= 10 else 16


def users_per_block(form):
    """launch_mfma: ublocks = (a.nU + 32 * WAVES - 1) / (32 * WAVES)"""
    return 32 * form[1]


def tiles(n_dishes):
    """m2d_topk_dense_launch: a.tiles = (h->I + 31) / 32"""
    return (n_dishes + TILE - 1) // TILE


def per_range(n_tiles, nsplit):
    """m2d_topk_mfma: per = (p.tiles + p.nsplit - 1) / p.nsplit"""
    return (n_tiles + nsplit - 1) // nsplit


def forced_nsplit(variant):
    """launch_mfma's test hook: variant >= 100 forces variant - 100 dish ranges, 1 .. 64"""
    return min(64, max(1, variant - 100))


def auto_nsplit(nU, n_dishes, form, num_cu):
    """launch_mfma: fewer than 2 num_cu user blocks -> ceil(2 num_cu / ublocks) dish ranges, at most 64 and at most tiles / 8"""
    ublocks = -(-nU // users_per_block(form))
    want = 2 * num_cu
    if ublocks >= want:
        return 1
    return min(-(-want // ublocks), 64, max(1, tiles(n_dishes) // 8))


def dish_ranges(n_dishes, nsplit):
    """[(first dish, one past the last)] of every range; (n, n) for a range that holds no tile"""
    T = tiles(n_dishes)
    per = per_range(T, nsplit)
    out = []
    for s in range(nsplit):
        t_begin = min(T, s * per)
        t_end = min(T, t_begin + per)
        out.append((min(n_dishes, t_begin * TILE), min(n_dishes, t_end * TILE)))
    return out


def range_of(n_dishes, nsplit):
    """the range index of every dish"""
    return np.arange(n_dishes) // (per_range(tiles(n_dishes), nsplit) * TILE)


# ---- exact tables ----------------------------------------------------------------------------------------------------------------------
MFMA_SHAPES = ((4, 32), (4, 64), (4, 128), (3, 40), (7, 40), (3, 160))       # (C, E): NB = 20, 40, 80, 20, 40, 80
GENERIC_SHAPES = tuple((4, E) for E in (4, 12, 20, 48, 100, 132, 200, 256, 260)) + ((3, 8), (6, 20))
KS = (1, 10, 11, 16, 17, 64)
WEIGHT_ROWS = ((2, 0, 0, 0), (.5, .5, 0, 0), (1, 1, 2, 0), (.5, .5, 1, 2), (1.5, 0, .5, 0))   # dyadic weights, every sum a power of two
NEGATIVE_USERS, ZERO_USERS = (0, 1, 2, 3), (4, 5, 6, 7)
# dishes with an empty mask: both half-lanes ((d >> 2) & 1 = 0 and 1) of the first tile and of the last, partial one, and the two dishes
# next to the range boundaries 96 (7 and 8 ranges), 224 (3 ranges) and 320 (2 ranges)
EMPTY = (2, 5, 95, 96, 223, 224, 319, 320, 593, 599)
# copied dishes (from, to, count): exact ties for every user.  0 .. 49 -> 541 .. 590: ids that differ by 1 mod 4 (another wave of
# m2d_topk_generic), the first tile against the last three; 100 .. 119 -> 400 .. 419: ids equal mod 4 (the same wave); 318 -> 321: a pair
# that straddles dish 320
COPIES = ((0, 541, 50), (100, 400, 20), (318, 321, 1))
RANGE_COUNTS = (1, 2, 3, 7, 8, 19, 20, 64)
RANGE_KS = (10, 16, 64)
RANGE_KS_33 = (10, 16, 33)                                  # I = 33: m2d_topk_users takes k <= I, so the whole catalogue stands for 64
PREFIXES = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257)
SMALL_CATALOGUES = (1, 2, 3, 5)
SHORT_I, SHORT_CUT = 70, 14
SHORT_EMPTY = (0, 3, 4, 9, 13, 20, 31, 32, 63, 69)          # five inside the cut of 14 dishes, one each side of tiles 0 | 1 and 1 | 2


def patterns(C):
    """the 0/1 masks whose popcount is a power of two (sd.EXACT_PATTERNS at C = 4): no division by 3, 5, 6 or 7"""
    return tuple(p for p in range(1, 2 ** C) if bin(p).count("1") in (1, 2, 4))


def weight_rows(C):
    """WEIGHT_ROWS at C categories: rows cut to C columns where what is cut is 0, zero columns added"""
    rows = [r[:C] for r in WEIGHT_ROWS if not any(r[C:])]
    return np.asarray([tuple(r) + (0,) * (C - len(r)) for r in rows], np.float32)


def _masks(rng, n, C, weighted):
    if not weighted:
        return sd.masks(rng, n, C, allowed=list(patterns(C)))
    rows = weight_rows(C)[rng.integers(0, len(weight_rows(C)), n)]
    return np.stack([row[rng.permutation(C)] for row in rows])      # any order of a row's weights: the sum stays


def _freeze(r):
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def _tables(rng, n_users, n_dishes, C, E, weighted, empty):
    """Entries n / 16: Personal_Memory in -16 .. 16, Recipe_Embedding and Category_Embedding in 1 .. 16 (positive, so that a user
    whose rows are negative scores below 0 on every dish); users 0 .. 3 negative rows, users 4 .. 7 zero rows"""
    f = lambda shape, lo: (rng.integers(lo, 17, shape) / 16.0).astype(np.float32)      # noqa: E731
    PM, RE, CE = f((n_users, C + 1, E), -16), f((n_dishes, E), 1), f((C, E), 1)
    PM[list(NEGATIVE_USERS)] = -f((len(NEGATIVE_USERS), C + 1, E), 1)
    PM[list(ZERO_USERS)] = 0.0
    cats = _masks(rng, n_dishes, C, weighted)
    for src, dst, n in COPIES:
        if dst + n <= n_dishes:
            RE[dst:dst + n] = RE[src:src + n]
            cats[dst:dst + n] = cats[src:src + n]
    cats[[d for d in empty if d < n_dishes]] = 0.0
    return PM, RE, CE, cats


def score_matrix(r, dtype=np.float64):
    """[U, I] oracle.inference (oracle.inference_ingredients where the recipe has an ingredient table) of every user on every dish"""
    if r.ing is None:
        return sd.score_matrix(r.PM, r.RE, r.CE, r.cats, r.coef, dtype)
    from oracle import m2d_oracle as oracle
    dd = np.tile(np.arange(r.I), 8)
    out = [oracle.inference_ingredients(r.PM, r.RE, *r.ing, np.repeat(np.arange(u0, u0 + 8), r.I), dd, r.cats[dd], r.coef, dtype)
           for u0 in range(0, r.U, 8)]
    return np.concatenate(out).reshape(r.U, r.I)


def dish_vectors(r, dtype=np.float64):
    """oracle.dish_vectors; with an ingredient table the first E columns are a H[d] (dish_vector_row: o[e] = a * hv[d * E + e])"""
    from oracle import m2d_oracle as oracle
    with np.errstate(invalid="ignore", divide="ignore"):
        Dt = oracle.dish_vectors(r.RE, r.CE, r.cats, r.coef, dtype)
        if r.ing is not None:
            Dt[:, :r.E] = dtype(oracle.blend_coefficients(r.coef)[0]) * oracle.dish_high_vectors(*r.ing, dtype=dtype)
    return Dt


@functools.lru_cache(maxsize=None)
def exact_recipe(C, E, weighted=False, ing=False):
    """Exact tables at U = 32, I = 600 for any (C, E): 0/1 masks from patterns(C) or rows of weight_rows(C), the EMPTY dishes, the
    COPIES, four negative and four all-zero users; `ing`: derived_table_cases' exact ingredient lists (rows n / 16 in 1 .. 16, list
    lengths and weight totals powers of two; a dish with an empty list scores NaN too).  S [U, I] float64: every value a float32."""
    rng = np.random.default_rng(31000 + 1000 * C + E + (500 if weighted else 0) + (250 if ing else 0))
    r = types.SimpleNamespace(C=C, E=E, U=U, I=I, coef=COEF, weighted=weighted, ing=None)
    r.PM, r.RE, r.CE, r.cats = _tables(rng, U, I, C, E, weighted, EMPTY)
    if ing:
        ING = (rng.integers(1, 17, (dt.R, E)) / 16.0).astype(np.float32)
        off, ids, w = dt.ingredient_lists(rng, I, dt.R, weighted=True)
        for a in (ING, off, ids, w):
            a.setflags(write=False)
        r.ing = (ING, off, ids, w)
    r.S = score_matrix(r)
    return _freeze(r)


@functools.lru_cache(maxsize=None)
def short_recipe(E):
    """I = 70 with ten empty-mask dishes (five of them among the first 14): lists longer than the rankable dishes"""
    rng = np.random.default_rng(33000 + E)
    r = types.SimpleNamespace(C=4, E=E, U=U, I=SHORT_I, coef=COEF, weighted=False, ing=None)
    r.PM, r.RE, r.CE, r.cats = _tables(rng, U, SHORT_I, 4, E, False, SHORT_EMPTY)
    r.S = score_matrix(r)
    return _freeze(r)


@functools.lru_cache(maxsize=None)
def remasked_recipe(E):
    """exact_recipe(4, E) under the masks of its weighted sibling (set_dish_categories a second time) and its reference"""
    base = exact_recipe(4, E)
    r = types.SimpleNamespace(**vars(base))
    r.cats, r.weighted = exact_recipe(4, E, True).cats, True
    r.S = score_matrix(r)
    return _freeze(r)


def call_users(n, seed=0, n_users=U):
    """n user ids: every user in a shuffled order, then repeats (n < U: a shuffled part)"""
    rng = np.random.default_rng(35000 + seed + n)
    return np.concatenate([rng.permutation(n_users), rng.integers(0, n_users, max(0, n - n_users))])[:n].astype(np.int32)


def lists(S, users, k, n_dishes=None, order=None):
    """(scores [n, k] float64, ids [n, k]) of the oracle's ranking over dishes 0 .. n_dishes - 1 for the rows S[users]"""
    n_dishes = S.shape[1] if n_dishes is None else n_dishes
    rows = S[np.asarray(users, np.int64)][:, :n_dishes]
    if order is None:
        return sc.exact_lists(rows, np.arange(n_dishes), k)
    ss, ii = [], []
    for row in rows:
        o = order(row)[:k]
        ss.append(row[o])
        ii.append(o)
    return np.asarray(ss), np.asarray(ii)


def assert_lists(got_s, got_i, want_s, want_i, what=""):
    """the ids as integers, the scores as float32 words (-0 folded onto +0), NaN where the reference is NaN"""
    got_s, got_i, want_s, want_i = np.asarray(got_s), np.asarray(got_i, np.int64), np.asarray(want_s), np.asarray(want_i, np.int64)
    assert got_i.shape == want_i.shape and got_s.shape == want_s.shape, (what, got_i.shape, want_i.shape)
    bad = (got_i != want_i).any(1)
    assert not bad.any(), "%s: the ids of %d of %d lists differ, first at row %d: %s vs %s" % (
        what, int(bad.sum()), bad.size, int(bad.argmax()), got_i[bad.argmax()], want_i[bad.argmax()])
    nan = np.isnan(want_s)
    assert np.array_equal(np.isnan(got_s), nan), "%s: NaN positions differ" % what
    g, w = sc.bits(np.where(nan, 0, got_s)), sc.bits(np.where(nan, 0, want_s))
    assert np.array_equal(g, w), "%s: %d of %d score words differ" % (what, int((g != w).sum()), g.size)


def assert_whole_lists(got_i, n_dishes, what=""):
    """no -1 left, every id a dish, none twice"""
    got_i = np.asarray(got_i)
    assert (got_i >= 0).all() and (got_i < n_dishes).all(), "%s: an id outside the catalogue: %s" % (what, got_i[(got_i < 0) | (got_i >= n_dishes)][:8])
    assert all(len(set(row.tolist())) == row.size for row in got_i), "%s: an id is listed twice" % what


def cross_range_ties(S, users, k, n_dishes, nsplit):
    """lists in which two neighbouring entries hold the same score and lie in different dish ranges"""
    s, i = lists(S, users, k, n_dishes)
    rg = range_of(n_dishes, nsplit)[i]
    with np.errstate(invalid="ignore"):
        return int(((s[:, :-1] == s[:, 1:]) & (rg[:, :-1] != rg[:, 1:])).any(1).sum())


# ---- normal tables -----------------------------------------------------------------------------------------------------------------------
NORMAL_U, NORMAL_I = 64, 300                               # 10 tiles, the last one of 12 dishes
NORMAL_EMPTY = (3, 150, 299)
NORMAL_MFMA, NORMAL_GENERIC = (32, 64, 128), (48, 200)
# {blend: k}: the k at which the reference alone leaves slate_cases.MIN_SHARP of the users sharp at every width, 0/1 and weighted
# (0.5: 0.70 .. 1.00 at k = 10; 0.99, where a score is its mask's high-level value to two digits: 0.81 .. 1.00 at k = 1, 0.00 .. 0.91
# at k = 10)
NORMAL_LISTS = {0.5: 10, 0.99: 1}


@functools.lru_cache(maxsize=None)
def normal_recipe(E, weighted, coef=COEF):
    """Normal tables (N(0, 1 / E)) at U = 64, I = 300, 0/1 masks or weights from {0, 0.5, 1, 2}, three empty-mask dishes; ref64, the
    derived bound (slate_cases.reference_and_bound: the same contraction of the same operands) and the sharp users at the blend's k
    (NORMAL_LISTS).  The tables do not depend on the blend."""
    rng = np.random.default_rng(41000 + 131 * E + int(weighted))
    r = types.SimpleNamespace(C=4, E=E, U=NORMAL_U, I=NORMAL_I, k=NORMAL_LISTS[coef], coef=coef, weighted=weighted, ing=None)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, r.U, r.I, E, 4)
    if weighted:
        r.cats = rng.choice(np.array([0, 0.5, 1, 2], np.float32), (r.I, 4))
        r.cats[r.cats.sum(1) == 0, 0] = 2.0
    else:
        r.cats = sd.masks(rng, r.I, 4)
    r.cats[list(NORMAL_EMPTY)] = 0.0
    r.users = np.arange(r.U, dtype=np.int32)
    r.dishes = np.arange(r.I)
    r.ref, r.bound = sc.reference_and_bound(r.PM, r.RE, r.CE, r.cats, coef, r.users, r.dishes)
    r.sharp = sc.sharp_users(r.ref, r.bound, r.dishes, r.k)
    return _freeze(r)


# ---- stand-ins: what a subtly wrong kernel would return --------------------------------------------------------------------------------
def _key(row):
    nan = np.isnan(row)
    return nan, -np.where(nan, -np.inf, row)


def standin_pad_rows(S, users, k, n_dishes):
    """(a) the pad rows of the last tile rank with their score 0 (ids n_dishes .. 32 tiles - 1)"""
    rows = np.zeros((len(users), tiles(n_dishes) * TILE))
    rows[:, :n_dishes] = S[np.asarray(users, np.int64)][:, :n_dishes]
    return sc.exact_lists(rows, np.arange(rows.shape[1]), k)


def standin_no_last_tile(S, users, k, n_dishes, nsplit):
    """(b) the last tile of every dish range is never scanned: its dishes are absent, and appended as such"""
    keep = np.ones(n_dishes, bool)
    for lo, hi in dish_ranges(n_dishes, nsplit):
        if hi > lo:
            keep[(tiles(hi) - 1) * TILE:hi] = False
    rows = np.where(keep[None, :], S[np.asarray(users, np.int64)][:, :n_dishes], np.nan)
    return sc.exact_lists(rows, np.arange(n_dishes), k)


def standin_tie_to_higher_range(S, users, k, n_dishes, nsplit):
    """(c) equal scores from different dish ranges go to the HIGHER range (inside a range: to the lower id)"""
    rg = range_of(n_dishes, nsplit)
    ids = np.arange(n_dishes)

    def order(row):
        nan, key = _key(row)
        return np.lexsort((ids, -rg, key, nan))
    return lists(S, users, k, n_dishes, order)


def standin_absent_descending(S, users, k, n_dishes):
    """(d) the dishes that never ranked (NaN) are appended in DESCENDING id"""
    ids = np.arange(n_dishes)

    def order(row):
        nan, key = _key(row)
        return np.lexsort((np.where(nan, -ids, ids), key, nan))
    return lists(S, users, k, n_dishes, order)


def standin_no_second_stage(r):
    """(e) NB = 80: the contraction without the second K stage of a dish tile (floats 320 .. 639 of the 640)"""
    assert (r.C + 1) * r.E == 640
    with np.errstate(invalid="ignore"):
        return r.PM.astype(np.float64).reshape(r.U, -1)[:, :320] @ dish_vectors(r)[:, :320].T


def changed_lists(a, b):
    """how many lists differ in an id"""
    return int((np.asarray(a[1]) != np.asarray(b[1])).any(1).sum())
