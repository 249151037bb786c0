"""Inputs, references and stand-ins of the derived-table tests (tests/test_derived_table_cases_cpu.py, tests/test_gpu_derived_tables.py).

Two tables the engine derives itself have no accessor: uh[u][c] = <U_high[u], CE_c> (option "user_high_table", m2d_build_user_high)
and H[d], the normalised ingredient sum (m2d_dish_high_from_ingredients).  A wrong row can only show in a score, so the recipes here
make every score an exact float32 number (seen_dish_cases.exact_tables; ingredient rows k / 16, list lengths and weight totals powers
of two) and spread 2^18 + 77 pairs over every user and dish: the GPU score must then equal the float64 restatement bit for bit, pair
by pair, whatever the order of summation.

Everything here is the oracle's; nothing imports the engine.  Recipes and references are computed once and shared (lru_cache);
callers do not write into them."""
import functools
import types

import numpy as np

import seen_dish_cases as sd

COEF = sd.COEF
WIDTHS = (4, 32, 36, 64, 68, 128, 132, 200, 256)            # every LPP in 8 / 16 / 32 / 64 full and partial; NQ 1 / 2 / 4 likewise
U, I, R = 1003, 517, 301                                    # odd: no group, wave or block count divides them
B = 2 ** 18 + 77                                            # the smallest batch that reads uh is 2^18
SLICE = 16384                                               # pairs per oracle call: no [B, 5, E] temporary
LENGTHS = (0, 1, 2, 4, 8, 16, 32, 64)
LIST_WEIGHTS = (0.5, 1.0, 2.0)
DB = 16                                                     # m2d_ingredients.hip: dishes per wave
BIG_WIDTH = {8: 4, 16: 36, 32: 68, 64: 132}                 # big_user_recipe: the partial form of each LPP
SMALL_CATALOGUES = (1, 15, 16, 17)
STANDIN_PAIRS = 2 ** 15                                     # a stand-in's share is taken over the first 2^15 pairs it touches
EXTRA_WIDTHS, EXTRA_PAIRS = (6, 260, 320), 2 ** 14 + 77     # the generic pair kernel over H; a second column block 4 / 64 columns wide
EDGE_WIDTHS = (64, 128, 200)                                # the H builder's NQ = 1, 2, 4


def lpp(E):
    """lanes per pair of the C = 4 pair kernels and of m2d_build_user_high (launch_any, m2d_ensure_user_high)"""
    E4 = E // 4
    return 8 if E4 <= 8 else 16 if E4 <= 16 else 32 if E4 <= 32 else 64


def nq(E):
    """m2d_launch_build_dish_high: columns per lane of one column block (64 NQ columns)"""
    return 1 if E <= 64 else 2 if E <= 128 else 4


def row_batch(E):
    """m2d_dish_high_from_ingredients: ingredient rows requested together (BR)"""
    return 8 if nq(E) >= 4 else 16


def uh_blocks(n_users, E, num_cu):
    """m2d_ensure_user_high's grid"""
    return min(16 * num_cu, (n_users * lpp(E) // 64 + 3) // 4 + 1)


def uh_first_trip(n_users, E, num_cu):
    """users the builder's grid-stride loop covers in its first trip: 4 waves a block, 64 / LPP users a wave"""
    return uh_blocks(n_users, E, num_cu) * 4 * (64 // lpp(E))


def reader_chunks_per_trip(num_cu, blocks_per_cu=8):
    """launch_any's cap: the pair kernels' chunk loop wraps above this many 64-pair chunks"""
    return num_cu * blocks_per_cu * 4


def _frozen(r):
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def spread_pairs(rng, n, n_users, n_items):
    """n pairs over every user and dish alike: two independent permutations of arange(n) % U and arange(n) % I"""
    return (rng.permutation(np.arange(n) % n_users).astype(np.int32), rng.permutation(np.arange(n) % n_items).astype(np.int32))


# ---- references: the oracle's restatements, a slice of pairs at a time ----------------------------------------------------------------
def pair_scores(PM, RE, CE, cats, users, items, dtype=np.float64):
    """oracle.inference on every pair, masks by dish"""
    from oracle import m2d_oracle as oracle
    out = np.empty(len(users), dtype)
    for s in range(0, len(users), SLICE):
        u, d = users[s:s + SLICE], items[s:s + SLICE]
        out[s:s + SLICE] = oracle.inference(PM, RE, CE, u, d, cats[d], COEF, dtype)
    return out


def ingredient_scores(PM, RE, cats, ING, off, ids, w, users, items, dtype=np.float64):
    """oracle.inference_ingredients on every pair, masks by dish"""
    from oracle import m2d_oracle as oracle
    out = np.empty(len(users), dtype)
    for s in range(0, len(users), SLICE):
        u, d = users[s:s + SLICE], items[s:s + SLICE]
        out[s:s + SLICE] = oracle.inference_ingredients(PM, RE, ING, off, ids, w, u, d, cats[d], COEF, dtype)
    return out


# ---- pairs over the plain tables: uh --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_recipe(E):
    """Exact tables at U = 1 003, I = 517, B = 2^18 + 77 pairs (every user at least 261 times, every dish at least 507 times), per-pair
    masks cats[items]; ref: oracle.inference in float64 on every pair."""
    rng = np.random.default_rng(11000 + E)
    r = types.SimpleNamespace(E=E, U=U, I=I, B=B, coef=COEF)
    r.PM, r.RE, r.CE, r.cats = sd.exact_tables(rng, U, I, E)
    r.users, r.items = spread_pairs(rng, B, U, I)
    r.ref = pair_scores(r.PM, r.RE, r.CE, r.cats, r.users, r.items)
    return _frozen(r)


@functools.lru_cache(maxsize=None)
def big_user_recipe(lanes, num_cu):
    """Enough users for m2d_build_user_high<lanes>'s second trip on a device of num_cu units: the first trip covers
    16 num_cu blocks x 4 waves x gpw users; the second holds three whole groups and, where a wave has several groups (gpw > 1), one
    more user -- a live group whose other users fail `u < U`.  Pairs cover every user at least twice (and reach the uh threshold).
    The reference is big_user_reference's."""
    E, gpw = BIG_WIDTH[lanes], 64 // lanes
    n_users = 16 * num_cu * 4 * gpw + 3 * gpw + (1 if gpw > 1 else 0)
    rng = np.random.default_rng(13000 + lanes)
    r = types.SimpleNamespace(E=E, U=n_users, I=I, coef=COEF, lanes=lanes, gpw=gpw, num_cu=num_cu)
    r.PM, r.RE, r.CE, r.cats = sd.exact_tables(rng, n_users, I, E)
    r.B = max(2 * n_users, B)
    r.users, r.items = spread_pairs(rng, r.B, n_users, I)
    r.first_trip = uh_first_trip(n_users, E, num_cu)
    return _frozen(r)


@functools.lru_cache(maxsize=None)
def big_user_reference(lanes, num_cu):
    r = big_user_recipe(lanes, num_cu)
    ref = pair_scores(r.PM, r.RE, r.CE, r.cats, r.users, r.items)
    ref.setflags(write=False)
    return ref


# ---- ingredient lists: H --------------------------------------------------------------------------------------------------------------
def fixed_lengths(n_dishes):
    """{dish: list length} of the fixed layout, cut to n_dishes: an empty first dish, an empty last dish of wave 0, wave 1 all empty,
    a list of 64 (8 row batches at BR = 8, 4 at 16) opening wave 2, whose last dish is empty too, and an empty last dish"""
    fixed = {0: 0, 15: 0, 32: 64, 47: 0}
    fixed.update({d: 0 for d in range(16, 32)})
    fixed = {d: n for d, n in fixed.items() if d < n_dishes}
    fixed[n_dishes - 1] = 0
    return fixed


def ingredient_lists(rng, n_dishes, n_rows, weighted, all_empty=False):
    """(offsets int32[I + 1], ids int32[nnz], weights float32[nnz] or None): fixed_lengths, then lengths drawn from LENGTHS; `weighted`:
    one weight from LIST_WEIGHTS for a whole list, so a list's total is a power of two"""
    lens = np.asarray(LENGTHS)[rng.integers(0, len(LENGTHS), n_dishes)]
    for d, n in fixed_lengths(n_dishes).items():
        lens[d] = n
    if all_empty:
        lens[:] = 0
    off = np.zeros(n_dishes + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    ids = rng.integers(0, n_rows, int(off[-1])).astype(np.int32)
    w = np.repeat(np.asarray(LIST_WEIGHTS, np.float32)[rng.integers(0, 3, n_dishes)], lens) if weighted else None
    return off, ids, w


def _ingredient_recipe(E, weighted, tables, users, items, seed, all_empty=False):
    rng = np.random.default_rng(seed)
    PM, RE, CE, cats = tables
    r = types.SimpleNamespace(E=E, U=PM.shape[0], I=RE.shape[0], R=R, B=len(users), coef=COEF, weighted=weighted,
                              PM=PM, RE=RE, CE=CE, cats=cats, users=users, items=items)
    r.ING = (rng.integers(-16, 17, (R, E)) / 16.0).astype(np.float32)
    r.off, r.ids, r.w = ingredient_lists(rng, r.I, R, weighted, all_empty)
    r.ref = ingredient_scores(PM, RE, cats, r.ING, r.off, r.ids, r.w, users, items)
    return _frozen(r)


@functools.lru_cache(maxsize=None)
def ingredient_recipe(E, weighted, pairs=B):
    """pair_recipe(E)'s tables and its first `pairs` pairs (widths outside WIDTHS: tables and pairs of their own), R = 301 ingredient
    rows of k / 16 and ingredient_lists' CSR; ref: oracle.inference_ingredients in float64 on every pair."""
    if E in WIDTHS:
        p = pair_recipe(E)
        tables, users, items = (p.PM, p.RE, p.CE, p.cats), p.users[:pairs], p.items[:pairs]
    else:
        rng = np.random.default_rng(11000 + E)
        tables = sd.exact_tables(rng, U, I, E)
        users, items = spread_pairs(rng, pairs, U, I)
    return _ingredient_recipe(E, weighted, tables, users, items, 12000 + 2 * E + int(weighted))


@functools.lru_cache(maxsize=None)
def small_catalogue_recipe(E, n_dishes, weighted=True, all_empty=False):
    """A catalogue of 1 / 15 / 16 / 17 dishes under the fixed layout cut to it (`all_empty`: any size, nnz = 0: every score NaN),
    37 users, 4 099 pairs."""
    rng = np.random.default_rng(14000 + 31 * E + n_dishes)
    tables = sd.exact_tables(rng, 37, n_dishes, E)
    users, items = spread_pairs(rng, 4099, 37, n_dishes)
    return _ingredient_recipe(E, weighted, tables, users, items, 15000 + 31 * E + n_dishes, all_empty)


def second_lists(r):
    """another CSR over the same rows for the recipe's dishes (set_ingredients a second time) and its reference"""
    rng = np.random.default_rng(16000 + r.E)
    lens = np.asarray(LENGTHS)[rng.integers(0, len(LENGTHS), r.I)]
    lens[[1, 16, 33]] = (0, 32, 0)
    off = np.zeros(r.I + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    ids = rng.integers(0, r.R, int(off[-1])).astype(np.int32)
    return off, ids, ingredient_scores(r.PM, r.RE, r.cats, r.ING, off, ids, None, r.users, r.items)


def bad_id_positions(r):
    """where test 7 puts a bad id: inside the second row batch of dish 32's list (the list opens a wave, so batches count from its first
    entry), and the last entry of the stream"""
    return int(r.off[32]) + row_batch(r.E) + 1, int(r.off[-1]) - 1


# ---- stand-ins: what a subtly wrong kernel would return -------------------------------------------------------------------------------
def _first(touched):
    return np.flatnonzero(touched)[:STANDIN_PAIRS]


def changed_share(ref, alt):
    """share of the pairs whose score differs (NaN against a number differs, NaN against NaN does not)"""
    same = (ref == alt) | (np.isnan(ref) & np.isnan(alt))
    return float(1.0 - same.mean())


def standin_uh_no_last_column(r):
    """(a) uh built without the last float4 column of U_high; touches every pair.  Returns (pairs, scores)"""
    PM = r.PM.copy()
    PM[:, 0, r.E - 4:] = 0.0
    t = _first(np.ones(r.B, bool))
    return t, pair_scores(PM, r.RE, r.CE, r.cats, r.users[t], r.items[t])


def standin_uh_no_fourth(r):
    """(b) uh[:, 3] lost: category 3 adds nothing to the high-level sum (the count n keeps it); touches the pairs with m_3 != 0"""
    CE = r.CE.copy()
    CE[3] = 0.0
    t = _first(r.cats[r.items, 3] != 0)
    return t, pair_scores(r.PM, r.RE, CE, r.cats, r.users[t], r.items[t])


def standin_uh_second_trip_zero(r):
    """(c) big_user_recipe: uh rows of the builder's second trip left at zero; touches the pairs of those users"""
    PM = r.PM.copy()
    PM[r.first_trip:, 0, :] = 0.0
    t = _first(r.users >= r.first_trip)
    return t, pair_scores(PM, r.RE, r.CE, r.cats, r.users[t], r.items[t])


def standin_h_no_last_entry(r):
    """(d) H without the last entry of every list longer than 8 (its weight gone with it); touches the pairs of those dishes"""
    lens = np.diff(r.off)
    keep = np.ones(len(r.ids), bool)
    keep[r.off[1:][lens > 8] - 1] = False
    off = np.zeros_like(r.off)
    np.cumsum(lens - (lens > 8), out=off[1:])
    t = _first((lens > 8)[r.items])
    return t, ingredient_scores(r.PM, r.RE, r.cats, r.ING, off, r.ids[keep], None if r.w is None else r.w[keep], r.users[t], r.items[t])


def standin_h_neighbour_row(r):
    """(e) an empty dish's row of H taken from its neighbour: the accumulator not cleared, so the row of the nearest dish before it
    that has a list (dish 0 has none before it and stays NaN); touches the pairs of the empty dishes"""
    lens = np.diff(r.off)
    src = np.arange(r.I)
    for d in range(r.I):
        if lens[d] == 0 and d > 0:
            src[d] = src[d - 1]
    off, ids = sd.gather_csr(r.off, r.ids, src)
    w = None if r.w is None else sd.gather_csr(r.off, r.w, src)[1]
    t = _first((lens == 0)[r.items])
    return t, ingredient_scores(r.PM, r.RE, r.cats, r.ING, off.astype(np.int32), ids, w, r.users[t], r.items[t])


def standin_h_no_last_column(r):
    """(f) H without its last float4 column; touches every pair of a dish that has a list"""
    ING = r.ING.copy()
    ING[:, r.E - 4:] = 0.0
    t = _first((np.diff(r.off) > 0)[r.items])
    return t, ingredient_scores(r.PM, r.RE, r.cats, ING, r.off, r.ids, r.w, r.users[t], r.items[t])
