"""Recipes, the numpy restatement and the stand-ins of the market-retrieval tests (tests/test_market_cases_cpu.py,
tests/test_gpu_market.py): m2d_set_recipes / m2d_cookable_dishes, the cookable-dish filter, and its composition with the slate.

The restatement is a plain loop over the CSR: a dish is cookable iff its list is non-empty and at most max_missing of its ENTRIES --
every occurrence counted -- name an id that is not in the market.  Nothing here imports the engine.  Recipes are computed once and
shared (lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

import seen_dish_cases as sd

# the kernel's constants, restated (tests/test_market_cases_cpu.py holds each against its source line)
DW = 64             # m2d_market.hip: constexpr int MK_DW = 64 (dishes per wave, one per lane)
WAVES = 4           # m2d_market.hip: constexpr int MK_WAVES = 4
DB = DW * WAVES     # m2d_market.hip: constexpr int MK_DB = MK_DW * MK_WAVES (dishes per block)
EB = 64             # m2d_market.hip: constexpr int MK_EB = 64 (entries per batch)
LB = 1 << 16        # m2d_market.hip: constexpr int MK_LDS_BITS = 1 << 16 (the bitmap is staged in LDS up to this many bits)

FLAG_LDS, FLAG_L2 = "m2d_market_flag_lds", "m2d_market_flag_l2"
CATALOGUES = (1, DW - 1, DW, DW + 1, DB - 1, DB, DB + 1, 3 * DB + 5)
LONG_LISTS = (EB - 1, EB, EB + 1, 3 * EB + 1)               # the last two need a second batch, the last one four
BITMAP_ROWS = (1, 31, 32, 33, 64, 65, LB, LB + 1)
MARKETS = ("empty", "first", "last", "all", "all twice reversed", "every second")
CAT_R = 100                                                 # ingredient ids of the catalogue cases: even ones are at the market


def _frozen(r):
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def restate(off, ids, R, market, max_missing, standin=None):
    """(cookable ids int32 ascending, missing int32[I]) -- missing[d] = entries of dish d not in the market, -1 for an empty list.
    Market ids outside [0, R) contribute nothing.  `standin`: what a subtly wrong kernel would return instead --
      "drop_last_long"   the last entry of every list longer than EB is not looked at (a batch loop that stops one short);
      "bit31"            bitmap bit 32 w + 31 reads as absent (a shift that loses the top bit of a word);
      "empty_cookable"   an empty list counts as cookable (0 missing entries <= max_missing);
      "descending"       the kept ids of each block of DB dishes are written in descending order."""
    off, ids = np.asarray(off, np.int64), np.asarray(ids, np.int64)
    present = np.zeros(R, bool)
    m = np.asarray(market, np.int64).reshape(-1)
    present[m[(m >= 0) & (m < R)]] = True
    if standin == "bit31":
        present[31::32] = False
    I = len(off) - 1
    missing = np.empty(I, np.int32)
    for d in range(I):
        seg = ids[off[d]:off[d + 1]]
        if standin == "drop_last_long" and seg.size > EB:
            seg = seg[:-1]
        missing[d] = -1 if seg.size == 0 else int((~present[seg]).sum())
    keep = (missing >= 0) & (missing <= max_missing)
    if standin == "empty_cookable":
        keep |= missing < 0
    out = np.flatnonzero(keep).astype(np.int32)
    if standin == "descending":
        out = np.concatenate([out[out // DB == b][::-1] for b in np.unique(out // DB)]).astype(np.int32) if out.size else out
    return out, missing


def same_answer(a, b):
    """the GPU file's comparison: ids, count and missing counts as integers"""
    return len(a[0]) == len(b[0]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def market_ids(name, R):
    if name == "empty":
        return np.zeros(0, np.int32)
    if name == "first":
        return np.asarray([0], np.int32)
    if name == "last":
        return np.asarray([R - 1], np.int32)
    if name == "all":
        return np.arange(R, dtype=np.int32)
    if name == "all twice reversed":
        return np.concatenate([np.arange(R), np.arange(R)])[::-1].astype(np.int32)
    if name == "every second":
        return np.arange(1, R, 2, dtype=np.int32)            # 1, 3, ..., 31, ...: bit 31 of every word is set, bit 0 is not
    raise KeyError(name)


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(l) for l in lists], out=off[1:])
    ids = np.asarray([v for l in lists for v in l], np.int32)
    return off, ids


# ---- catalogue edges ------------------------------------------------------------------------------------------------------------------
def fixed_lengths(n_dishes):
    """{dish: list length} of derived_table_cases' fixed opening layout at this kernel's constants, cut to n_dishes: an empty first dish,
    an empty last dish of wave 0, wave 1 all empty, lists of EB - 1 / EB / EB + 1 / 3 EB + 1 entries opening wave 2, whose last dish is
    empty too, and an empty last dish"""
    fixed = {0: 0, DW - 1: 0, 3 * DW - 1: 0}
    fixed.update({d: 0 for d in range(DW, 2 * DW)})
    fixed.update({2 * DW + j: n for j, n in enumerate(LONG_LISTS)})
    fixed = {d: n for d, n in fixed.items() if d < n_dishes}
    fixed[n_dishes - 1] = 0
    return fixed


@functools.lru_cache(maxsize=None)
def catalogue_recipe(n_dishes):
    """fixed_lengths, every other list 1 - 12 entries, ids in [0, CAT_R); the market is the even ids.  A list holds 0 - 3 odd (absent)
    entries, the long lists one: their LAST entry, so a batch loop that stops short of it counts 0 instead of 1."""
    rng = np.random.default_rng(31000 + n_dishes)
    fixed = fixed_lengths(n_dishes)
    even, odd = np.arange(0, CAT_R, 2), np.arange(1, CAT_R, 2)
    lists = []
    for d in range(n_dishes):
        n = fixed.get(d, int(rng.integers(1, 13)))
        if n > 12:
            lists.append(list(rng.choice(even, n - 1)) + [int(rng.choice(odd))])
            continue
        bad = min(n, int(rng.choice([0, 0, 0, 1, 2, 3])))
        lists.append(list(rng.permutation(np.concatenate([rng.choice(odd, bad), rng.choice(even, n - bad)]).astype(np.int64))))
    r = types.SimpleNamespace(I=n_dishes, R=CAT_R, market=even.astype(np.int32), longest=max(map(len, lists)))
    r.off, r.ids = _csr(lists)
    return _frozen(r)


# ---- bitmap edges ---------------------------------------------------------------------------------------------------------------------
BITMAP_DISHES = 300


@functools.lru_cache(maxsize=None)
def bitmap_recipe(R):
    """300 dishes whose lists name ids 0, 31, 32 and R - 1 (those below R) only: 1 - 3 entries, every tenth dish empty; each named id
    opens a list of its own among the first dishes"""
    rng = np.random.default_rng(32000 + R % 9973)
    named = np.unique([i for i in (0, 31, 32, R - 1) if i < R])
    lists = [[int(i)] for i in named]
    for d in range(len(lists), BITMAP_DISHES):
        lists.append([] if d % 10 == 9 else [int(v) for v in rng.choice(named, int(rng.integers(1, 4)))])
    r = types.SimpleNamespace(I=BITMAP_DISHES, R=R, named=named)
    r.off, r.ids = _csr(lists)
    return _frozen(r)


def bit31_is_aimed(R, market):
    """the market holds an id 32 w + 31 that a list names"""
    m = np.asarray(market)
    return any(i % 32 == 31 and (m == i).any() for i in (31, R - 1) if 0 <= i < R)


# ---- tolerance, extremes ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tolerance_recipe():
    """40 dishes over 10 ingredients, market 0 .. 4: dish 5 lists the absent id 7 twice (cookable at 2, not at 1), dish 6 lists it once
    beside a present one, dish 7 is all present, dish 8 all absent with 5 entries, dish 9 empty; the rest random, 1 - 5 entries"""
    rng = np.random.default_rng(33000)
    lists = [[int(v) for v in rng.integers(0, 10, int(rng.integers(1, 6)))] for _ in range(40)]
    lists[5], lists[6], lists[7], lists[8], lists[9] = [7, 7], [7, 1], [0, 1, 2], [5, 6, 7, 8, 9], []
    r = types.SimpleNamespace(I=40, R=10, market=np.arange(5, dtype=np.int32), longest=5)
    r.off, r.ids = _csr(lists)
    return _frozen(r)


@functools.lru_cache(maxsize=None)
def extreme_recipe(which):
    """R = 8, the market is {0 .. 3}; an absent list is [7].
      "none"        3 DB + 5 dishes, every list names an absent id: count = 0;
      "every"       2 DB + 7 dishes, every list present: count = I;
      "hollow"      3 DB dishes: block 1 has no kept dish, blocks 0 and 2 have some;
      "last wave"   2 DB dishes: kept dishes only in the last wave of the last block"""
    rng = np.random.default_rng(34000)
    good = lambda: [int(v) for v in rng.integers(0, 4, int(rng.integers(1, 4)))]
    n = {"none": 3 * DB + 5, "every": 2 * DB + 7, "hollow": 3 * DB, "last wave": 2 * DB}[which]
    if which == "none":
        lists = [good() + [7] for _ in range(n)]
    elif which == "every":
        lists = [good() for _ in range(n)]
    elif which == "hollow":
        lists = [[7] if DB <= d < 2 * DB or d % 3 == 0 else good() for d in range(n)]
    else:
        lists = [good() if d >= n - DW and d % 2 else [7] for d in range(n)]
    r = types.SimpleNamespace(I=n, R=8, market=np.arange(4, dtype=np.int32))
    r.off, r.ids = _csr(lists)
    return _frozen(r)


# ---- the composed call: slate_cases.exact_recipe's 600 dishes ---------------------------------------------------------------------------------
COMPOSED_R = 50
RARE = COMPOSED_R - 1                                       # named by SEVEN dishes alone, as their whole list
SEVEN = (3, 77, 150, 299, 301, 450, 598)                   # none of seen_dish_cases.LAUNCH_EMPTY: those are cookable at the main market
COMPOSED_MARKET = tuple(range(25))


@functools.lru_cache(maxsize=None)
def composed_recipe():
    """Recipe lists for the I = 600 dishes of slate_cases.exact_recipe(E) (they do not depend on E), ids 0 .. 48 in lists of 1 - 8 and
    every 50th dish empty; at the market 0 .. 24 some 60 % of the lists are whole, the four empty-mask dishes' among them.  Seven
    dishes list the rare id 49 and nothing else, and nobody else lists it: the market {49} makes exactly those cookable."""
    I = 600
    rng = np.random.default_rng(35000)
    lists = []
    for d in range(I):
        n = int(rng.integers(1, 9))
        if d in sd.LAUNCH_EMPTY or rng.random() < 0.6:
            lists.append([int(v) for v in rng.integers(0, 25, n)])
        else:
            lists.append([int(v) for v in rng.permutation(np.concatenate([rng.integers(25, RARE, 1), rng.integers(0, RARE, n - 1)]))])
        if d % 50 == 49 and d not in sd.LAUNCH_EMPTY:
            lists[-1] = []
    for d in SEVEN:
        lists[d] = [RARE]
    r = types.SimpleNamespace(I=I, R=COMPOSED_R, market=np.asarray(COMPOSED_MARKET, np.int32), market7=np.asarray([RARE], np.int32))
    r.off, r.ids = _csr(lists)
    r.lists = {str(d): l for d, l in enumerate(lists) if l}              # the dict form Model.set_recipes takes
    r.cookable = restate(r.off, r.ids, r.R, r.market, 0)[0]
    r.cookable7 = restate(r.off, r.ids, r.R, r.market7, 0)[0]
    return _frozen(r)
