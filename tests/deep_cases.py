"""Inputs, host restatements and stand-ins of the deep-list tests (tests/test_deep_cases_cpu.py, tests/test_gpu_deep.py; DESIGN.md
sections 4.11 and 8.8).

Every comparison of the two files is ids as integers and scores as 32-bit words: the order is restated here as the 64-bit key of
m2d_engine.h (tkm_key), the selection as the radix select of m2d_select.hip (digit passes, early exit, gather, fill) and the
launcher as its walk over dish ranges with a running list.  Nothing here imports the engine.  Recipes are computed once and shared
(lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

import seen_dish_cases as sd
from helpers import mlp_head

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)        # m2d_engine.h: TKM_NONE
NAN_WORD = 0x7FC00000                        # the score word of an empty slot
BITS, BINS = 11, 2048                        # m2d_select.hip: SD_BITS, SD_BINS
K_MAX = 1024
DEFAULT_P = 1 << 22
KS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024)
SIZES = (255, 256, 257, 1023, 1024, 1025, 1300, 16385)      # 16 385: past select_threads' switch to 1 024 threads
EXACT_WIDTHS = (4, 64, 200)
STANDINS = ("higher_id", "forget", "nan_first", "one_short", "strike_after")


def words(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def keys(w, ids, higher_id=False, nan_first=False):
    """tkm_key of score words `w` (uint32) and dish ids: a smaller key comes earlier.  Stand-ins: `higher_id` resolves equal scores to
    the higher id, `nan_first` ranks NaN in front of everything."""
    w = np.asarray(w, np.uint32)
    f = w.view(np.float32)
    b = np.where(f == 0, np.uint32(0), w)
    hi = np.where(b & np.uint32(0x80000000), b, ~(b | np.uint32(0x80000000)))
    hi = np.where(np.isnan(f), np.uint32(0 if nan_first else 0xFFFFFFFF), hi).astype(np.uint64)
    lo = np.asarray(ids, np.int64).astype(np.uint32)
    if higher_id:
        lo = ~lo
    return (hi << np.uint64(32)) | lo.astype(np.uint64)


def sort_select(key, k):
    """the first k of each row of `key` [n, W] by a plain sort, TKM_NONE where a row has fewer"""
    key = np.atleast_2d(key)
    out = np.full((key.shape[0], k), NONE, np.uint64)
    s = np.sort(key, axis=1)[:, :k]
    out[:, :s.shape[1]] = s
    return out


def radix_select(key, k, one_short=False, stats=None):
    """m2d_select_deep restated for a batch of rows `key` [n, W] (TKM_NONE: no entry): per pass a 2 048-bin histogram of the next 11
    bits (the last pass: 9) of the real keys that share the prefix, a scan for the bin of the k-th key, the count in front of it and
    the keys in it; the passes end when less + m == k, at 64 bits, or after the first pass when a row holds no more than k real
    keys; the gather takes the keys in front of the prefix and the first k - less that share it (arrival order), the rest of the
    list is TKM_NONE; a sort of the list.  `one_short`: the stand-in that takes one key too few of the k-th bin.  `stats`: a dict
    that receives the passes each row took."""
    key = np.atleast_2d(np.asarray(key, np.uint64))
    n, W = key.shape
    real = key != NONE
    prefix = np.zeros(n, np.uint64)
    less = np.zeros(n, np.int64)
    all_in = np.zeros(n, bool)               # no more than k real keys: all are listed
    done = np.zeros(n, bool)
    passes = np.zeros(n, np.int64)
    width = np.zeros(n, np.int64)            # bits of `prefix`
    rows = np.arange(n)
    bits = 0
    while not done.all():
        nb = min(BITS, 64 - bits)
        sh = np.uint64(64 - bits - nb)
        live = real & ~done[:, None]
        if bits:
            live &= (key >> np.uint64(64 - bits)) == prefix[:, None]
        digit = ((key >> sh) & np.uint64((1 << nb) - 1)).astype(np.int64)
        hist = np.bincount((rows[:, None] * BINS + digit)[live], minlength=n * BINS).reshape(n, BINS)
        cum = np.cumsum(hist, axis=1)
        want = k - less
        act = ~done
        passes[act] += 1
        short = act & (cum[:, -1] < want)
        assert bits == 0 or not short.any()
        all_in |= short
        done |= short
        act &= ~short
        b = (cum < want[:, None]).sum(1)                     # the first bin whose running count reaches `want`
        b = np.minimum(b, BINS - 1)
        m = hist[rows, b]
        before = cum[rows, b] - m
        less = np.where(act, less + before, less)
        prefix = np.where(act, (prefix << np.uint64(nb)) | b.astype(np.uint64), prefix)
        bits += nb
        width = np.where(act, bits, width)                  # a row that is done keeps its prefix at the width it had
        done |= act & ((less + m == k) | (bits == 64))
    if stats is not None:
        stats["passes"] = passes
    out = np.full((n, k), NONE, np.uint64)
    for r in range(n):
        kr = key[r][real[r]]
        if all_in[r]:
            got = kr
        else:
            hi = kr >> np.uint64(64 - int(width[r]))
            need = k - int(less[r]) - (1 if one_short else 0)
            got = np.concatenate([kr[hi < prefix[r]], kr[hi == prefix[r]][:need]])
        got = np.sort(got)[:k]
        out[r, :got.size] = got
    return out


def key_lists(W32, k, lists=None, ids=None):
    """(score words uint32 [n, k], ids int64 [n, k]): the first k of the key order per row of the float32 matrix `W32` [n, I] over the
    dishes `ids` (default 0 .. I - 1) less row j's lists[j]; -1 / NAN_WORD where fewer remain"""
    W32 = np.ascontiguousarray(W32, np.float32)
    n, I = W32.shape
    ids = np.arange(I) if ids is None else np.asarray(ids, np.int64)
    out_w = np.full((n, k), NAN_WORD, np.uint32)
    out_i = np.full((n, k), -1, np.int64)
    for j in range(n):
        keep = ids >= 0
        if lists is not None and len(lists[j]):
            keep &= ~np.isin(ids, np.asarray(list(lists[j]), np.int64))
        w = words(W32[j])
        o = np.argsort(keys(w[keep], ids[keep]), kind="stable")[:k]
        out_w[j, :o.size] = w[keep][o]
        out_i[j, :o.size] = ids[keep][o]
    return out_w, out_i


def ranges(I, P):
    """m2d_launch_deep_lists: (W, R) -- dish ranges of W dishes, user blocks of R rows (before the cap at nU)"""
    W = min(I, P, 65536)
    return W, max(1, P // W)


def model_lists(W32, k, lists=None, W=None, standin=None):
    """The deep call on the host: per row the catalogue in ranges of W dishes, each range's radix select merged with the running list
    (the list's k keys take part as k more candidates), excluded dishes TKM_NONE before the selection.  `standin`: one of STANDINS --
    a wrong kernel or launcher under the same comparisons."""
    assert standin in (None,) + STANDINS
    W32 = np.ascontiguousarray(W32, np.float32)
    n, I = W32.shape
    W = I if W is None else W
    kw = dict(higher_id=standin == "higher_id", nan_first=standin == "nan_first")
    out_w = np.full((n, k), NAN_WORD, np.uint32)
    out_i = np.full((n, k), -1, np.int64)
    ids = np.arange(I)
    for j in range(n):
        w = words(W32[j])
        key = keys(w, ids, **kw)
        gone = np.zeros(I, bool)
        if lists is not None and len(lists[j]):
            gone[np.asarray(list(lists[j]), np.int64)] = True
        if standin != "strike_after":
            key = np.where(gone, NONE, key)
        run = np.full(k, NONE, np.uint64)
        for d0 in range(0, I, W):
            cand = key[d0:d0 + W]
            if d0 and standin != "forget":
                cand = np.concatenate([cand, run])
            run = radix_select(cand, k, one_short=standin == "one_short")[0]
        if standin == "strike_after":
            low = (run & np.uint64(0xFFFFFFFF)).astype(np.int64)
            hit = (run != NONE) & gone[np.minimum(low, I - 1)]
            run = np.concatenate([run[~hit], np.full(int(hit.sum()), NONE, np.uint64)])
        real = run != NONE
        low = (run[real] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        d = (~low if standin == "higher_id" else low).astype(np.int64)
        out_i[j, :d.size] = d
        out_w[j, :d.size] = w[d]
    return out_w, out_i


def same(a, b):
    return np.array_equal(np.asarray(a[0], np.uint32), np.asarray(b[0], np.uint32)) and np.array_equal(np.asarray(a[1], np.int64), np.asarray(b[1], np.int64))


# ---- exact tables ------------------------------------------------------------------------------------------------------------------
def nan_dishes(I):
    """the empty-mask dishes planted in a catalogue of I dishes: at its ends, around 256 and in the middle"""
    return sorted({d for d in (0, 5, 254, 255, 256, I // 2, I - 2, I - 1) if 0 <= d < I})


@functools.lru_cache(maxsize=None)
def exact_recipe(E, I, U=6):
    """seen_dish_cases.exact_tables at width E with I dishes, empty-mask (NaN) dishes planted; S float64 [U, I]: every value a float32"""
    rng = np.random.default_rng(40000 + 17 * E + I)
    r = types.SimpleNamespace(E=E, I=I, U=U, coef=sd.COEF)
    r.PM, r.RE, r.CE, r.cats = sd.exact_tables(rng, U, I, E)
    r.cats[nan_dishes(I)] = 0.0
    r.S = sd.score_matrix(r.PM, r.RE, r.CE, r.cats)
    r.users = np.asarray(list(range(U)) + [1, 0], np.int32)
    r.W32 = r.S[r.users].astype(np.float32)
    for a in (r.PM, r.RE, r.CE, r.cats, r.S, r.W32):
        a.setflags(write=False)
    return r


def exact_ks(I):
    return sorted({min(k, I) for k in KS})


# ---- normal tables -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normal_recipe(E, I=1300, U=24, seed=0, head=True):
    rng = np.random.default_rng(50000 + 13 * E + I + seed)
    r = types.SimpleNamespace(E=E, I=I, U=U, coef=sd.COEF)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, U, I, E)
    r.cats = sd.masks(rng, I)
    r.cats[nan_dishes(I)] = 0.0
    r.head = mlp_head(5 * E, 256, 64, rng, scale=4.0) if head else None
    r.users = np.concatenate([rng.permutation(U), [3, 3, 0]]).astype(np.int32)
    for a in (r.PM, r.RE, r.CE, r.cats):
        a.setflags(write=False)
    return r


# ---- exclusions --------------------------------------------------------------------------------------------------------------------
SEGMENTS = (0, 1, 63, 64, 65, 300, -5)       # ids per segment; -5: I - 5


def segment_lists(I, n, seed=0, best=None):
    """n exclusion lists cycling through SEGMENTS (row j: SEGMENTS[j % 7] ids, with repeats of some of them); `best` [n, >= 2]: ids each
    row's own list starts with, where the size allows (a row's best dishes: what the exclusion must remove)"""
    rng = np.random.default_rng(600 + seed + I)
    out = []
    for j in range(n):
        size = SEGMENTS[j % len(SEGMENTS)]
        size = I + size if size < 0 else min(size, I)
        own = [int(best[j][0]), int(best[j][1])] if best is not None and size >= 2 else []
        x = own + rng.choice(np.setdiff1d(np.arange(I), own), size - len(own), replace=False).tolist()
        out.append(sorted(x + x[:3]))                        # ascending, the first three ids twice
    return out


def csr(lists):
    """ascending lists WITH their repeats -> (offsets int64, ids int32)"""
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = [d for x in lists for d in x]
    return off, np.asarray(flat if flat else [0], np.int32)


def boundary_lists(I, W, n):
    """exclusions on both sides of every range edge: ids edge - 2 and edge + 1 for every edge (a multiple of W inside the catalogue)"""
    edges = list(range(W, I, W))
    x = sorted({d for e in edges for d in (e - 2, e + 1) if 0 <= d < I})
    return [x for _ in range(n)], edges


RANGE_W = 256                                # the narrowest ranges ("deep_chunk_pairs" = 256); every wider range's edge is one of theirs


@functools.lru_cache(maxsize=None)
def range_recipe(case):
    """The tables of the range cases -- "exact1300": exact_recipe(64, 1300), "normal5000": normal tables, I = 5 000 -- with best dishes
    planted on both sides of every range edge e (a multiple of 256): dishes e - 1 and e copy the best dish of user (e / 256) mod U, so
    both stand among that user's first three.  r.lists, r.edges: boundary_lists."""
    b = exact_recipe(64, 1300) if case == "exact1300" else normal_recipe(64, I=5000, U=12)
    r = types.SimpleNamespace(E=64, I=b.I, U=b.U, coef=b.coef, PM=b.PM, CE=b.CE, users=b.users)
    r.RE, r.cats = b.RE.copy(), b.cats.copy()
    S = b.S if case == "exact1300" else sd.score_matrix(b.PM, b.RE, b.CE, b.cats)
    for e in range(RANGE_W, r.I, RANGE_W):
        near = (np.arange(r.I) + 2) % RANGE_W < 4            # the planted and the excluded dishes of every edge: no source
        src = int(np.nanargmax(np.where(near, -np.inf, S[(e // RANGE_W) % r.U])))
        for d in (e - 1, e):
            r.RE[d], r.cats[d] = b.RE[src], b.cats[src]
    r.S = sd.score_matrix(r.PM, r.RE, r.CE, r.cats)
    r.W32 = r.S[r.users].astype(np.float32)                  # (exact1300: the engine's words)
    r.lists, r.edges = boundary_lists(r.I, RANGE_W, len(r.users))
    return r


def boundary_condition(out_i, lists, edges):
    """a boundary case has listed and excluded dishes on both sides of every range edge"""
    listed = set(np.asarray(out_i).ravel().tolist())
    excluded = set(d for x in lists for d in x)
    return all((e - 1) in listed and e in listed and (e - 2) in excluded and (e + 1) in excluded for e in edges)


# ---- ties and digits -----------------------------------------------------------------------------------------------------------------
TIE_GROUPS = (2, 65, 700)
TIE_I = 1300


@functools.lru_cache(maxsize=None)
def tie_recipe(group):
    """Exact tables (E = 64, I = 1 300) in which `group` dishes are copies of one dish: a group of bit-equal scores.  r.k[j]: a k at
    which the group straddles position k in row j's order (entries k - 1 and k of the order score the same word)."""
    base = exact_recipe(64, TIE_I)
    rng = np.random.default_rng(70 + group)
    r = types.SimpleNamespace(E=64, I=TIE_I, U=base.U, coef=base.coef, PM=base.PM, CE=base.CE)
    r.RE, r.cats = base.RE.copy(), base.cats.copy()
    src = 100
    r.copies = np.sort(np.concatenate([[src], rng.choice(np.setdiff1d(np.arange(TIE_I), nan_dishes(TIE_I) + [src]), group - 1, replace=False)]))
    r.RE[r.copies] = base.RE[src]
    r.cats[r.copies] = base.cats[src]
    r.S = sd.score_matrix(r.PM, r.RE, r.CE, r.cats)
    users, ks = [], []
    for u in range(r.U):                                     # the users whose order has the group's middle within the first 1 024
        _, o = key_lists(r.S[u:u + 1].astype(np.float32), TIE_I)
        at = np.flatnonzero(np.isin(o[0], r.copies))
        if at[0] + (group + 1) // 2 <= K_MAX:
            users.append(u)
            ks.append(int(at[0] + (group + 1) // 2))
    assert len(users) >= 2
    r.users, r.k = np.asarray(users, np.int32), ks
    r.W32 = r.S[r.users].astype(np.float32)
    return r


def straddles(W32row, k):
    """entries k - 1 and k of the row's order score the same word (a tie group lies across position k)"""
    w, _ = key_lists(np.asarray(W32row, np.float32)[None], k + 1)
    return w[0, k - 1] == w[0, k] and w[0, k] != NAN_WORD


@functools.lru_cache(maxsize=None)
def neighbour_recipe(I=700, k=300):
    """Scores that are neighbouring floats: every dish has the mask (1, 0, 0, 0), user 0 holds 1.0 in one low-level component and
    zeros elsewhere, so at coef 0.5 dish d scores 0.5 RE[d, 0] exactly; RE[d, 0] walks the floats next to 1.0 in a shuffled order."""
    rng = np.random.default_rng(81)
    r = types.SimpleNamespace(E=64, I=I, U=2, coef=0.5, k=k)
    r.PM = np.zeros((2, 5, 64), np.float32)
    r.PM[0, 1, 0] = 1.0
    r.RE = np.zeros((I, 64), np.float32)
    steps = rng.permutation(I) - I // 2
    r.RE[:, 0] = (np.float32(1.0).view(np.uint32) + steps.astype(np.int64)).astype(np.uint32).view(np.float32)
    r.CE = (rng.integers(-16, 17, (4, 64)) / 16.0).astype(np.float32)
    r.cats = np.zeros((I, 4), np.float32)
    r.cats[:, 0] = 1.0
    r.users = np.asarray([0, 1], np.int32)                  # user 1: the all-zero user, every score equal
    r.W32 = np.stack([np.float32(0.5) * r.RE[:, 0], np.zeros(I, np.float32)])
    return r


@functools.lru_cache(maxsize=None)
def nan40_recipe():
    """40 dishes of which 30 score NaN"""
    rng = np.random.default_rng(91)
    r = types.SimpleNamespace(E=64, I=40, U=4, coef=sd.COEF, k=35)
    r.PM, r.RE, r.CE, r.cats = sd.exact_tables(rng, r.U, r.I, r.E)
    r.nan = np.sort(rng.permutation(40)[:30])
    r.cats[r.nan] = 0.0
    r.S = sd.score_matrix(r.PM, r.RE, r.CE, r.cats)
    r.users = np.arange(r.U, dtype=np.int32)
    r.W32 = r.S.astype(np.float32)
    return r


def adversarial_rows(rng):
    """(key rows [n, W], k) of the radix select's hard cases, as keys: a tie group of 2 / 65 / 700 bit-equal scores across position k,
    a row of one value, neighbouring floats around the k-th, both signs and both zeros, 40 entries of which 30 are NaN at k = 35,
    several TKM_NONE keys, fewer real keys than k"""
    out = []
    W = 1500
    ids = np.arange(W)
    base = rng.standard_normal(W).astype(np.float32)
    for g in TIE_GROUPS:
        s = base.copy()
        pick = rng.choice(W, g, replace=False)
        s[pick] = np.float32(0.125)
        at = int((s > 0.125).sum())
        out.append((keys(words(s), ids), min(at + (g + 1) // 2, K_MAX), "tie group of %d" % g))
    out.append((keys(words(np.zeros(W, np.float32)), ids), 1024, "one value"))
    out.append((keys(words(np.full(W, np.inf, np.float32)), ids), 77, "all +inf"))
    nb = (np.float32(1.0).view(np.uint32) + rng.permutation(W).astype(np.uint32)).view(np.float32)
    out.append((keys(words(nb), ids), 700, "neighbouring floats"))
    z = base.copy()
    z[::7] = 0.0
    z[3::7] = -0.0
    out.append((keys(words(z), ids), int((z > 0).sum()) + 50, "both signs, both zeros"))
    n40 = rng.standard_normal(40).astype(np.float32)
    n40[rng.permutation(40)[:30]] = np.nan
    out.append((keys(words(n40), np.arange(40)), 35, "30 of 40 NaN"))
    holes = keys(words(base), ids)
    holes[rng.choice(W, 900, replace=False)] = NONE
    out.append((holes, 500, "900 TKM_NONE keys"))
    out.append((holes, 1024, "fewer real keys than k"))
    out.append((np.full(300, NONE, np.uint64), 10, "no real key"))
    return out
