"""Inputs, host restatement and stand-ins of the filtered-menu tests (tests/test_menu_filtered_cases_cpu.py,
tests/test_gpu_menu_filtered.py): m2d_topk_menu_filtered, m2d_topk_menu's greedy walk over the dishes of a
slate (the whole catalogue without one) less each user's exclusion list.

The restatement (filtered_lists) is menu_cases' own: a row's order is mc.order_of over the ALLOWED ids, then the same greedy steps.
merged_filtered is the call as the engine computes it: the slate partitioned by signature, per signature the first k of the order
over its allowed dishes, cut in ranges of W with a running list, then the capped merge.  The CPU file asserts that the two agree.
Nothing here imports the engine; recipes are menu_cases' (shared, not written into)."""
import functools
import types

import numpy as np

import deep_cases as dc
import menu_cases as mc
import seen_dish_cases as sd

NAN_WORD = mc.NAN_WORD
RANGE_W = mc.RANGE_W
# wrong kernels under the same comparisons: the first lives in the walk, the others in the per-signature lists
STANDINS = ("counted", "by_position", "consume_others", "first_range_only", "slate_descending", "outside_shift")
EXCL_SIZES = (0, 1, 63, 64, 65, 300)           # ids per exclusion segment, cycling over the rows
SEGMENT_NS = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)      # and one of 16 385: select_threads' 1 / 4 / 16 waves, a wave's second step
SLATE_NDS = (1, 63, 64, 65, 255, 256, 257, 1300)


def _base(I, slate):
    return np.arange(I, dtype=np.int64) if slate is None else np.asarray(slate, np.int64)


def _lists(lists, n):
    return [np.zeros(0, np.int64)] * n if lists is None else [np.asarray(x, np.int64) for x in lists]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _ghost_steps(order, osig, ghost, cap, k, C):
    """stand-in `counted`: the walk over the slate's whole order in which an excluded dish (ghost) is left out of the list but, where it
    would have been taken, still counts against its caps"""
    n = np.zeros(C, np.int64)
    out = []
    for d, s, g in zip(order.tolist(), osig.tolist(), ghost.tolist()):
        cs = [c for c in range(C) if (s >> c) & 1]
        if all(n[c] < cap[c] for c in cs):
            if not g:
                out.append(d)
            for c in cs:
                n[c] += 1
            if len(out) == k:
                break
    return out


def filtered_lists(W32, cats, caps, k, lists=None, slate=None, standin=None):
    """THE RESTATEMENT: (score words uint32 [n, k], ids int64 [n, k]) of the float32 matrix W32 [n, I]: row j's menu over the dishes of
    `slate` (ascending ids; None: all I) less lists[j], under caps [n, C]; -1 / NAN_WORD where fewer than k can be taken.  An excluded
    id outside the slate is ignored; a dish that is left out counts against no cap."""
    assert standin in (None,) + STANDINS
    if standin not in (None, "counted"):
        return merged_filtered(W32, cats, caps, k, lists, slate, W=RANGE_W, standin=standin)
    W32 = np.ascontiguousarray(W32, np.float32)
    n, I = W32.shape
    C = np.asarray(cats).shape[1]
    sig = mc.signatures(cats)
    caps = np.broadcast_to(np.asarray(caps, np.int64), (n, C))
    base, lists, w = _base(I, slate), _lists(lists, n), dc.words(W32)
    out = []
    for j in range(n):
        gone = np.isin(base, lists[j])
        if standin == "counted":
            order = mc.order_of(w[j][base], base)
            out.append(_ghost_steps(order, sig[order], np.isin(order, lists[j]), caps[j], k, C))
        else:
            ids = base[~gone]
            order = mc.order_of(w[j][ids], ids)
            out.append(mc._steps(order, sig[order], caps[j], k, C))
    return mc._rows(out, w, k)


def slate_index(sig, I, slate=None):
    """(slate_perm, seg_off[65]): the slate's ids by (signature, id)"""
    base = _base(I, slate)
    s = np.asarray(sig, np.int64)[base]
    seg_off = np.zeros(65, np.int64)
    np.cumsum(np.bincount(s, minlength=64), out=seg_off[1:])
    return base[np.argsort(s, kind="stable")], seg_off


def _struck(ids, r0, X, base, standin, cursor):
    """the columns of one range (ids: its ascending id table, r0: where it starts in its segment) that row's exclusion list X (ascending,
    repeats allowed) removes -- as the kernel does it, or as a wrong one would"""
    if standin == "by_position":             # the dish-range strike on an id table: column e is taken for dish e
        return np.isin(np.arange(len(ids)), X)
    if standin == "first_range_only":
        return np.isin(ids, X) if r0 == 0 else np.zeros(len(ids), bool)
    if standin == "outside_shift":           # no equality test behind the lower bound: an id outside the slate strikes the next dish of it
        at = np.searchsorted(base, X)
        return np.isin(ids, base[at[at < len(base)]])
    if standin == "consume_others":          # a cursor that moves one entry per column: ids of other signatures hold it back
        out = np.zeros(len(ids), bool)
        c = cursor[0]
        for e, d in enumerate(ids.tolist()):
            if c < len(X):
                if X[c] == d:
                    out[e] = True
                if X[c] <= d:
                    c += 1
        cursor[0] = c
        return out
    return np.isin(ids, X)


def merged_filtered(W32, cats, caps, k, lists=None, slate=None, W=None, standin=None):
    """The call as the engine computes it.  Stand-ins: STANDINS[1:] -- `slate_descending`: the per-signature lists resolve equal
    scores to the higher id, as a partition in descending id would across ranges."""
    W32 = np.ascontiguousarray(W32, np.float32)
    n, I = W32.shape
    C = np.asarray(cats).shape[1]
    sig = mc.signatures(cats)
    caps = np.broadcast_to(np.asarray(caps, np.int64), (n, C))
    base, lists, w = _base(I, slate), _lists(lists, n), dc.words(W32)
    perm, seg_off = slate_index(sig, I, slate)
    hi = standin == "slate_descending"
    out = []
    for j in range(n):
        X = np.sort(lists[j])
        heads = {}
        for s in range(64):
            seg = perm[seg_off[s]:seg_off[s + 1]]
            if not len(seg):
                continue
            Wr = len(seg) if W is None else W
            cand, cursor = np.zeros(0, np.int64), [0]
            for r0 in range(0, len(seg), Wr):
                ids = seg[r0:r0 + Wr]
                both = np.concatenate([cand, ids[~_struck(ids, r0, X, base, standin, cursor)]])      # the running list is not struck again
                cand = mc.order_of(w[j][both], both, higher_id=hi)[:k]
            heads[s] = list(cand)
        cap = caps[j]
        cnt = np.zeros(C, np.int64)
        full = sum(1 << c for c in range(C) if cap[c] <= 0)
        row = []
        while len(row) < k:
            adm = [s for s, h in heads.items() if h and (s & full) == 0]
            if not adm:
                break
            first = [heads[s][0] for s in adm]
            s = adm[int(np.argmin(dc.keys(w[j][first], first)))]
            row.append(int(heads[s].pop(0)))
            for c in range(C):
                if (s >> c) & 1:
                    cnt[c] += 1
                    if cnt[c] >= cap[c]:
                        full |= 1 << c
        out.append(row)
    return mc._rows(out, w, k)


def host_workaround(W32, cats, caps, k, lists, depth=1024):
    """what callers did before: topk_users_deep(depth, exclude) and the greedy walk on the host -- wrong or short where the caps are
    not filled within `depth`"""
    W32 = np.ascontiguousarray(W32, np.float32)
    C = np.asarray(cats).shape[1]
    sig = mc.signatures(cats)
    caps = np.broadcast_to(np.asarray(caps, np.int64), (W32.shape[0], C))
    _, deep = dc.key_lists(W32, min(depth, W32.shape[1]), lists)
    out = []
    for j in range(W32.shape[0]):
        order = deep[j][deep[j] >= 0]
        out.append(mc._steps(order, sig[order], caps[j], k, C))
    return mc._rows(out, dc.words(W32), k)


# ---- exclusion lists ---------------------------------------------------------------------------------------------------------------------
def own_menu_lists(W32, cats, caps, k, slate=None, sizes=EXCL_SIZES, seed=0, take=2):
    """Row j's list: sizes[j % len(sizes)] ids, ascending WITH repeats -- the first `take` dishes of the row's OWN unfiltered menu
    (where the size allows: the exclusion must change the row), the rest drawn from the whole catalogue: ids of every signature
    interleaved, ids outside a slate included; every fifth id of a longer list is repeated."""
    W32 = np.ascontiguousarray(W32, np.float32)
    n, I = W32.shape
    rng = np.random.default_rng(700 + seed + I)
    _, own = filtered_lists(W32, cats, caps, k, None, slate)
    out = []
    for j in range(n):
        m = sizes[j % len(sizes)]
        mine = own[j][own[j] >= 0][:min(take, m)]
        rest = rng.choice(np.setdiff1d(np.arange(I), mine), min(max(m - len(mine), 0), I - len(mine)), replace=False)
        x = np.sort(np.concatenate([mine, rest]).astype(np.int64))
        if len(x) >= 5:
            x = np.sort(np.concatenate([x, x[::5]]))
        out.append(x)
    return out


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids = np.concatenate([np.asarray(x, np.int64) for x in lists]).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
    return off, ids


def differs(a, b):
    return (np.asarray(a[1]) != np.asarray(b[1])).any(1)


# ---- recipes ---------------------------------------------------------------------------------------------------------------------------------
SEG_SIG = 5                                  # the planted segment's signature in segment_recipe_n


@functools.lru_cache(maxsize=None)
def segment_recipe_n(n, E=64, multi=True, C=4):
    """A segment of exactly n dishes (signature SEG_SIG) spread over the id range -- `multi`: among dishes of nine other signatures, about
    as many again and at least 300; otherwise the segment is the whole catalogue (one_signature_recipe's form)."""
    I = n + max(n, 300) if multi else n
    rng = np.random.default_rng(37000 + 3 * n + (1 if multi else 0) + E)
    r = types.SimpleNamespace(C=C, E=E, I=I, U=6, coef=sd.COEF)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, r.U, I, E, C)
    sig = np.full(I, SEG_SIG)
    if multi:
        other = [s for s in (1, 2, 3, 4, 6, 7, 0, (1 << C) - 1, (1 << C) - 2) if s != SEG_SIG]
        sig[rng.permutation(I)[:I - n]] = rng.choice(other, I - n)
    r.cats = mc._bits(sig, C)
    r.users = np.asarray(list(range(r.U)) + [2, 2], np.int32)
    r.segment = np.flatnonzero(sig == SEG_SIG)
    assert len(r.segment) == n
    return mc._finish(r)


def step_edges(n):
    """positions inside a segment of n dishes where a 64-slice (and with it every 256-step) begins"""
    return list(range(64, n, 64))


@functools.lru_cache(maxsize=None)
def slice_edge_recipe(n=1025, multi=True):
    """segment_recipe_n(n) with best dishes planted on both sides of every 64-slice edge, at the segment's first and at its last dish:
    position p of the segment that is an edge, p - 1, 0 and n - 1 take the row of the dish user (p / 64 mod U) likes best in the segment
    -- bit-equal copies that head the segment's list for that user.  r.planted[u]: (position, dish) pairs of user u; in a pair across
    an edge one side is to be excluded and the other must be listed."""
    b = segment_recipe_n(n, multi=multi)
    r = types.SimpleNamespace(C=b.C, E=b.E, I=b.I, U=b.U, coef=b.coef, PM=b.PM.copy(), CE=b.CE.copy(), cats=b.cats.copy(), users=b.users,
                              segment=b.segment)
    S = mc.host_scores(b)
    RE = b.RE.copy()
    r.planted = {u: [] for u in range(r.U)}
    for p in [0] + step_edges(n) + [n]:
        u = (p // 64) % r.U
        best = r.segment[int(np.argmax(S[u][r.segment]))]
        for q in (p - 1, p):
            if 0 <= q < n:
                RE[r.segment[q]] = b.RE[best]
                r.planted[u].append((q, int(r.segment[q])))
    r.RE = RE
    return mc._finish(r)


def edge_lists(r, users):
    """per row of `users`: of every planted pair of that user, the dish at the even position is excluded (across an edge p: p - 1 when p
    is odd ... the other side stays); -> (lists, kept): kept[j] the planted dishes that must be listed"""
    lists, kept = [], []
    for u in np.asarray(users).tolist():
        x = sorted(d for q, d in r.planted[u] if q % 2 == 0)
        lists.append(np.asarray(x, np.int64))
        kept.append([d for q, d in r.planted[u] if q % 2 == 1])
    return lists, kept


def range_edge_lists(r, users):
    """menu_cases.edge_recipe: at every index edge p the dishes perm[p - 1] and perm[p] head their segment's list for user p mod U.  The
    row of user u excludes perm[p - 1] at the even-numbered edges of the index and perm[p] at the odd-numbered ones, and the dish on the
    other side stays; -> (lists, pairs): pairs[j] the (excluded, kept) dishes of row j"""
    lists, pairs = [], []
    for u in np.asarray(users).tolist():
        mine = [(t, p) for t, p in enumerate(r.edges) if p % r.U == u]
        pairs.append([(int(r.perm[p - 1]), int(r.perm[p])) if t % 2 == 0 else (int(r.perm[p]), int(r.perm[p - 1])) for t, p in mine])
        lists.append(np.asarray(sorted(x for x, _ in pairs[-1]), np.int64))
    return lists, pairs


def slate_of(I, nD, seed=0, keep=None):
    """nD ascending ids out of I, `keep` among them"""
    rng = np.random.default_rng(800 + seed + I + nD)
    keep = np.zeros(0, np.int64) if keep is None else np.unique(keep)[:nD]
    rest = rng.choice(np.setdiff1d(np.arange(I), keep), nD - len(keep), replace=False)
    return np.sort(np.concatenate([keep, rest])).astype(np.int32)
