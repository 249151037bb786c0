"""Inputs, host restatement and stand-ins of the menu tests (tests/test_menu_cases_cpu.py, tests/test_gpu_menu.py; DESIGN.md section
4.13): m2d_topk_menu, the k best dishes of the whole catalogue with at most cap[u][c] dishes of category c in a list.

Every comparison is ids as integers and scores as 32-bit words.  The order is deep_cases' restatement of tkm_key; the greedy is stated
three times: as the definition reads (plain_menu, a Python loop over the whole order), as k vectorised steps over the order
(menu_lists: the restatement the GPU file compares with) and as the engine computes it (merged_menu: each signature's own first k
dishes, merged under the caps) -- the CPU file asserts that the three agree.  Nothing here imports the engine.  Recipes are computed
once and shared (lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

import deep_cases as dc
import group_cases as gc      # noqa: F401  (the exact tables are the ones the deep and group cases use)
import seen_dish_cases as sd

MAX_C = 6                                    # include/m2d.h: M2D_MENU_MAX_CATEGORIES
K_MAX = 64
NAN_WORD = dc.NAN_WORD
STANDINS = ("per_signature", "higher_id", "cap_empty", "readmit", "first_cap_cut", "minus_zero_member")


# ---- membership ---------------------------------------------------------------------------------------------------------------------
def signatures(cats, minus_zero_member=False):
    """sig[d]: bit c iff cats[d][c] != 0.0f in C semantics (-0.0 is no member; a NaN or a negative weight is one).  Stand-in
    `minus_zero_member`: the comparison on the word, which takes -0.0 for a member."""
    cats = np.asarray(cats, np.float32)
    member = (cats.view(np.uint32) != 0) if minus_zero_member else (cats != 0)
    return (member.astype(np.int64) << np.arange(cats.shape[1])[None, :]).sum(1)


def index(sig):
    """the signature index: (perm, seg_off[65]) -- the dish ids by (signature, id)"""
    sig = np.asarray(sig, np.int64)
    perm = np.argsort(sig, kind="stable")
    seg_off = np.zeros(65, np.int64)
    np.cumsum(np.bincount(sig, minlength=64), out=seg_off[1:])
    return perm, seg_off


def order_of(wrow, ids=None, **kw):
    """the dish ids of one row of score words in m2d_topk_users' order"""
    ids = np.arange(len(wrow)) if ids is None else np.asarray(ids, np.int64)
    return ids[np.argsort(dc.keys(wrow, ids, **kw), kind="stable")]


# ---- the greedy, three ways -----------------------------------------------------------------------------------------------------------
def plain_menu(order, sig, cap, k):
    """the definition as it reads: walk `order`, take d iff n[c] < cap[c] for every c of sig[d], count, stop at k"""
    n = [0] * MAX_C
    out = []
    for d in order:
        cs = [c for c in range(MAX_C) if (int(sig[d]) >> c) & 1]
        if all(n[c] < cap[c] for c in cs):
            out.append(int(d))
            for c in cs:
                n[c] += 1
            if len(out) == k:
                break
    return out


def _steps(order, osig, cap, k, C, standin=None):
    """k vectorised steps over one row's order: the first position behind the last one taken whose signature shares no bit with `full`"""
    cap = np.asarray(cap, np.int64)
    n = np.zeros(C, np.int64)
    per_sig = np.zeros(64, np.int64)
    full = sum(1 << c for c in range(C) if cap[c] <= 0)
    out, at = [], 0
    while len(out) < k and at < len(order):
        ok = (osig[at:] & full) == 0
        if standin == "cap_empty":               # empty-mask dishes count against category 0
            ok &= (osig[at:] != 0) | (n[0] < cap[0])
        if standin == "per_signature":           # a signature's own count against its categories' caps
            lim = np.asarray([min([cap[c] for c in range(C) if (s >> c) & 1] + [1 << 30]) for s in range(64)])
            ok = per_sig[osig[at:]] < lim[osig[at:]]
        if not ok.any():
            break
        at += int(np.argmax(ok))
        s = int(osig[at])
        out.append(int(order[at]))
        per_sig[s] += 1
        for c in range(C):
            if (s >> c) & 1 or (standin == "cap_empty" and s == 0 and c == 0):
                n[c] += 1
                if n[c] >= cap[c]:
                    full |= 1 << c
        at += 1
    return out


def _rows(lists, wrows, k):
    out_w = np.full((len(lists), k), NAN_WORD, np.uint32)
    out_i = np.full((len(lists), k), -1, np.int64)
    for j, ids in enumerate(lists):
        out_i[j, :len(ids)] = ids
        out_w[j, :len(ids)] = wrows[j][np.asarray(ids, np.int64)] if len(ids) else []
    return out_w, out_i


def menu_lists(W32, cats, caps, k, standin=None):
    """THE RESTATEMENT: (score words uint32 [n, k], ids int64 [n, k]) of the float32 matrix W32 [n, I] under caps [n, C]; -1 / NAN_WORD
    where the caps leave fewer than k.  `standin`: one of STANDINS -- a wrong kernel under the same comparisons (the three that live
    in the merge are merged_menu's)."""
    assert standin in (None,) + STANDINS
    if standin in ("higher_id", "readmit", "first_cap_cut"):
        return merged_menu(W32, cats, caps, k, standin)
    W32 = np.ascontiguousarray(W32, np.float32)
    C = np.asarray(cats).shape[1]
    sig = signatures(cats, minus_zero_member=standin == "minus_zero_member")
    caps = np.broadcast_to(np.asarray(caps, np.int64), (W32.shape[0], C))
    w = dc.words(W32)
    lists = []
    for j in range(W32.shape[0]):
        order = order_of(w[j])
        lists.append(_steps(order, sig[order], caps[j], k, C, standin))
    return _rows(lists, w, k)


def merged_menu(W32, cats, caps, k, standin=None, W=None):
    """The call as the engine computes it: per signature the first k of the order over its own dishes (in ranges of W dishes with a
    running list when `W` is given), then k steps that take the best admissible head.  Stand-ins: `higher_id` (equal scores of two
    segments go to the higher id), `readmit` (only the categories the last dish filled are closed), `first_cap_cut` (every
    segment's list is cut to category 0's cap)."""
    W32 = np.ascontiguousarray(W32, np.float32)
    C = np.asarray(cats).shape[1]
    sig = signatures(cats)
    perm, seg_off = index(sig)
    caps = np.broadcast_to(np.asarray(caps, np.int64), (W32.shape[0], C))
    w = dc.words(W32)
    lists = []
    for j in range(W32.shape[0]):
        cap = caps[j]
        heads = {}
        for s in range(64):
            ids = perm[seg_off[s]:seg_off[s + 1]]
            if not len(ids):
                continue
            if W is None:
                cand = order_of(w[j][ids], ids)[:k]
            else:
                cand = np.zeros(0, np.int64)
                for r0 in range(0, len(ids), W):
                    both = np.concatenate([cand, ids[r0:r0 + W]])
                    cand = order_of(w[j][both], both)[:k]
            if standin == "first_cap_cut":
                cand = cand[:max(int(cap[0]), 0)]
            heads[s] = list(cand)
        n = np.zeros(C, np.int64)
        full = sum(1 << c for c in range(C) if cap[c] <= 0)
        out = []
        while len(out) < k:
            adm = [s for s, h in heads.items() if h and (s & full) == 0]
            if not adm:
                break
            hk = dc.keys(w[j][[heads[s][0] for s in adm]], [heads[s][0] for s in adm], higher_id=standin == "higher_id")
            s = adm[int(np.argmin(hk))]
            out.append(int(heads[s].pop(0)))
            if standin == "readmit":
                full = sum(1 << c for c in range(C) if cap[c] <= 0)
            for c in range(C):
                if (s >> c) & 1:
                    n[c] += 1
                    if n[c] >= cap[c]:
                        full |= 1 << c
        lists.append(out)
    return _rows(lists, w, k)


def host_workaround(W32, cats, caps, k, depth):
    """what callers did before: the first `depth` of the order, filtered on the host -- wrong or short where the caps are not filled
    within `depth`"""
    W32 = np.ascontiguousarray(W32, np.float32)
    C = np.asarray(cats).shape[1]
    sig = signatures(cats)
    caps = np.broadcast_to(np.asarray(caps, np.int64), (W32.shape[0], C))
    w = dc.words(W32)
    lists = []
    for j in range(W32.shape[0]):
        order = order_of(w[j])[:depth]
        lists.append(_steps(order, sig[order], caps[j], k, C))
    return _rows(lists, w, k)


# ---- caps ----------------------------------------------------------------------------------------------------------------------------
def caps_uncapped(n, C, k, more=0):
    return np.full((n, C), k + more, np.int32)


def caps_all(n, C, cap):
    return np.full((n, C), cap, np.int32)


def caps_zero_on(n, C, k, c):
    caps = np.full((n, C), k, np.int32)
    caps[:, c] = 0
    return caps


def caps_mixed(n, C, seed=0, hi=3):
    """every user its own caps in 0 .. hi, row 0 all `hi`, a row of all ones"""
    rng = np.random.default_rng(900 + seed + 7 * C)
    caps = rng.integers(0, hi + 1, (n, C)).astype(np.int32)
    caps[0] = hi
    if n > 1:
        caps[1] = 1
    return caps


CAP_SETS = ("one", "two", "zero_on_busiest", "mixed", "none")


def busiest(W32, cats, k=10):
    """the category with most dishes in the uncapped lists of k: the one whose cap of 0 shows"""
    sig = signatures(cats)
    ids = dc.key_lists(W32, k)[1]
    top = sig[ids[ids >= 0]]
    return int(np.argmax([((top >> c) & 1).sum() for c in range(np.asarray(cats).shape[1])]))


def cap_set(name, n, C, k, busy=0):
    """"one" / "two": that cap everywhere; "zero_on_busiest": cap 0 on category `busy`, k elsewhere; "mixed": every user its own;
    "none": cap 0 everywhere -- the empty-mask dishes are all a list can hold"""
    return {"one": lambda: caps_all(n, C, 1), "two": lambda: caps_all(n, C, 2), "zero_on_busiest": lambda: caps_zero_on(n, C, k, busy),
            "mixed": lambda: caps_mixed(n, C), "none": lambda: caps_all(n, C, 0)}[name]()


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def host_scores(r, dtype=np.float64, users=None):
    """[len(users), I]: Model_Recommender.py:67-96 for every dish, in `dtype` throughout (sums in increasing e, the two products and
    one sum of the blend) -- the exact recipes' float32 words, the other recipes' scores up to rounding"""
    users = np.arange(r.U) if users is None else np.asarray(users)
    PM, RE, CE, m = (np.asarray(x, dtype) for x in (r.PM, r.RE, r.CE, r.cats))
    a = dtype(r.coef)
    b = dtype(1.0) - a
    with np.errstate(invalid="ignore", divide="ignore"):
        n = m.sum(1, dtype=dtype)
        high = (PM[users, 0] @ (m @ CE).T).astype(dtype)                              # [n, I]
        low = np.einsum("ie,uie->ui", RE, np.einsum("ic,uce->uie", m, PM[users, 1:])).astype(dtype)
        return (a * (high / n) + b * (low / n)).astype(dtype)


EXACT_PATTERNS = {3: (1, 2, 4, 3, 5, 6), 4: sd.EXACT_PATTERNS, 5: (1, 2, 4, 8, 16, 3, 5, 6, 9, 10, 12, 17, 18, 20, 24, 15, 23, 27, 29, 30),
                  6: (1, 2, 4, 8, 16, 32, 3, 5, 6, 9, 10, 12, 17, 33, 34, 36, 40, 48, 15, 23, 39, 51, 60)}      # popcounts 1, 2, 4: exact divisions


def _bits(sig, C):
    return ((np.asarray(sig, np.int64)[:, None] >> np.arange(C)[None, :]) & 1).astype(np.float32)


def _finish(r):
    for a in (r.PM, r.RE, r.CE, r.cats):
        a.setflags(write=False)
    r.sig = signatures(r.cats)
    return r


@functools.lru_cache(maxsize=None)
def exact_recipe(C=4, E=64, I=1300, U=6):
    """Exact-arithmetic tables (entries j / 16, coef 0.5, masks whose popcount is 1, 2 or 4: every float32 operation of a score is
    exact); C = 4: deep_cases.exact_recipe's own tables.  Empty-mask dishes at deep_cases.nan_dishes."""
    r = types.SimpleNamespace(C=C, E=E, I=I, U=U, coef=sd.COEF)
    if C == 4:
        b = dc.exact_recipe(E, I, U)
        r.PM, r.RE, r.CE, r.cats = b.PM.copy(), b.RE.copy(), b.CE.copy(), b.cats.copy()
    else:
        rng = np.random.default_rng(31000 + 101 * C + 17 * E + I)
        f = lambda shape: (rng.integers(-16, 17, shape) / 16.0).astype(np.float32)      # noqa: E731
        r.PM, r.RE, r.CE = f((U, C + 1, E)), f((I, E)), f((C, E))
        r.cats = _bits(np.asarray(EXACT_PATTERNS[C])[rng.integers(0, len(EXACT_PATTERNS[C]), I)], C)
        r.cats[dc.nan_dishes(I)] = 0.0
    r.users = np.asarray(list(range(U)) + [1, 0], np.int32)
    return _finish(r)


@functools.lru_cache(maxsize=None)
def normal_recipe(C=6, E=64, I=1300, U=8, form="multi", seed=0):
    """Normal tables with every one of the 2^C signatures present (C = 6: all 64).  `form`: "multi" 0 / 1 masks; "weighted" member
    weights 0.5 / 1 / 2; "negative" also -0.5; "minus_zero" multi-hot with -0.0 in half of the places that hold no member."""
    rng = np.random.default_rng(32000 + 101 * C + 17 * E + I + seed)
    r = types.SimpleNamespace(C=C, E=E, I=I, U=U, coef=sd.COEF, form=form)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, U, I, E, C)
    sig = rng.integers(1, 1 << C, I)
    sig[rng.permutation(I)[:1 << C]] = np.arange(1 << C)     # every signature, the empty one included
    r.cats = _bits(sig, C)
    if form in ("weighted", "negative"):
        r.cats *= rng.choice(np.asarray([0.5, 1.0, 2.0] + ([-0.5] if form == "negative" else []), np.float32), (I, C))
    if form == "minus_zero":
        r.cats = np.where((r.cats == 0) & (rng.random((I, C)) < 0.5), np.float32(-0.0), r.cats).astype(np.float32)
    r.users = np.concatenate([rng.permutation(U), [3, 3, 0]]).astype(np.int32)
    return _finish(r)


SEGMENT_SIZES = {1: 1, 2: 63, 3: 64, 4: 65, 5: 0}          # signature -> dishes; three empty-mask dishes; the rest: signatures 6 .. 15


@functools.lru_cache(maxsize=None)
def segment_recipe(E=64, I=600):
    """C = 4, segments of 0 / 1 / 63 / 64 / 65 dishes (SEGMENT_SIZES), their dishes spread over the id range"""
    rng = np.random.default_rng(33000 + I)
    r = types.SimpleNamespace(C=4, E=E, I=I, U=6, coef=sd.COEF)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, r.U, I, E)
    planted = [s for s, n in SEGMENT_SIZES.items() for _ in range(n)] + [0, 0, 0]
    sig = np.concatenate([planted, rng.choice([6, 7, 8, 9, 10, 11, 12, 13, 14, 15], I - len(planted))])
    r.cats = _bits(rng.permutation(sig), 4)
    r.users = np.asarray(list(range(r.U)) + [2, 2], np.int32)
    return _finish(r)


@functools.lru_cache(maxsize=None)
def one_signature_recipe(E=64, I=700, sig=5):
    """one signature holds the whole catalogue: one segment, cut into ranges"""
    rng = np.random.default_rng(34000 + I)
    r = types.SimpleNamespace(C=4, E=E, I=I, U=6, coef=sd.COEF)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, r.U, I, E)
    r.cats = _bits(np.full(I, sig), 4)
    r.users = np.arange(r.U, dtype=np.int32)
    return _finish(r)


TIE_GROUPS = (2, 65)


@functools.lru_cache(maxsize=None)
def tie_recipe(group, C=4, E=64, I=1300):
    """Bit-equal scores ACROSS segments.  Categories 0 and 1 are twins (CE[1] = CE[0], PM[:, 2] = PM[:, 1]): a dish scores the same word
    under the mask {0} and under {1} -- the same non-zero terms in the same order.  `group` dishes copy one dish's row, their masks
    alternating {0}, {1}: a tie group over two segments.  r.k[j]: a k at which the group lies across position k of user j's uncapped
    order; the last user is the all-zero user (every score equal: one tie group over every segment)."""
    b = exact_recipe(C, E, I)
    rng = np.random.default_rng(35000 + group)
    r = types.SimpleNamespace(C=C, E=E, I=I, U=b.U, coef=b.coef)
    r.PM, r.RE, r.CE, r.cats = b.PM.copy(), b.RE.copy(), b.CE.copy(), b.cats.copy()
    r.CE[1] = r.CE[0]
    r.PM[:, 2] = r.PM[:, 1]
    r.PM[b.U - 1] = 0.0
    W32 = host_scores(r, np.float32)
    single = np.flatnonzero(np.isin(signatures(r.cats), (1, 2)))                      # the source: the {0} / {1} dish most users rank high
    place = np.stack([np.argsort(order_of(dc.words(W32[j]))) for j in range(b.U - 1)])[:, single]
    src = int(single[np.lexsort((place.sum(0), -(place < 20).sum(0)))[0]])
    r.copies = np.sort(np.concatenate([[src], rng.choice(np.setdiff1d(np.arange(I), dc.nan_dishes(I) + [src]), group - 1, replace=False)]))
    r.RE[r.copies] = b.RE[src]
    r.cats[r.copies] = 0.0
    r.cats[r.copies[0::2], 0] = 1.0
    r.cats[r.copies[1::2], 1] = 1.0
    _finish(r)
    W32 = host_scores(r, np.float32)
    users, ks = [], []
    for j in range(r.U):                                     # the users whose order has the group's middle within the first 64
        at = np.flatnonzero(np.isin(order_of(dc.words(W32[j])), r.copies))
        if j == r.U - 1:                                     # the all-zero user: any k cuts its one tie group
            users.append(j)
            ks.append(10)
        elif at[0] + (group + 1) // 2 <= K_MAX:
            users.append(j)
            ks.append(int(at[0] + (group + 1) // 2))
    assert len(users) >= 3
    r.users, r.k = np.asarray(users, np.int32), ks
    return r


RANGE_W = 256                                # the narrowest ranges ("deep_chunk_pairs" = 256)


@functools.lru_cache(maxsize=None)
def edge_recipe(E=64, I=1300):
    """C = 4 normal tables with best dishes planted on both sides of every range edge and every segment edge of the index: at every
    position p of perm that starts a segment or a 256-dish range of one, the dishes perm[p - 1] and perm[p] take the row of the dish
    user (p mod U) likes best in their own segment -- so both head their segment's list for that user.  r.edges: the positions."""
    rng = np.random.default_rng(36000 + I)
    r = types.SimpleNamespace(C=4, E=E, I=I, U=6, coef=sd.COEF)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, r.U, I, E)
    RE = r.RE.copy()
    sig = rng.choice([1, 2, 3, 5, 8, 12, 15], I, p=[0.45, 0.3, 0.05, 0.05, 0.05, 0.05, 0.05])
    r.cats = _bits(sig, 4)
    perm, seg_off = index(sig)
    S = host_scores(types.SimpleNamespace(PM=r.PM, RE=r.RE, CE=r.CE, cats=r.cats, coef=r.coef, U=r.U))
    edges = sorted({int(seg_off[s] + r0) for s in range(64) for r0 in range(0, int(seg_off[s + 1] - seg_off[s]), RANGE_W)} - {0})
    for p in edges:
        for q in (p - 1, p):
            d = perm[q]
            seg = perm[seg_off[sig[d]]:seg_off[sig[d] + 1]]
            RE[d] = r.RE[seg[int(np.argmax(S[p % r.U][seg]))]]
    r.RE = RE
    r.edges, r.perm = edges, perm
    r.segment_edges = [p for p in edges if p in set(seg_off.tolist())]               # the others: range edges inside a segment
    r.users = np.asarray(list(range(r.U)) + [4, 1, 1, 0, 5], np.int32)      # 11 rows: blocks of 8 end in a partial one
    return _finish(r)


def edges_listed(out_i, r):
    """the index edges with the planted dish of each side in some list"""
    listed = set(np.asarray(out_i).ravel().tolist())
    return [p for p in r.edges if int(r.perm[p - 1]) in listed and int(r.perm[p]) in listed]


def edge_condition(out_i, r):
    """an edge case has listed dishes on both sides of at least two range edges and two segment edges"""
    seen = edges_listed(out_i, r)
    return len([p for p in seen if p in r.segment_edges]) >= 2 and len([p for p in seen if p not in r.segment_edges]) >= 2


def changed_rows(a, b):
    return (np.asarray(a[1]) != np.asarray(b[1])).any(1)


def short_rows(x):
    return (np.asarray(x[1]) < 0).any(1)
