"""Inputs, host restatement and stand-ins of the household meal-plan tests (tests/test_plan_group_cases_cpu.py,
tests/test_gpu_plan_groups.py): m2d_plan_groups, m2d_plan_menus for groups of users.

The restatement is a composition of restatements that exist: group_cases.group_words turns member words into group words,
fold_caps turns per-member cap tables into one row per group, plan_cases.plan_lists walks the days.  Nothing here imports the engine
and nothing is written into plan_cases, group_cases or menu_cases."""
import numpy as np

import deep_cases as dc
import group_cases as gc
import menu_cases as mc
import plan_cases as pc

NAN_WORD = pc.NAN_WORD
UNCAPPED = 2 ** 31 - 1
# wrong kernels under the same comparisons: three in the cap fold, three in what the lists are taken from
STANDINS = ("fold_max", "fold_all_slots", "fold_next_group", "member_row", "mode_ignored", "reduce_lists")
SHAPES = ((1, 10), (7, 3), (8, 8), (13, 5), (16, 64))         # L = 10, 21, 64, 65, 1024: the selection changes behind 64
MEMBER_COUNTS = gc.MEMBER_COUNTS
CATALOGUES = gc.LIST_SIZES


def fold_caps(table, members, standin=None):
    """THE FOLD, vectorised: table int [nG, M, C], members int [nG, M] (-1 padding) -> int64 [nG, C], the minimum over each group's
    first cnt[g] slots of max(cap, 0).  Stand-ins: `fold_max` (the maximum), `fold_all_slots` (all M slots), `fold_next_group` (the
    rows of group g + 1; the last group its own)."""
    assert standin in (None, "fold_max", "fold_all_slots", "fold_next_group")
    t = np.maximum(np.asarray(table, np.int64), 0)
    m = np.asarray(members, np.int64)
    nG, M = m.shape
    cnt = gc.counts(m)
    if standin == "fold_next_group":
        t = np.concatenate([t[1:], t[-1:]])
    live = np.arange(M)[None, :] < (M if standin == "fold_all_slots" else cnt[:, None])
    if standin == "fold_max":
        return np.where(live[:, :, None], t, -1).max(1)
    return np.where(live[:, :, None], t, UNCAPPED).min(1)


def fold_caps_loop(table, members):
    """the same as the header words it: a plain loop over groups, real members and categories"""
    out = []
    for g, row in enumerate(members):
        cnt = 0
        while cnt < len(row) and row[cnt] >= 0:
            cnt += 1
        caps = []
        for c in range(len(table[g][0])):
            lo = None
            for j in range(cnt):
                v = max(int(table[g][j][c]), 0)
                lo = v if lo is None or v < lo else lo
            caps.append(lo)
        out.append(caps)
    return np.asarray(out, np.int64)


def negative_caps(table, members, offset=0):
    """what m2d_group_caps may latch: (value, position) of every cap below 0 in a real member's row"""
    t = np.asarray(table, np.int64)
    nG, M, C = t.shape
    cnt = gc.counts(members)
    return [(int(t[g, j, c]), offset + (g * M + j) * C + c) for g in range(nG) for j in range(int(cnt[g])) for c in range(C) if t[g, j, c] < 0]


def spread_caps(group_caps, members, slot="first", filler=0, seed=0):
    """per-member tables int32 [nG, M, C] whose fold is `group_caps` [nG, C]: the binding row stands in ONE used slot -- "first",
    "middle" or "last" -- the other real members hold caps above it, filler slots hold `filler` (0 or a negative cap: they must not
    bind and must not latch)"""
    gcaps = np.asarray(group_caps, np.int64)
    m = np.asarray(members, np.int64)
    nG, M = m.shape
    cnt = gc.counts(m)
    rng = np.random.default_rng(4160 + seed)
    t = np.full((nG, M, gcaps.shape[1]), filler, np.int64)
    for g in range(nG):
        at = {"first": 0, "middle": cnt[g] // 2, "last": cnt[g] - 1}[slot]
        t[g, :cnt[g]] = gcaps[g][None, :] + rng.integers(1, 4, (cnt[g], gcaps.shape[1]))
        t[g, at] = gcaps[g]
    return t.astype(np.int32)


def group_plan(S, members, mode, cats, caps, plan_caps, days, k, per_member=False, lists=None, slate=None, user_base=0, standin=None,
               merged=False):
    """THE RESTATEMENT: (score words uint32 [nG, days, k], ids int64 [nG, days, k]) of m2d_plan_groups over the float32 matrix S
    [U, I] of member words (row u: user user_base + u, column d: dish d).  caps / plan_caps: [nG, C] or [C], with per_member
    [nG, M, C].  merged: plan_cases.merged_plan -- the call as the engine computes it -- instead of plan_lists."""
    assert standin in (None,) + STANDINS
    m = np.asarray(members, np.int64)
    fold = standin if standin in ("fold_max", "fold_all_slots", "fold_next_group") else None
    if per_member:
        caps = fold_caps(caps, m, fold)
        plan_caps = None if plan_caps is None else fold_caps(plan_caps, m, fold)
    if standin == "member_row":                               # the selection reads a member's row, not the reduced one: the last member's
        cnt = gc.counts(m)
        W = np.ascontiguousarray(S, np.float32)[m[np.arange(len(m)), cnt - 1] - user_base]
    else:
        W = gc.group_words(S, m, gc.LEAST if standin == "mode_ignored" else mode, user_base).view(np.float32)
    if standin == "reduce_lists":                             # each member's own list of L first, the reduction over what they list
        return _reduce_lists(S, m, W, cats, caps, plan_caps, days, k, lists, slate, user_base)
    walk = pc.merged_plan if merged else pc.plan_lists
    return walk(W, cats, caps, plan_caps, days, k, lists, slate)


def _reduce_lists(S, m, W, cats, caps, plan_caps, days, k, lists, slate, user_base):
    S = np.ascontiguousarray(S, np.float32)
    nG, I = len(m), S.shape[1]
    C = np.asarray(cats).shape[1]
    caps = np.broadcast_to(np.asarray(caps, np.int64), (nG, C))
    plan = None if plan_caps is None else np.broadcast_to(np.asarray(plan_caps, np.int64), (nG, C))
    base = np.arange(I) if slate is None else np.asarray(slate, np.int64)
    cnt = gc.counts(m)
    out_w, out_i = [], []
    for g in range(nG):
        rows = S[m[g, :cnt[g]] - user_base]
        x = None if lists is None else [lists[g]] * len(rows)
        listed = pc.plan_lists(rows, cats, caps[g], None if plan is None else plan[g], days, k, x, slate)[1]
        own = np.intersect1d(np.unique(listed[listed >= 0]), base)
        if not len(own):
            own = base[:1]
        w, i = pc.plan_lists(W[g:g + 1], cats, caps[g:g + 1], None if plan is None else plan[g:g + 1], days, k,
                             None if lists is None else [lists[g]], own)
        out_w.append(w[0])
        out_i.append(i[0])
    return np.stack(out_w), np.stack(out_i)


def host_workaround(S, members, mode, cats, caps, plan_caps, days, k, depth=1024):
    """what a caller did before: m2d_topk_groups' first `depth` dishes, walked on the host"""
    W = gc.group_words(S, members, mode).view(np.float32)
    ids = dc.key_lists(W, min(depth, W.shape[1]))[1]
    out_w, out_i = [], []
    C = np.asarray(cats).shape[1]
    caps = np.broadcast_to(np.asarray(caps, np.int64), (len(W), C))
    for g in range(len(W)):
        w, i = pc.plan_lists(W[g:g + 1], cats, caps[g:g + 1], None if plan_caps is None else np.broadcast_to(plan_caps, (len(W), C))[g:g + 1],
                             days, k, None, np.sort(ids[g][ids[g] >= 0]))
        out_w.append(w[0])
        out_i.append(i[0])
    return np.stack(out_w), np.stack(out_i)


def binds(W32, cats, caps, plan_caps, days, k, lists=None, slate=None):
    """per row: does some cap bind -- does the plan differ from the plan under no caps at all"""
    C = np.asarray(cats).shape[1]
    free = pc.plan_lists(W32, cats, np.full(C, days * k), None, days, k, lists, slate)
    return pc.differs(pc.plan_lists(W32, cats, caps, plan_caps, days, k, lists, slate), free)


def crosses_a_day(plan_ids):
    """per row: dishes on the second day"""
    i = np.asarray(plan_ids)
    return (i[:, 1:] >= 0).any((1, 2)) if i.shape[1] > 1 else np.zeros(len(i), bool)


def same(a, b, mode=None):
    """ids as integers, scores as words; under MEAN a NaN is compared as a NaN (group_cases.same_words)"""
    if not np.array_equal(np.asarray(a[1], np.int64), np.asarray(b[1], np.int64)):
        return False
    return gc.same_words(a[0], b[0], gc.MEAN if mode == gc.MEAN else gc.LEAST)


def permuted_members(members, seed=0):
    """every group's real members in another order, the first member kept first (the tie rule and the sequential mean hang on the
    order: the cases that use this run on tables where neither shows, and say so)"""
    m = np.asarray(members, np.int32).copy()
    rng = np.random.default_rng(4161 + seed)
    for g, c in enumerate(gc.counts(m)):
        if c > 2:
            m[g, 1:c] = m[g, 1:c][rng.permutation(c - 1)]
    return m


def padded(members, M, fill=-1):
    m = np.asarray(members, np.int32)
    out = np.full((len(m), M), fill, np.int32)
    out[:, :m.shape[1]] = m
    return out


def group_exclusions(W32, cats, caps, k, slate=None, sizes=(0, 1, 65, 300), seed=0):
    """per-group exclusion segments of the given sizes, cycling: a segment starts with the group's own best dishes of the one-day menu
    (so leaving it out shows), the rest drawn at random; ascending"""
    n, I = W32.shape
    rng = np.random.default_rng(4162 + seed + I)
    best = pc.plan_lists(W32, cats, caps, None, 1, k, None, slate)[1][:, 0]
    out = []
    for g in range(n):
        size = min(sizes[g % len(sizes)], I - 1)
        own = [int(d) for d in best[g][best[g] >= 0][:max(size // 2, 1 if size else 0)]][:size]
        rest = rng.choice(np.setdiff1d(np.arange(I), own), size - len(own), replace=False).tolist()
        out.append(np.asarray(sorted(own + rest), np.int64))
    return out


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    ids = np.concatenate([np.asarray(x, np.int64) for x in lists]) if len(lists) and off[-1] else np.zeros(0, np.int64)
    return off, ids.astype(np.int32)


def slate_of(I, nD, seed=0):
    """an ascending slate of nD of I dishes"""
    if nD >= I:
        return np.arange(I, dtype=np.int32)
    return np.sort(np.random.default_rng(4163 + seed + nD).choice(I, nD, replace=False)).astype(np.int32)


def exact_words(r):
    """float32 [U, I]: the exact recipe's member words on the host (menu_cases.host_scores in float32 = in float64)"""
    return mc.host_scores(r, np.float32)
