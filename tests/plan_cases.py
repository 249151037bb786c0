"""Inputs, host restatement and stand-ins of the meal-plan tests (tests/test_plan_cases_cpu.py, tests/test_gpu_plan.py; DESIGN.md section
4.15): m2d_plan_menus, `days` menus of k dishes per user with no dish twice, every day under the day caps and the whole plan under the
plan caps.

The restatement (plan_lists) is the definition as it reads: day d is menu_filtered_cases' walk over the allowed ids less the dishes of
the earlier days, under min(cap, plan cap - used) floored at 0.  merged_plan is the call as the engine computes it: per signature the
first L = days k allowed dishes (in ranges of W with a running list), cursors that persist over the days, day counts that do not, `full`
= day-full | plan-full.  The CPU file asserts that the two agree.  Nothing here imports the engine; recipes are menu_cases' (shared, not
written into)."""
import numpy as np

import deep_cases as dc
import menu_cases as mc
import menu_filtered_cases as mf

NAN_WORD = mc.NAN_WORD
MAX_LIST = 1024                               # include/m2d.h: M2D_PLAN_MAX_LIST
# wrong kernels under the same comparisons, all in the merge
STANDINS = ("cursor_reset", "day_counts_kept", "plan_ignored", "plan_per_day", "lists_of_k", "higher_id", "full_kept")
# (days, k) of the GPU cases: L = 10, 2, 21, 64, 65, 65, 192, 1024, 1024 -- L = 64 / 65 is where the selection changes
SHAPES = ((1, 10), (2, 1), (7, 3), (8, 8), (13, 5), (65, 1), (3, 64), (16, 64), (1024, 1))


def _rows3(plans, wrows, days, k):
    out_w = np.full((len(plans), days, k), NAN_WORD, np.uint32)
    out_i = np.full((len(plans), days, k), -1, np.int64)
    for j, plan in enumerate(plans):
        for d, ids in enumerate(plan):
            if len(ids):
                out_i[j, d, :len(ids)] = ids
                out_w[j, d, :len(ids)] = wrows[j][np.asarray(ids, np.int64)]
    return out_w, out_i


def _tables(caps, plan_caps, n, C):
    caps = np.broadcast_to(np.asarray(caps, np.int64), (n, C))
    plan = None if plan_caps is None else np.broadcast_to(np.asarray(plan_caps, np.int64), (n, C))
    return caps, plan


def day_caps(cap, plan, used):
    """the caps of one day: min(cap, plan - used) floored at 0 (a cap below 0 counts as 0); plan None: the day caps"""
    cap = np.maximum(np.asarray(cap, np.int64), 0)
    return cap if plan is None else np.maximum(np.minimum(cap, np.maximum(np.asarray(plan, np.int64), 0) - used), 0)


def used_by(sig, ids, C):
    """how many of `ids` are in each category"""
    s = np.asarray(sig, np.int64)[np.asarray(ids, np.int64)]
    return ((s[:, None] >> np.arange(C)[None, :]) & 1).sum(0) if len(s) else np.zeros(C, np.int64)


def plan_lists(W32, cats, caps, plan_caps, days, k, lists=None, slate=None, standin=None):
    """THE RESTATEMENT: (score words uint32 [n, days, k], ids int64 [n, days, k]) of the float32 matrix W32 [n, I]: the definition as a
    loop over the days; -1 / NAN_WORD where a day cannot take k dishes."""
    assert standin in (None,) + STANDINS
    if standin is not None:
        return merged_plan(W32, cats, caps, plan_caps, days, k, lists, slate, W=mf.RANGE_W, standin=standin)
    W32 = np.ascontiguousarray(W32, np.float32)
    n, I = W32.shape
    C = np.asarray(cats).shape[1]
    sig = mc.signatures(cats)
    caps, plan = _tables(caps, plan_caps, n, C)
    base, lists, w = mf._base(I, slate), mf._lists(lists, n), dc.words(W32)
    out = []
    for j in range(n):
        allowed = base[~np.isin(base, lists[j])]
        order = mc.order_of(w[j][allowed], allowed)      # removing dishes leaves the order of the rest as it is
        used = np.zeros(C, np.int64)
        rows = []
        for d in range(days):
            row = mc._steps(order, sig[order], day_caps(caps[j], None if plan is None else plan[j], used), k, C) if len(order) else []
            rows.append(row)
            if not row:
                rows += [[] for _ in range(days - d - 1)]    # the same walk again: nothing
                break
            used += used_by(sig, row, C)
            order = order[~np.isin(order, row)]
        out.append(rows)
    return _rows3(out, w, days, k)


def merged_plan(W32, cats, caps, plan_caps, days, k, lists=None, slate=None, W=None, standin=None):
    """The call as the engine computes it.  Stand-ins: `cursor_reset` (every day starts at the heads of the lists: dishes repeat),
    `day_counts_kept` (the day counts are not set back), `plan_ignored`, `plan_per_day` (the plan counts are set back with the day's),
    `lists_of_k` (lists of k instead of days k), `higher_id` (equal scores of two segments go to the higher id), `full_kept` (a
    category full for the day is still full the next day)."""
    W32 = np.ascontiguousarray(W32, np.float32)
    n, I = W32.shape
    C = np.asarray(cats).shape[1]
    sig = mc.signatures(cats)
    caps, plan = _tables(caps, plan_caps, n, C)
    if standin == "plan_ignored":
        plan = None
    base, lists, w = mf._base(I, slate), mf._lists(lists, n), dc.words(W32)
    perm, seg_off = mf.slate_index(sig, I, slate)
    L = k if standin == "lists_of_k" else days * k
    out = []
    for j in range(n):
        X = np.sort(lists[j])
        heads = {}
        for s in range(64):
            seg = perm[seg_off[s]:seg_off[s + 1]]
            if not len(seg):
                continue
            Wr = len(seg) if W is None else W
            cand = np.zeros(0, np.int64)
            for r0 in range(0, len(seg), Wr):
                ids = seg[r0:r0 + Wr]
                both = np.concatenate([cand, ids[~np.isin(ids, X)]])
                cand = mc.order_of(w[j][both], both)[:L]
            heads[s] = cand.tolist()
        cap = caps[j]
        cur = {s: 0 for s in heads}
        cnt, pcnt, full = np.zeros(C, np.int64), np.zeros(C, np.int64), 0
        rows = []
        for d in range(days):
            if standin == "cursor_reset":
                cur = {s: 0 for s in heads}
            if standin != "day_counts_kept":
                cnt[:] = 0
            if standin == "plan_per_day":
                pcnt[:] = 0
            carried = full if standin == "full_kept" else 0
            at_cap = lambda c: cnt[c] >= cap[c] or (plan is not None and pcnt[c] >= plan[j][c])      # noqa: E731
            full = carried | sum(1 << c for c in range(C) if at_cap(c))
            row = []
            while len(row) < k:
                adm = [s for s, h in heads.items() if cur[s] < len(h) and (s & full) == 0]
                if not adm:
                    break
                first = [heads[s][cur[s]] for s in adm]
                s = adm[int(np.argmin(dc.keys(w[j][first], first, higher_id=standin == "higher_id")))]
                row.append(int(heads[s][cur[s]]))
                cur[s] += 1
                for c in range(C):
                    if (s >> c) & 1:
                        cnt[c] += 1
                        pcnt[c] += 1
                        if at_cap(c):
                            full |= 1 << c
            rows.append(row)
        out.append(rows)
    return _rows3(out, w, days, k)


def taken_per_signature(plan_ids, sig):
    """per row of [n, days, k] ids: the most dishes one signature contributes to the plan"""
    out = []
    for row in np.asarray(plan_ids).reshape(len(plan_ids), -1):
        s = np.asarray(sig, np.int64)[row[row >= 0]]
        out.append(int(np.bincount(s, minlength=64).max()) if len(s) else 0)
    return np.asarray(out)


def doubled_workaround(W32, cats, caps, k, lists=None, slate=None):
    """what a caller might try for day 2: positions k .. 2k - 1 of the one-day menu of length 2k under doubled caps"""
    w, i = mf.filtered_lists(W32, cats, 2 * np.asarray(caps, np.int64), 2 * k, lists, slate)
    return w[:, k:], i[:, k:]


def plan_caps_of(n, C, days, k, seed=0, tight=2):
    """plan caps that bind: every user its own in 1 .. max(tight, days k / 4), one category per row left without a bound (days k); a
    plan of two dishes: 1 everywhere"""
    rng = np.random.default_rng(950 + seed + 7 * C + days)
    t = rng.integers(1, max(tight, days * k // 4) + 1, (n, C)).astype(np.int32)
    t[np.arange(n), rng.integers(0, C, n)] = days * k
    return t if days * k > 2 else np.ones((n, C), np.int32)


def differs(a, b):
    return (np.asarray(a[1]).reshape(len(a[1]), -1) != np.asarray(b[1]).reshape(len(b[1]), -1)).any(1)


def same(a, b):
    return np.array_equal(np.asarray(a[1], np.int64), np.asarray(b[1], np.int64)) and np.array_equal(np.asarray(a[0], np.uint32),
                                                                                                      np.asarray(b[0], np.uint32))
