"""Time household meal plans, in scripts/plan_time.py's style: bench-style tables (N(0, 1/E), uniformly random
non-empty masks, C = 4), one process, HIP events, warm-up first, the median of the repeats and their range; the calls of a comparison
alternate.  Prints one JSON line per measurement, each with the library's hash and the commit given by --commit.

    groups      _plan_groups(days, k) at M members a group (every slot used, caps per member) against what it could be composed from or
                compared with: _plan_menus on as many users (the M = 1 floor), topk_groups at k = days k (no caps: the scoring, the
                reduction and one deep selection), and -- on --sample groups -- the host workaround, topk_groups(1 024) followed by a
                numpy greedy walk, with its share of rows that are wrong or short
    caps        m2d_group_caps alone: a call with caps per member less the same call with the folded caps per group
    existing    _plan_menus, _topk_menu_filtered and topk_groups alone: runs on the parent too
    trace       --repeats group-plan calls of every shape and nothing else, for `rocprofv3 --kernel-trace --stats -- python
                scripts/plan_groups_time.py --parts trace ...`; --shares <dir> then prints the shares of scoring, reduction, selection
                and merge

    python scripts/plan_groups_time.py --parts groups caps --groups 8192 65536 --members 2 4 --embeds 64 200 --shapes 7x3 16x64
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

GROUPS = (("merge", ("m2d_plan_merge", "m2d_menu_merge")), ("selection", ("m2d_select_deep", "m2d_topk_mlp_select")),
          ("reduction", ("m2d_group_reduce",)), ("scoring", ("m2d_score_slate",)), ("slate vectors", ("m2d_build_slate_vectors",)),
          ("member check and cap fold", ("m2d_group_members", "m2d_group_caps")), ("index and list checks", ("m2d_menu_", "m2d_check_exclusions")))


def shares(out_dir):
    """the kernel trace of a `trace` run -> time per group of kernels and its share"""
    total, per, calls = 0, {}, {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name, ns = r.get("Kernel_Name", ""), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                group = next((g for g, keys in GROUPS if any(key in name for key in keys)), "other: " + name.split("(")[0][:60])
                if "m2d_group_caps" in name:
                    per["m2d_group_caps alone"] = per.get("m2d_group_caps alone", 0) + ns
                    calls["m2d_group_caps alone"] = calls.get("m2d_group_caps alone", 0) + 1
                per[group] = per.get(group, 0) + ns
                calls[group] = calls.get(group, 0) + 1
                total += ns
    for g, ns in sorted(per.items(), key=lambda x: -x[1]):
        print(json.dumps({"part": "shares", "group": g, "launches": calls[g], "ms": round(ns / 1e6, 3), "share": round(ns / max(total, 1), 4)}))


def greedy(ids, sig, cap, days, k, C):
    """the host workaround's walk over one row of listed ids: day caps `cap` per category, no dish twice"""
    left, plan = [int(d) for d in ids if d >= 0], []
    for _ in range(days):
        n, row, rest = [0] * C, [], []
        for d in left:
            cs = [c for c in range(C) if (sig[d] >> c) & 1]
            if len(row) < k and all(n[c] < cap for c in cs):
                row.append(d)
                for c in cs:
                    n[c] += 1
            else:
                rest.append(d)
        plan.append(row + [-1] * (k - len(row)))
        left = rest
    return plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["groups", "caps", "existing"])
    ap.add_argument("--groups", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--table-users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embeds", type=int, nargs="+", default=[64, 200])
    ap.add_argument("--shapes", nargs="+", default=["7x3", "16x64"], help="days x k")
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--sample", type=int, default=128, help="groups the host workaround is walked for")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--shares", default=None, help="summarise the kernel trace under this directory and exit")
    a = ap.parse_args()
    if a.shares:
        return shares(a.shares)

    import time

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks

    lib = os.path.join(os.path.dirname(foodrec_amd.__file__), "libm2d.so")
    stamp = {"lib": hashlib.sha256(open(lib, "rb").read()).hexdigest()[:12], "commit": a.commit}
    dev = torch.device("cuda", 0)
    U, I, C = a.table_users, a.dishes, 4
    has_new = hasattr(foodrec_amd.ScoringEngine, "_plan_groups")
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes]

    def timed(fns):
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in fns}
        for _ in range(a.repeats):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1))
        return {name: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)) for name, v in ts.items()}

    def emit(res, t):
        for name, v in t.items():
            res[name + "_ms"], res[name + "_range_ms"] = v[0], v[1:]
        res.update(stamp)
        print(json.dumps(res), flush=True)

    for E in a.embeds:
        g = torch.Generator(device=dev)
        g.manual_seed(a.seed)
        s = 1.0 / (E ** 0.5)
        PM = torch.randn((U, C + 1, E), generator=g, device=dev) * s
        RE = torch.randn((I, E), generator=g, device=dev) * s
        CE = torch.randn((C, E), generator=g, device=dev) * s
        _, cats = random_masks(torch, I, C, dev, g)
        eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=dev)
        eng.set_dish_categories(cats)
        sig = ((cats != 0).to(torch.int64) << torch.arange(C, device=dev)[None, :]).sum(1).cpu().numpy()
        caps = torch.full((C,), a.cap, dtype=torch.int32, device=dev)
        for nG in a.groups:
            users = torch.randint(0, U, (nG,), generator=g, device=dev, dtype=torch.int32)
            base = {"groups": nG, "dishes": I, "embed": E, "cap": a.cap, "repeats": a.repeats}
            if "existing" in a.parts:
                members = torch.randint(0, U, (nG, 2), generator=g, device=dev, dtype=torch.int32)
                emit(dict(base, part="existing"),
                     timed({"plan_menus_7x3": lambda: eng._plan_menus(users, 7, 3, caps),
                            "plan_menus_16x64": lambda: eng._plan_menus(users, 16, 64, caps),
                            "topk_menu_filtered_k10": lambda: eng._topk_menu_filtered(users, 10, caps),
                            "topk_groups_M2_k21": lambda: eng.topk_groups(members, 21, "least")}))
                eng.check()
            for M in a.members:
                members = torch.randint(0, U, (nG, M), generator=g, device=dev, dtype=torch.int32)
                per_member = caps.reshape(1, 1, C).expand(nG, M, C).contiguous()
                for days, k in shapes:
                    if not has_new:
                        continue
                    L = days * k
                    res = dict(base, members=M, days=days, k=k)
                    plan = lambda: eng._plan_groups(members, days, k, per_member, None, "least", caps_per_member=True)       # noqa: E731
                    if "trace" in a.parts:
                        for _ in range(a.repeats):
                            plan()
                        torch.cuda.synchronize()
                    if "caps" in a.parts:
                        t = timed({"caps_per_member": plan, "caps_per_group": lambda: eng._plan_groups(members, days, k, caps, None, "least")})
                        emit(dict(res, part="caps", group_caps_ms=round(t["caps_per_member"][0] - t["caps_per_group"][0], 3)), t)
                    if "groups" in a.parts:
                        t = timed({"plan_groups": plan, "plan_menus": lambda: eng._plan_menus(users, days, k, caps),
                                   "topk_groups_L": lambda: eng.topk_groups(members, L, "least"),
                                   "topk_groups_1024": lambda: eng.topk_groups(members, 1024, "least")})
                        n = min(a.sample, nG)
                        want = eng._plan_groups(members[:n], days, k, per_member[:n], None, "least", caps_per_member=True)[1].cpu().numpy()
                        listed = eng.topk_groups(members[:n], 1024, "least")[1].cpu().numpy()
                        t0 = time.perf_counter()
                        work = np.asarray([greedy(listed[j], sig, a.cap, days, k, C) for j in range(n)])
                        host_ms = (time.perf_counter() - t0) * 1e3 / n
                        bad = (work != want).reshape(n, -1).any(1)
                        short = ((work < 0) & (want >= 0)).reshape(n, -1).any(1)
                        emit(dict(res, part="groups", plan_groups_over_plan_menus=round(t["plan_groups"][0] / t["plan_menus"][0], 3),
                                  plan_groups_over_topk_groups_L=round(t["plan_groups"][0] / t["topk_groups_L"][0], 3),
                                  workaround_ms=round(t["topk_groups_1024"][0] + host_ms * nG, 1), workaround_host_ms_per_group=round(host_ms, 3),
                                  workaround_sample=n, workaround_wrong_rows=round(float(bad.mean()), 4),
                                  workaround_short_rows=round(float(short.mean()), 4)), t)
                    eng.check()
        eng.close()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
