"""Time meal plans, in scripts/menu_filtered_time.py's style: bench-style tables (N(0, 1/E), uniformly random
non-empty masks, C = 4), one process, HIP events, warm-up first, the median of the repeats and their range; the calls of a comparison
alternate.  Prints one JSON line per measurement, each with the library's hash and the commit given by --commit.

    plan        _plan_menus(days, k) against THE COMPOSITION IT REPLACES: `days` calls of _topk_menu_filtered, the exclusion CSR grown on
                the device by torch between the calls (the day's ids appended to every row, a -1 replaced by the row's first id of the
                day, rows sorted: ascending with repeats, offsets unchanged in form).  Without plan caps, so the caps need no lowering.
                With --excl 0 the first call of the composition has no exclusions.
    compose     the composition alone: runs on a tree without the new call (the parent, for comparison)
    existing    topk_menu and topk_menu_filtered (with --excl exclusions) alone: runs on the parent too
    trace       --repeats plan calls of every shape and nothing else, for `rocprofv3 --kernel-trace --stats -- python scripts/plan_time.py
                --parts trace ...`; scripts/plan_time.py --shares <dir> then prints the shares of scoring, selection and merge

    python scripts/plan_time.py --parts plan --users 8192 65536 --embeds 64 200 --shapes 7x3 7x10 16x64 --excls 0 200
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
          ("scoring", ("m2d_score_slate",)), ("slate vectors", ("m2d_build_slate_vectors",)),
          ("index and list checks", ("m2d_menu_", "m2d_check_exclusions")))


def shares(out_dir):
    """the kernel trace of a `trace` run -> time per group of kernels and its share"""
    total, per, calls = 0, {}, {}
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name, ns = r.get("Kernel_Name", ""), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                group = next((g for g, keys in GROUPS if any(key in name for key in keys)), "other: " + name.split("(")[0][:60])
                per[group] = per.get(group, 0) + ns
                calls[group] = calls.get(group, 0) + 1
                total += ns
    for g, ns in sorted(per.items(), key=lambda x: -x[1]):
        print(json.dumps({"part": "shares", "group": g, "launches": calls[g], "ms": round(ns / 1e6, 3), "share": round(ns / max(total, 1), 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["plan", "existing"])
    ap.add_argument("--users", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--table-users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embeds", type=int, nargs="+", default=[64, 200])
    ap.add_argument("--shapes", nargs="+", default=["7x3", "7x10", "16x64"], help="days x k")
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 64], help="k of the `existing` part")
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--excls", type=int, nargs="+", default=[0, 200], help="excluded dishes per user")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--shares", default=None, help="summarise the kernel trace under this directory and exit")
    a = ap.parse_args()
    if a.shares:
        return shares(a.shares)

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks

    lib = os.path.join(os.path.dirname(foodrec_amd.__file__), "libm2d.so")
    stamp = {"lib": hashlib.sha256(open(lib, "rb").read()).hexdigest()[:12], "commit": a.commit}
    dev = torch.device("cuda", 0)
    U, I, C = a.table_users, a.dishes, 4
    has_new = hasattr(foodrec_amd.ScoringEngine, "_plan_menus")
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
        caps = torch.full((C,), a.cap, dtype=torch.int32, device=dev)
        for nU in a.users:
            users = torch.randint(0, U, (nU,), generator=g, device=dev, dtype=torch.int32)
            base = {"users": nU, "dishes": I, "embed": E, "cap": a.cap, "repeats": a.repeats}
            for excl in a.excls:
                X0 = torch.randint(0, I, (nU, excl), generator=g, device=dev, dtype=torch.int32).sort(dim=1).values.contiguous()

                def csr(X):
                    m = X.shape[1]
                    return (torch.arange(nU + 1, device=dev, dtype=torch.int64) * m).contiguous(), X.reshape(-1).contiguous()

                x0 = csr(X0) if excl else None
                if "existing" in a.parts and excl == a.excls[-1]:
                    for k in a.ks:
                        emit(dict(base, part="existing", k=k, excl=excl),
                             timed({"topk_menu": lambda: torch.ops.m2d.topk_menu(eng.id, users, caps, k),
                                    "topk_menu_filtered": lambda: eng._topk_menu_filtered(users, k, caps, x0)}))
                for days, k in shapes:
                    def compose():
                        X, rows = X0, []
                        for d in range(days):
                            s_, i_ = eng._topk_menu_filtered(users, k, caps, csr(X) if X.shape[1] else None)
                            rows.append(i_)
                            X = torch.cat([X, torch.where(i_ < 0, i_[:, :1], i_)], 1).sort(dim=1).values
                        return rows

                    plan = lambda: eng._plan_menus(users, days, k, caps, None, x0)                   # noqa: E731
                    res = dict(base, days=days, k=k, excl=excl)
                    if "trace" in a.parts and has_new:
                        for _ in range(a.repeats):
                            plan()
                        torch.cuda.synchronize()
                    if "compose" in a.parts:
                        emit(dict(res, part="compose"), timed({"composition": compose}))
                    if "plan" in a.parts and has_new:
                        t = timed({"composition": compose, "plan": plan})
                        got = plan()[1]
                        same = bool(torch.equal(got, torch.stack(compose(), 1)))                    # the two compute the same ids
                        emit(dict(res, part="plan", plan_over_composition=round(t["plan"][0] / t["composition"][0], 4),
                                  composition_over_days_ms=round(t["composition"][0] / days, 3), same_ids=same), t)
                    eng.check()
        eng.close()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
