"""Time filtered menu retrieval, in scripts/menu_time.py's style: bench-style tables (N(0, 1/E), uniformly
random non-empty masks, C = 4), one process, HIP events, warm-up first, the median of the repeats and their range; the calls of a
comparison alternate.  Prints one JSON line per measurement, each with the library's hash and the commit given by --commit.

    null        topk_menu_filtered with null filters against topk_menu (the same launches)
    excl        topk_menu_filtered with --excl exclusions per user against the same call without exclusions
    slate       the slate form at every --slates nD against topk_slate at the same nD and k; and the host's wait in the call on an idle
                stream (the slate form's one synchronisation: index passes, copy of 65 words, the wait), wall clock
    workaround  topk_users_deep(1 024, exclude) + the numpy greedy: its time and the rows it gets wrong or short
    existing    topk_menu and topk_users_deep with exclusions alone: runs on a tree without the new call (the parent, for comparison)

    python scripts/menu_filtered_time.py --parts null excl --users 8192 65536 --embeds 64 200 --ks 10 64
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["null", "excl", "slate", "workaround", "existing"])
    ap.add_argument("--users", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--table-users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embeds", type=int, nargs="+", default=[64, 200])
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--excl", type=int, default=200, help="excluded dishes per user")
    ap.add_argument("--slates", type=int, nargs="+", default=[1024, 8192, 65536])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks
    from menu_time import host_greedy

    lib = os.path.join(os.path.dirname(foodrec_amd.__file__), "libm2d.so")
    stamp = {"lib": hashlib.sha256(open(lib, "rb").read()).hexdigest()[:12], "commit": a.commit}
    dev = torch.device("cuda", 0)
    U, I, C = a.table_users, a.dishes, 4
    has_new = hasattr(foodrec_amd.ScoringEngine, "_topk_menu_filtered")

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
        for nU in a.users:
            users = torch.randint(0, U, (nU,), generator=g, device=dev, dtype=torch.int32)
            xids = torch.randint(0, I, (nU, a.excl), generator=g, device=dev, dtype=torch.int32).sort(dim=1).values.reshape(-1).contiguous()
            xoff = (torch.arange(nU + 1, device=dev, dtype=torch.int64) * a.excl).contiguous()      # ascending per user, repeats allowed
            base = {"users": nU, "dishes": I, "embed": E, "cap": a.cap, "repeats": a.repeats}
            for k in a.ks:
                menu = lambda: torch.ops.m2d.topk_menu(eng.id, users, caps, k)                     # noqa: E731
                deep_x = lambda: eng.topk_users_deep(users, k, (xoff, xids))                       # noqa: E731
                if "existing" in a.parts:
                    emit(dict(base, part="existing", k=k, excl=a.excl), timed({"topk_menu": menu, "topk_users_deep_excl": deep_x}))
                if not has_new:
                    continue
                null = lambda: eng._topk_menu_filtered(users, k, caps)                             # noqa: E731
                excl = lambda: eng._topk_menu_filtered(users, k, caps, (xoff, xids))               # noqa: E731
                if "null" in a.parts:
                    t = timed({"topk_menu": menu, "filtered_null": null})
                    emit(dict(base, part="null", k=k, null_over_menu=round(t["filtered_null"][0] / t["topk_menu"][0], 4),
                              inside_menus_range=bool(t["topk_menu"][1] <= t["filtered_null"][0] <= t["topk_menu"][2])), t)
                if "excl" in a.parts:
                    t = timed({"filtered_null": null, "filtered_excl": excl})
                    emit(dict(base, part="excl", k=k, excl=a.excl, excl_over_null=round(t["filtered_excl"][0] / t["filtered_null"][0], 4)), t)
                if "slate" in a.parts:
                    for nD in a.slates:
                        if nD > I or k > nD:
                            continue
                        slate = torch.randperm(I, generator=g, device=dev)[:nD].sort().values.to(torch.int32).contiguous()
                        t = timed({"filtered_slate": lambda: eng._topk_menu_filtered(users, k, caps, None, slate),
                                   "filtered_slate_excl": lambda: eng._topk_menu_filtered(users, k, caps, (xoff, xids), slate),
                                   "topk_slate": lambda: eng.topk_slate(users, slate, k)})
                        waits = []
                        for _ in range(a.repeats):              # the host's wait inside the call on an idle stream, against the catalogue form's
                            w = []
                            for sl in (slate, None):
                                torch.cuda.synchronize()
                                t0 = time.perf_counter()
                                eng._topk_menu_filtered(users[:1], k, caps, None, sl)
                                w.append(1e3 * (time.perf_counter() - t0))
                            waits.append(w)
                        torch.cuda.synchronize()
                        med = np.median(np.asarray(waits), 0)
                        emit(dict(base, part="slate", k=k, nD=nD, excl=a.excl, slate_over_topk_slate=round(t["filtered_slate"][0] / t["topk_slate"][0], 3),
                                  host_in_call_one_user_slate_ms=round(float(med[0]), 3), host_in_call_one_user_catalogue_ms=round(float(med[1]), 3)), t)
                eng.check()
            if "workaround" in a.parts and has_new:
                k = a.ks[0]
                depth = min(1024, I)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, mi = eng._topk_menu_filtered(users, k, caps, (xoff, xids))
                mi = mi.cpu().numpy().astype(np.int64)
                t1 = time.perf_counter()
                _, di = eng.topk_users_deep(users, depth, (xoff, xids))
                di = di.cpu().numpy().astype(np.int64)
                t2 = time.perf_counter()
                wi = host_greedy(di, sig, np.full(C, a.cap, np.int64), k, C)
                t3 = time.perf_counter()
                eng.check()
                differ = (wi != mi).any(1)
                res = dict(base, part="workaround", k=k, excl=a.excl, depth=depth, filtered_with_copy_ms=round(1e3 * (t1 - t0), 1),
                           deep_1024_excl_with_copy_ms=round(1e3 * (t2 - t1), 1), host_greedy_ms=round(1e3 * (t3 - t2), 1),
                           workaround_ms=round(1e3 * (t3 - t1), 1), rows_wrong_or_short=int(differ.sum()),
                           share_wrong_or_short=round(float(differ.mean()), 4), rows_short=int(((wi < 0).any(1) & ~(mi < 0).any(1)).sum()))
                res.update(stamp)
                print(json.dumps(res), flush=True)
        eng.close()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
