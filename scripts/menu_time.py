"""Time menu retrieval: topk_menu against (a) topk_users_deep at the same shape -- the same scoring work,
the selection over the same columns in more, shorter launches -- and (b) the host workaround it replaces: topk_users_deep(k = 1 024)
and a numpy greedy over the fetched lists, with the share of rows that workaround gets wrong or short.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks, C = 4).  One process, HIP events, warm-up first, the median of the
repeats and their range; the calls of a comparison alternate.  Prints one JSON line per measurement.
    call       topk_menu (both values of option "menu_select") against topk_users_deep, for --users x --dishes at every --embeds, --ks
    workaround topk_users_deep(1 024) + the numpy greedy under caps of --caps per category: its time (device call, copy, host greedy)
               and the rows that differ from topk_menu's
    trace      a few topk_menu calls and nothing else worth a trace: run it under `rocprofv3 --kernel-trace --stats` and read
               m2d_menu_merge's share of the call's kernels

    python scripts/menu_time.py --parts call --users 8192 65536 --embeds 64 200 --ks 10 64
    python scripts/menu_time.py --parts workaround --users 8192 --caps 1 2 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_greedy(ids, sig, cap, k, C):
    """the workaround's greedy over fetched lists ids [n, depth] (every row under the same caps), vectorised over the rows"""
    import numpy as np
    n, depth = ids.shape
    cnt = np.zeros((n, C), np.int64)
    taken = np.zeros(n, np.int64)
    out = np.full((n, k), -1, np.int64)
    rows = np.arange(n)
    bits = ((np.arange(64)[:, None] >> np.arange(C)[None, :]) & 1).astype(bool)      # [signature, category]
    for p in range(depth):
        d = ids[:, p]
        b = bits[sig[np.maximum(d, 0)]]
        ok = (d >= 0) & (taken < k) & ~(b & (cnt >= cap[None, :])).any(1)
        out[rows[ok], taken[ok]] = d[ok]
        cnt[ok] += b[ok]
        taken[ok] += 1
        if (taken == k).all():
            break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["call", "workaround"])
    ap.add_argument("--users", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--table-users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embeds", type=int, nargs="+", default=[64, 200])
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--caps", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--cap", type=int, default=2, help="the cap per category of the `call` part")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks

    dev = torch.device("cuda", 0)
    U, I, C = a.table_users, a.dishes, 4

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
        for nU in a.users:
            users = torch.randint(0, U, (nU,), generator=g, device=dev, dtype=torch.int32)
            if "call" in a.parts:
                caps = torch.full((C,), a.cap, dtype=torch.int32, device=dev)
                for k in a.ks:
                    def menu(select):
                        eng.set_option("menu_select", select)
                        return torch.ops.m2d.topk_menu(eng.id, users, caps, k)
                    t = timed({"topk_menu_list": lambda: menu(0), "topk_menu_radix": lambda: menu(1),
                               "topk_users_deep": lambda: eng.topk_users_deep(users, k)})
                    eng.set_option("menu_select", 0)
                    eng.check()
                    best = min(("topk_menu_list", "topk_menu_radix"), key=lambda n: t[n][0])
                    spread = t["topk_users_deep"][2] - t["topk_users_deep"][1]
                    res = {"part": "call", "users": nU, "dishes": I, "embed": E, "k": k, "cap": a.cap, "repeats": a.repeats,
                           "segments": int((np.bincount(sig, minlength=64) > 0).sum()), "better_select": best,
                           "menu_over_deep": round(t["topk_menu_list"][0] / t["topk_users_deep"][0], 3),
                           "menu_radix_over_deep": round(t["topk_menu_radix"][0] / t["topk_users_deep"][0], 3)}
                    d = t["topk_menu_list"][0] - t["topk_users_deep"][0]
                    res["verdict"] = "faster" if -d > spread else "SLOWER" if d > spread else "within topk_users_deep's spread"
                    for name, v in t.items():
                        res[name + "_ms"], res[name + "_range_ms"] = v[0], v[1:]
                    print(json.dumps(res), flush=True)
            if "workaround" in a.parts:
                k = a.ks[0]
                depth = min(1024, I)
                for cap in a.caps:
                    caps = torch.full((C,), cap, dtype=torch.int32, device=dev)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ms, mi = torch.ops.m2d.topk_menu(eng.id, users, caps, k)
                    mi = mi.cpu().numpy().astype(np.int64)
                    t1 = time.perf_counter()
                    _, di = eng.topk_users_deep(users, depth)
                    di = di.cpu().numpy().astype(np.int64)
                    t2 = time.perf_counter()
                    wi = host_greedy(di, sig, np.full(C, cap, np.int64), k, C)
                    t3 = time.perf_counter()
                    eng.check()
                    differ = (wi != mi).any(1)
                    print(json.dumps({"part": "workaround", "users": nU, "dishes": I, "embed": E, "k": k, "cap": cap, "depth": depth,
                                      "topk_menu_with_copy_ms": round(1e3 * (t1 - t0), 1), "deep_1024_with_copy_ms": round(1e3 * (t2 - t1), 1),
                                      "host_greedy_ms": round(1e3 * (t3 - t2), 1), "workaround_ms": round(1e3 * (t3 - t1), 1),
                                      "rows_wrong_or_short": int(differ.sum()), "share_wrong_or_short": round(float(differ.mean()), 4),
                                      "rows_short": int(((wi < 0).any(1) & ~(mi < 0).any(1)).sum())}), flush=True)
            if "trace" in a.parts:
                caps = torch.full((C,), a.cap, dtype=torch.int32, device=dev)
                for _ in range(3):
                    torch.ops.m2d.topk_menu(eng.id, users, caps, a.ks[0])
                torch.cuda.synchronize()
                eng.check()
                print(json.dumps({"part": "trace", "users": nU, "embed": E, "k": a.ks[0], "calls": 3}), flush=True)
        eng.close()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
