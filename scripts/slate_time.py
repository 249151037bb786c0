"""Time ScoringEngine.score_slate / topk_slate against what the public API offered before them.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks), nU distinct users, a slate of nD ascending dish ids drawn from a
catalogue of --dishes.  On one engine, alternating, each a serial loop without graph capture:
    new        score_slate(users, slate)                      topk_slate(users, slate, k)
    baseline   a torch expansion of the nU x nD id pairs plus score_pairs_bydish -- with torch.topk on top for the lists -- all pairs
               at once, and ("sliced") in slices of max(1, 2^22 / nD) users, which keeps its buffers at the new call's scratch size
One process, HIP events, warm-up first, the median of the repeats and their range.  Prints one JSON line per (embed, slate size):
executed flops = 2 K nU nD over the new score call's time, against the 157.3 TF f32 MFMA peak and the 122 TF of an untuned tiled kernel.

    python scripts/slate_time.py --users 65536 --slates 64 1024 8192 --embeds 64 128 200
    python scripts/slate_time.py --users 65536 --slates 1024 --embeds 64 --only-new       (the run to put under rocprofv3 --kernel-trace --stats)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF, UNTUNED_TF = 157.3, 122.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--slates", type=int, nargs="+", default=[64, 1024, 8192])
    ap.add_argument("--embeds", type=int, nargs="+", default=[64, 128, 200])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks

    dev = torch.device("cuda", 0)
    lib = os.path.join(ROOT, "foodrec_amd", "libm2d.so")
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    stamp = {"git_head": head or None, "libm2d_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest()}
    U, I, C, k = a.users, a.dishes, 4, a.k

    def timed(fns):
        """The calls of `fns` alternating: name -> (median ms, min, max)."""
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
        users = torch.randperm(U, generator=g, device=dev).to(torch.int32)
        for nD in a.slates:
            slate = torch.sort(torch.randperm(I, generator=g, device=dev)[:nD])[0].to(torch.int32)
            rows = max(1, (1 << 22) // nD)

            def base_scores(step=None):
                out = []
                for u0 in range(0, U, step or U):
                    r = users[u0:u0 + (step or U)]
                    out.append(eng.score_pairs_bydish(r.repeat_interleave(nD), slate.repeat(r.numel())).view(r.numel(), nD))
                return out

            def base_lists(step=None):
                out = []
                for sc in base_scores(step):
                    ts, pos = torch.topk(sc, k, dim=1)
                    out.append((ts, slate[pos]))
                return out

            fns = {"score_new": lambda: eng.score_slate(users, slate), "topk_new": lambda: eng.topk_slate(users, slate, k)}
            if not a.only_new:
                fns.update({"score_base": base_scores, "score_base_sliced": lambda: base_scores(rows),
                            "topk_base": base_lists, "topk_base_sliced": lambda: base_lists(rows)})
            t = timed(fns)
            eng.check()
            res = {"users": U, "dishes": I, "slate": nD, "embed": E, "k": k, "repeats": a.repeats, "kernel": None, "sliced_rows": rows}
            eng.score_slate(users[:1], slate)
            res["kernel"] = eng.last_kernel()
            for name, v in t.items():
                res[name + "_ms"], res[name + "_range_ms"] = v[0], v[1:]
            tf = 2.0 * (C + 1) * E * U * nD / (t["score_new"][0] * 1e-3) / 1e12
            res["score_new_tflops"] = round(tf, 2)
            res["share_of_f32_mfma_peak"] = round(tf / PEAK_TF, 3)
            res["share_of_untuned_tiled"] = round(tf / UNTUNED_TF, 3)
            res["score_new_gpairs_per_s"] = round(U * nD / (t["score_new"][0] * 1e-3) / 1e9, 2)
            if not a.only_new:
                for what in ("score", "topk"):
                    best = min(t[what + "_base"], t[what + "_base_sliced"])
                    new = t[what + "_new"]
                    res[what + "_speedup"] = round(best[0] / new[0], 2)
                    # the new call's median below the baseline's by more than the two ranges together
                    res[what + "_clear"] = bool(best[0] - new[0] > (best[2] - best[1]) + (new[2] - new[1]))
                got = eng.score_slate(users[:256], slate)
                ref = eng.score_pairs_bydish(users[:256].repeat_interleave(nD), slate.repeat(min(256, U))).view(-1, nD)
                res["max_abs_diff_vs_bydish"] = float((got - ref).abs().max().item())
            res.update(stamp)
            print(json.dumps(res), flush=True)
        eng.close()
        del PM, RE, CE, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
