"""Time the profile calls: the composer alone, and topk_profiles against the topk_users it runs.

Bench-style tables (N(0, 1/E), uniformly random non-empty 0/1 masks), --users rows of Personal_Memory, L = --labels rows of
General_Memory, --nnz labels of weight 1 per request, distinct known users (a guest reads no base row: the known user is the
expensive request).  Everything is resident on the device.  One process, HIP events, warm-up first, the median of the repeats with
[min, max], the forms of a part alternating.

    composer   compose_profiles at n = 2^10 .. 2^20 and each --embed: time, the bytes the call has to move -- n (4 L + 2 * 4 (C + 1) E):
               labels, base row, composed row; General_Memory's L rows are read once and stay in L2 -- and that over the HBM peak
    topk       topk_users(users, k) | compose_profiles | topk_profiles(labels, GM, k, users) over --dishes dishes at --topk-n requests
    --tree T --parts topk_old   topk_users alone from another checkout (the parent commit): the same line, for alternating processes

    python scripts/profiles_time.py
    python scripts/profiles_time.py --tree ../parent --parts topk_old
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parts", nargs="+", default=["composer", "topk"])
    ap.add_argument("--users", type=int, default=1 << 20)
    ap.add_argument("--labels", type=int, default=95)
    ap.add_argument("--nnz", type=int, default=5)
    ap.add_argument("--embed", type=int, nargs="+", default=[64, 128, 200])
    ap.add_argument("--log2n", type=int, nargs="+", default=[10, 12, 14, 16, 18, 20])
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--topk-n", type=int, nargs="+", default=[1 << 10, 1 << 14, 1 << 16])
    ap.add_argument("--topk-embed", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    sys.path.insert(0, root)

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import HBM_PEAK_GBS, random_masks

    dev = torch.device("cuda", 0)
    lib = os.path.join(root, "foodrec_amd", "libm2d.so")
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    stamp = {"tree": os.path.relpath(root, HERE), "git_head": head or None, "libm2d_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest()}
    C, L = 4, a.labels

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fns):
        for fn in fns.values():
            for _ in range(a.warmup):
                once(fn)
        ts = {name: [] for name in fns}
        for _ in range(a.repeats):
            for name, fn in fns.items():
                ts[name].append(once(fn))
        return {name: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)) for name, v in ts.items()}

    def tables(U, E, I, g):
        s = 1.0 / (E ** 0.5)
        return (torch.randn((U, C + 1, E), generator=g, device=dev) * s, torch.randn((I, E), generator=g, device=dev) * s,
                torch.randn((C, E), generator=g, device=dev) * s, torch.randn((L, C + 1, E), generator=g, device=dev) * s)

    def requests(n, U, rng):
        y = np.zeros((n, L), np.float32)
        y[np.arange(n)[:, None], rng.integers(0, L, (n, a.nnz))] = 1.0      # (a repeated draw: one label fewer)
        users = rng.permutation(U)[:n].astype(np.int32) if n <= U else rng.integers(0, U, n).astype(np.int32)
        return torch.from_numpy(y).to(dev), torch.from_numpy(users).to(dev)

    rng = np.random.default_rng(a.seed)
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    if "composer" in a.parts:
        for E in a.embed:
            PM, RE, CE, GM = tables(a.users, E, 16, g)
            eng = foodrec_amd.ScoringEngine(PM, RE, CE)
            for p in a.log2n:
                n = 1 << p
                y, users = requests(n, a.users, rng)
                t = timed({"compose": lambda: eng.compose_profiles(y, GM, users, 0.5)})["compose"]
                eng.check()
                nbytes = n * (4 * L + 2 * 4 * (C + 1) * E)
                gbs = nbytes / (t[0] * 1e-3) / 1e9
                print(json.dumps(dict(stamp, part="composer", E=E, n=n, L=L, nnz=a.nnz, ms=t, bytes=nbytes, gb_per_s=round(gbs, 1),
                                      frac_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))), flush=True)
                del y, users
            eng.close()
            del PM, RE, CE, GM, eng
            torch.cuda.empty_cache()
    if "topk" in a.parts or "topk_old" in a.parts:
        E, I = a.topk_embed, a.dishes
        PM, RE, CE, GM = tables(a.users, E, I, g)
        eng = foodrec_amd.ScoringEngine(PM, RE, CE)
        eng.set_dish_categories(random_masks(torch, I, C, dev, g)[1])
        for n in a.topk_n:
            y, users = requests(n, a.users, rng)
            fns = {"topk_users": lambda: eng.topk_users(users, a.k)}
            if "topk" in a.parts:
                fns["compose"] = lambda: eng.compose_profiles(y, GM, users, 0.5)
                fns["topk_profiles"] = lambda: eng.topk_profiles(y, GM, a.k, users, 0.5)
            t = timed(fns)
            eng.check()
            print(json.dumps(dict(stamp, part="topk", E=E, dishes=I, n=n, k=a.k, ms=t)), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
