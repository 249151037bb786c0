"""Time ScoringEngine.topk_users_mlp against the composition the public API allowed before it.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks, benchlib's synthetic head).  Two calls on one engine and the
same users, alternating, each a serial loop without graph capture:
    new        topk_users_mlp(users, k, candidates)
    baseline   exact:      torch expands the nU x I id pairs, score_pairs_mlp, torch.topk -- all pairs at once, and ("baseline_sliced")
                           in slices of --baseline-rows users, which keeps its buffers at the new call's size
               two-stage:  topk_users(users, K1), a torch expansion of the users, score_pairs_mlp, torch.topk
One process, HIP events, warm-up first, the median of the repeats and their range.  Prints one JSON line.

    python scripts/topk_mlp_time.py --users 1024 --dishes 100000 --embed 128
    python scripts/topk_mlp_time.py --users 65536 --dishes 100000 --embed 64 --candidates 64
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embed", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=0)
    ap.add_argument("--chunks", type=int, nargs="*", default=[], help="further topk_mlp_chunk_pairs values to time beside the default")
    ap.add_argument("--baseline-rows", type=int, default=41, help="users per slice of the sliced baseline (41 x 100 000 pairs: the new call's default chunk)")
    ap.add_argument("--only-new", action="store_true", help="time the new call alone (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks
    from benchlib.mlp import synthetic_head

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    U, I, C, E, k, K1 = a.users, a.dishes, 4, a.embed, a.k, a.candidates
    s = 1.0 / (E ** 0.5)
    PM = torch.randn((U, C + 1, E), generator=g, device=dev) * s
    RE = torch.randn((I, E), generator=g, device=dev) * s
    CE = torch.randn((C, E), generator=g, device=dev) * s
    _, cats = random_masks(torch, I, C, dev, g)
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=dev)
    eng.set_dish_categories(cats)
    eng.set_mlp_head(*synthetic_head(torch, (C + 1) * E, dev, g))
    users = torch.arange(U, dtype=torch.int32, device=dev)
    dishes = torch.arange(I, dtype=torch.int32, device=dev)

    def new_call():
        return eng.topk_users_mlp(users, k, K1)

    def baseline_exact(step=None):
        out_s, out_i = [], []
        for u0 in range(0, U, step or U):
            rows = users[u0:u0 + (step or U)]
            uu = rows.repeat_interleave(I)
            dd = dishes.repeat(rows.numel())
            sc = eng.score_pairs_mlp(uu, dd).view(rows.numel(), I)
            ts, ti = torch.topk(sc, k, dim=1)
            out_s.append(ts)
            out_i.append(ti.to(torch.int32))
        return torch.cat(out_s), torch.cat(out_i)

    def baseline_two_stage():
        _, cand = eng.topk_users(users, K1)
        sc = eng.score_pairs_mlp(users.repeat_interleave(K1), cand.reshape(-1)).view(U, K1)
        ts, pos = torch.topk(sc, k, dim=1)
        return ts, torch.gather(cand, 1, pos)

    baseline = baseline_two_stage if K1 else baseline_exact

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
        eng.check()
        return {name: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)) for name, v in ts.items()}

    res = {"users": U, "dishes": I, "embed": E, "k": k, "candidates": K1, "repeats": a.repeats,
           "chunk_pairs": eng.get_option("topk_mlp_chunk_pairs")}
    if a.only_new:
        res["new_ms"], res["launches"], res["head_kernel"] = timed({"new": new_call})["new"][0], eng.get_option("topk_mlp_launches"), eng.last_kernel()
        print(json.dumps(res))
        return
    fns = {"new": new_call, "baseline": baseline}
    if not K1:
        fns["baseline_sliced"] = lambda: baseline_exact(a.baseline_rows)
    t = timed(fns)
    if not K1:
        res["baseline_sliced_ms"], res["baseline_sliced_range_ms"] = t["baseline_sliced"][0], t["baseline_sliced"][1:]
    res["new_ms"], res["new_range_ms"] = t["new"][0], t["new"][1:]
    res["baseline_ms"], res["baseline_range_ms"] = t["baseline"][0], t["baseline"][1:]
    res["new_over_baseline"] = round(t["new"][0] / t["baseline"][0], 3)
    res["launches"] = eng.get_option("topk_mlp_launches")
    res["head_kernel"] = eng.last_kernel()
    res["pairs_per_s"] = round((U * (K1 or I)) / (t["new"][0] * 1e-3), 0)
    # the two agree where torch.topk's order and the engine's are the same: the share of equal id rows, for the record
    ns, ni = new_call()
    bs, bi = baseline()
    res["rows_with_equal_ids"] = round(float((ni == bi).all(dim=1).float().mean().item()), 4)
    for P in a.chunks:
        eng.set_option("topk_mlp_chunk_pairs", P)
        res["new_ms_chunk_%d" % P] = timed({"new": new_call})["new"]
    lib = os.path.join(ROOT, "foodrec_amd", "libm2d.so")
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    res["git_head"] = head or None
    res["libm2d_sha256"] = hashlib.sha256(open(lib, "rb").read()).hexdigest()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
