"""Time seen-dish filtering under the MLP head: ScoringEngine.topk_users_mlp_excluding and
evaluate_model_full(head=True).

Bench-style tables (N(0, 1/E), uniformly random non-empty masks, benchlib's synthetic head).  One process, HIP events, warm-up
first, the calls alternating, the median of the repeats and their range.  Prints one JSON line.

  --mode topk   new         topk_users_mlp_excluding(users, k, exclude) with --excluded random dishes per user (device CSR, built once)
                plain       the same call without exclusions (topk_users_mlp)
                baseline    the correct composition the public API allowed before: torch expands the id pairs, score_pairs_mlp, the
                            excluded positions set to -inf with torch, torch.topk -- in slices of --baseline-rows users
  --mode eval   evaluate_model_full(head=True) at --users x --dishes: wall time of the whole call (host work included), the rank
                call alone by HIP events, and the base evaluate_model_full on a twin model without a head for scale.  --only-new: one
                call and nothing else (the run to put under rocprofv3 --kernel-trace --stats)

    python scripts/head_seen_time.py --users 1024 --dishes 100000 --embed 128
    python scripts/head_seen_time.py --mode eval --users 64657 --dishes 4548 --embed 32
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("topk", "eval"), default="topk")
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embed", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--excluded", type=int, default=200, help="excluded dishes per user")
    ap.add_argument("--baseline-rows", type=int, default=41, help="users per slice of the baseline (41 x 100 000 pairs: the new call's default chunk)")
    ap.add_argument("--only-new", action="store_true")
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
    U, I, C, E, k, X = a.users, a.dishes, 4, a.embed, a.k, a.excluded
    s = 1.0 / (E ** 0.5)
    PM = torch.randn((U, C + 1, E), generator=g, device=dev) * s
    RE = torch.randn((I, E), generator=g, device=dev) * s
    CE = torch.randn((C, E), generator=g, device=dev) * s
    _, cats = random_masks(torch, I, C, dev, g)
    head = synthetic_head(torch, (C + 1) * E, dev, g)
    rng = np.random.default_rng(a.seed)
    # X distinct dishes per user, ascending (one from each of X strata of the catalogue): the device CSR the calls take as it is
    xid = (rng.integers(0, max(I // max(X, 1), 1), (U, X)) + np.arange(X) * (I // max(X, 1))).astype(np.int32)

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

    res = {"mode": a.mode, "users": U, "dishes": I, "embed": E, "k": k, "excluded": X, "repeats": a.repeats}
    if a.mode == "topk":
        eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=dev)
        eng.set_dish_categories(cats)
        eng.set_mlp_head(*head)
        users = torch.arange(U, dtype=torch.int32, device=dev)
        dishes = torch.arange(I, dtype=torch.int32, device=dev)
        off = torch.arange(U + 1, dtype=torch.int64, device=dev) * X
        ids = torch.from_numpy(xid.reshape(-1)).to(dev)
        xcol = torch.from_numpy(xid.astype(np.int64)).to(dev)

        def new_call():
            return eng.topk_users_mlp_excluding(users, k, (off, ids))

        def plain():
            return eng.topk_users_mlp(users, k)

        def baseline():
            out_s, out_i = [], []
            for u0 in range(0, U, a.baseline_rows):
                rows = users[u0:u0 + a.baseline_rows]
                sc = eng.score_pairs_mlp(rows.repeat_interleave(I), dishes.repeat(rows.numel())).view(rows.numel(), I)
                sc.scatter_(1, xcol[u0:u0 + a.baseline_rows], float("-inf"))
                ts, ti = torch.topk(sc, k, dim=1)
                out_s.append(ts)
                out_i.append(ti.to(torch.int32))
            return torch.cat(out_s), torch.cat(out_i)

        if a.only_new:
            res["new_ms"] = timed({"new": new_call})["new"]
        else:
            t = timed({"new": new_call, "plain": plain, "baseline": baseline})
            for name in t:
                res[name + "_ms"], res[name + "_range_ms"] = t[name][0], t[name][1:]
            res["new_over_plain"] = round(t["new"][0] / t["plain"][0], 3)
            res["new_over_baseline"] = round(t["new"][0] / t["baseline"][0], 3)
            res["rows_with_equal_ids"] = round(float((new_call()[1] == baseline()[1]).all(dim=1).float().mean().item()), 4)
        eng.check()
        res["launches"], res["head_kernel"] = eng.get_option("topk_mlp_launches"), eng.last_kernel()
    else:
        args = types.SimpleNamespace(num_categories=C, num_users=U, embed_size=E, high_level_score_coefficient=0.99)
        model = foodrec_amd.Model(args, PM, RE, CE, None, device=dev)
        model.set_mlp_head(*head)
        cats_h = cats.cpu().numpy()
        d2c = {str(d): cats_h[d].tolist() for d in range(I)}
        test = {str(u): [int(d)] for u, d in enumerate(rng.integers(0, I, U))}
        train = {str(u): xid[u].tolist() for u in range(U)}

        def wall(m, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            foodrec_amd.evaluate_model_full(None, m, test, train, k, d2c, **kw)
            return (time.perf_counter() - t0) * 1e3

        if a.only_new:
            res["head_wall_ms"] = [round(wall(model, head=True), 1)]
        else:
            plain_model = foodrec_amd.Model(args, PM, RE, CE, None, device=dev)
            wall(model, head=True)
            wall(plain_model)
            hw, bw = [], []
            for _ in range(a.repeats):
                hw.append(wall(model, head=True))
                bw.append(wall(plain_model))
            res["head_wall_ms"] = (round(float(np.median(hw)), 1), round(min(hw), 1), round(max(hw), 1))
            res["base_wall_ms"] = (round(float(np.median(bw)), 1), round(min(bw), 1), round(max(bw), 1))
            eng = model.engine
            users = torch.arange(U, dtype=torch.int32, device=dev)
            held = torch.tensor([test[str(u)][0] for u in range(U)], dtype=torch.int32, device=dev)
            off = torch.arange(U + 1, dtype=torch.int64, device=dev) * X
            ids = torch.from_numpy(xid.reshape(-1)).to(dev)
            res["rank_call_ms"] = timed({"rank": lambda: eng.catalogue_rank(users, held, (off, ids), head=True)})["rank"]
            eng.check()
            res["launches"], res["head_kernel"] = eng.get_option("topk_mlp_launches"), eng.last_kernel()
    lib = os.path.join(ROOT, "foodrec_amd", "libm2d.so")
    res["git_head"] = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip() or None
    res["libm2d_sha256"] = hashlib.sha256(open(lib, "rb").read()).hexdigest()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
