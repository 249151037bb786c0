"""Time ScoringEngine.cookable_dishes / topk_market against the same result from torch on the device.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks), --users distinct users, recipe lists of 5 .. 15 entries (10 on
average) over --ingredients ids, a market holding a share of the ingredients.  On one engine, alternating, each a serial loop without
graph capture, the market uploaded from the host inside the timed call in both:
    new        cookable_dishes(market, max_missing)            topk_market(users, market, k, max_missing)
    baseline   torch on the device: a bool table of the market indexed by the resident ids, index_add_ of the absent flags into a
               per-dish sum, nonzero -- followed by topk_slate(users, that list, k) for the composed call
    parts      of the new call, timed in the same alternation (in this order: cook new, topk new, upload, cook_resident,
               cook_resident_into, cook base, topk base -- so `cook new` and `upload` stand behind a slate call, the other two do not):
               the market's upload alone; cookable_dishes on a resident market; the same into a caller-owned id buffer
One process, HIP events, warm-up first, the median of the repeats and their range.  Prints one JSON line per (dishes, share, tolerance).

    python scripts/market_time.py --dishes 100000 1000000 --shares 0.1 0.5 0.9 --max-missing 0 2
    python scripts/market_time.py --dishes 100000 --shares 0.5 --max-missing 0 --only-new   (the run to put under rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--ingredients", type=int, default=10000)
    ap.add_argument("--shares", type=float, nargs="+", default=[0.1, 0.5, 0.9])
    ap.add_argument("--max-missing", type=int, nargs="+", default=[0, 2])
    ap.add_argument("--embed", type=int, default=64)
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
    U, C, E, R, k = a.users, 4, a.embed, a.ingredients, a.k

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

    for I in a.dishes:
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
        rng = np.random.default_rng(a.seed)
        lens = rng.integers(5, 16, I)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ids = rng.integers(0, R, int(off[-1])).astype(np.int32)
        eng.set_recipes(off, ids, R)
        # the baseline's resident arrays: the ids as an index, every entry's dish, the list lengths
        ids64 = torch.from_numpy(ids.astype(np.int64)).to(dev)
        seg = torch.repeat_interleave(torch.arange(I, device=dev), torch.from_numpy(lens).to(dev))
        nonempty = torch.from_numpy(lens > 0).to(dev)
        for share in a.shares:
            market = rng.permutation(R)[:int(round(share * R))].astype(np.int32)          # host: uploaded inside every timed call
            for mm in a.max_missing:
                def base_cook():
                    present = torch.zeros(R, dtype=torch.bool, device=dev)
                    present[torch.from_numpy(market).to(dev).long()] = True
                    miss = torch.zeros(I, dtype=torch.int32, device=dev).index_add_(0, seg, (~present[ids64]).to(torch.int32))
                    return torch.nonzero(nonempty & (miss <= mm)).squeeze(1).to(torch.int32)

                def base_topk():
                    slate = base_cook()
                    return eng.topk_slate(users, slate, min(k, slate.numel())) if slate.numel() else None

                new_cook = lambda: eng.cookable_dishes(torch.from_numpy(market).to(dev), mm)
                new_topk = lambda: eng.topk_market(users, torch.from_numpy(market).to(dev), k, mm)
                got, want = new_cook(), base_cook()
                assert torch.equal(got, want), "the two lists differ"
                # the new call's parts: the market's upload alone; the call on a market that is already resident; and that call
                # into a buffer of the caller's (no allocation inside it)
                resident = torch.from_numpy(market).to(dev)
                ids_buf = torch.empty(I, dtype=torch.int32, device=dev)
                fns = {"cook_new": new_cook, "topk_new": new_topk, "upload": lambda: torch.from_numpy(market).to(dev),
                       "cook_resident": lambda: eng.cookable_dishes(resident, mm),
                       "cook_resident_into": lambda: eng.cookable_dishes(resident, mm, out_ids=ids_buf)}
                if not a.only_new:
                    fns.update({"cook_base": base_cook, "topk_base": base_topk})
                t = timed(fns)
                eng.check()
                new_cook()
                res = {"users": U, "dishes": I, "ingredients": R, "entries": int(off[-1]), "share": share, "max_missing": mm, "cookable": int(got.numel()),
                       "embed": E, "k": k, "repeats": a.repeats, "kernel": eng.last_kernel()}
                for name, v in t.items():
                    res[name + "_ms"], res[name + "_range_ms"] = v[0], v[1:]
                if not a.only_new:
                    for what in ("cook", "topk"):
                        base, new = t[what + "_base"], t[what + "_new"]
                        res[what + "_speedup"] = round(base[0] / new[0], 2)
                        # the new call's median below the baseline's by more than the two ranges together
                        res[what + "_clear"] = bool(base[0] - new[0] > (base[2] - base[1]) + (new[2] - new[1]))
                res.update(stamp)
                print(json.dumps(res), flush=True)
        eng.close()
        del PM, RE, CE, eng, ids64, seg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
