"""Time ScoringEngine.topk_markets -- one (user, market) per request, one call per batch -- against the only other way to answer the
same requests: a host loop of topk_market(users[q:q+1], market_q, k, max_missing).

Bench-style tables (N(0, 1/E), uniformly random non-empty masks), --users distinct users, recipe lists of 5 .. 15 entries over
--ingredients ids, one market per request holding a share of the ingredients, drawn per request.  Markets and users are resident on
the device in both forms (the upload is the same bytes either way).  On one engine, alternating:
    new        topk_markets(users[:nQ], (offsets, ids), k, max_missing, return_counts=True)
    baseline   for q in range(nQ): topk_market(users[q:q+1], market_q, k, max_missing)      (synchronises once per request, as it must)
The baseline loop is timed over at most --base-cap requests and scaled to nQ (`base_extrapolated`): its cost per request does not depend
on how many follow.  One process, HIP events, warm-up first, the median of the repeats and their range; a call whose warm-up took more
than --slow-ms is repeated --slow-repeats times only.  Prints one JSON line per (dishes, share, tolerance, nQ).

    python scripts/market_requests_time.py --dishes 100000 1000000 --shares 0.1 0.5 0.9 --max-missing 0 2 --requests 1 64 1024 16384
    python scripts/market_requests_time.py --dishes 1000000 --shares 0.5 --max-missing 0 --requests 1024 --only-new   (under rocprofv3 --kernel-trace --stats)
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
    ap.add_argument("--requests", type=int, nargs="+", default=[1, 64, 1024, 16384])
    ap.add_argument("--embed", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--base-cap", type=int, default=64)
    ap.add_argument("--slow-ms", type=float, default=400.0)
    ap.add_argument("--slow-repeats", type=int, default=3)
    ap.add_argument("--market-shares", type=int, default=0, help="option market_shares (0 = the launcher's rule)")
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
    nmax = max(a.requests)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fns):
        """The calls of `fns` alternating: name -> (median ms, min, max, repeats)."""
        slow = False
        for fn in fns.values():
            for _ in range(a.warmup):
                slow = once(fn) > a.slow_ms or slow
                if slow:
                    break
        reps = a.slow_repeats if slow else a.repeats
        ts = {name: [] for name in fns}
        for _ in range(reps):
            for name, fn in fns.items():
                ts[name].append(once(fn))
        return {name: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)) for name, v in ts.items()}, reps

    rng = np.random.default_rng(a.seed)
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
        eng.set_option("market_shares", a.market_shares)
        users = torch.randperm(U, generator=g, device=dev).to(torch.int32)[:nmax].contiguous()
        lens = rng.integers(5, 16, I)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ids = rng.integers(0, R, int(off[-1])).astype(np.int32)
        eng.set_recipes(off, ids, R)
        nnz = int(off[-1])
        for share in a.shares:
            m = int(round(share * R))
            # one market per request: the first m of a permutation each (argsort of uniform draws, a block of requests at a time)
            mids = torch.cat([torch.rand((min(1024, nmax - b), R), generator=g, device=dev).argsort(1)[:, :m].to(torch.int32).reshape(-1)
                              for b in range(0, nmax, 1024)])
            moff = torch.arange(nmax + 1, device=dev, dtype=torch.int64) * m
            rows = mids.reshape(nmax, m)
            for mm in a.max_missing:
                for nQ in a.requests:
                    uq, oq, iq = users[:nQ], moff[:nQ + 1], mids[:nQ * m]
                    new = lambda: eng.topk_markets(uq, (oq, iq), k, mm, return_counts=True)
                    nb = min(nQ, a.base_cap)

                    def base():
                        return [eng.topk_market(users[q:q + 1], rows[q], k, mm) for q in range(nb)]

                    s_new, i_new, c_new = new()
                    ref = base()
                    eng.check()
                    for q in range(nb):                      # the same requests, the same dishes (scores: another arithmetic, within 1e-4)
                        assert int(c_new[q]) == ref[q][2], "counts differ at request %d" % q
                    fns = {"new": new} if a.only_new else {"new": new, "base": base}
                    t, reps = timed(fns)
                    eng.check()
                    counts = c_new.cpu().numpy()
                    res = {"users": U, "dishes": I, "ingredients": R, "entries": nnz, "share": share, "max_missing": mm, "requests": nQ,
                           "cookable_mean": round(float(counts.mean()), 1), "cookable_max": int(counts.max()), "embed": E, "k": k,
                           "repeats": reps, "kernel": "m2d_markets_topk_lds" if R <= 65536 else "m2d_markets_topk_l2",
                           "shares_used": eng.get_option("market_shares_used"), "walk_l2_bytes_per_request": 4 * nnz + 8 * I}
                    new()
                    res["shares_used"] = eng.get_option("market_shares_used")
                    res["new_ms"], res["new_range_ms"] = t["new"][0], t["new"][1:]
                    res["new_us_per_request"] = round(1e3 * t["new"][0] / nQ, 2)
                    if not a.only_new:
                        f = nQ / nb
                        b0 = t["base"]
                        res["base_requests_timed"], res["base_extrapolated"] = nb, nb < nQ
                        res["base_ms"], res["base_range_ms"] = round(b0[0] * f, 3), (round(b0[1] * f, 3), round(b0[2] * f, 3))
                        res["base_us_per_request"] = round(1e3 * b0[0] / nb, 2)
                        res["speedup"] = round(b0[0] * f / t["new"][0], 2)
                        # the new call's median below the baseline's by more than the two ranges together
                        res["clear"] = bool(b0[0] * f - t["new"][0] > (b0[2] - b0[1]) * f + (t["new"][2] - t["new"][1]))
                    res.update(stamp)
                    print(json.dumps(res), flush=True)
            del mids, moff, rows
        eng.close()
        del PM, RE, CE, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
