"""Time ScoringEngine.topk_markets_excluding -- market requests that leave out what the shopper has had and name what to buy
 -- against the call it extends and against the host workaround it replaces.

Workload of scripts/market_requests_time.py: bench-style tables (N(0, 1/E), uniformly random non-empty masks), --users distinct users,
recipe lists of 5 .. 15 entries over --ingredients ids, one market per request holding --share of the ingredients.  Everything is
resident on the device.  The forms, alternating on one engine:
    old          topk_markets(users, markets, k, max_missing, return_counts=True)                      (also on a tree without the new call)
    null         topk_markets_excluding(users, markets, None, k, max_missing, return_counts=True)      the same kernels through the new entry
    excl         ... with --history excluded dishes per request                                         lists only
    excl_missing ... and return_missing=True (max_missing > 0)                                           lists and what to buy
    workaround   topk_markets at k = 64, the rows copied to the host, the excluded ids filtered there, the first k kept, and (max_missing
                 > 0) each listed dish's recipe list re-walked against the request's market in numpy
A shopper's history: "random" -- --history dishes drawn uniformly from the catalogue --, or "favourites" -- the shopper's
--favourites best cookable dishes at that market and random dishes up to --history.  `workaround_wrong` is the share of requests
whose workaround ids differ from the call's.  One process, HIP events (the workaround's host work lies between its two events), warm-up
first, the median of the repeats and their range.  --tree imports the package from another checkout (forms: old only there).

    python scripts/market_excluding_time.py --dishes 100000 1000000 --requests 64 256 1024
    python scripts/market_excluding_time.py --tree ../parent --forms old
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
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--ingredients", type=int, default=10000)
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--max-missing", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--requests", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--history", type=int, default=200)
    ap.add_argument("--favourites", type=int, default=60)
    ap.add_argument("--models", nargs="+", default=["random", "favourites"])
    ap.add_argument("--forms", nargs="+", default=["old", "null", "excl", "excl_missing", "workaround"])
    ap.add_argument("--embed", type=int, default=64)
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
    from benchlib.common import random_masks

    dev = torch.device("cuda", 0)
    lib = os.path.join(root, "foodrec_amd", "libm2d.so")
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    stamp = {"tree": os.path.relpath(root, HERE), "git_head": head or None, "libm2d_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest()}
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
        for fn in fns.values():
            for _ in range(a.warmup):
                once(fn)
        ts = {name: [] for name in fns}
        for _ in range(a.repeats):
            for name, fn in fns.items():
                ts[name].append(once(fn))
        return {name: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)) for name, v in ts.items()}

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
        has_new = hasattr(eng, "topk_markets_excluding")
        users = torch.randperm(U, generator=g, device=dev).to(torch.int32)[:nmax].contiguous()
        lens = rng.integers(5, 16, I)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ids = rng.integers(0, R, int(off[-1])).astype(np.int32)
        eng.set_recipes(off, ids, R)
        m = int(round(a.share * R))
        mids = torch.cat([torch.rand((min(1024, nmax - b), R), generator=g, device=dev).argsort(1)[:, :m].to(torch.int32).reshape(-1)
                          for b in range(0, nmax, 1024)])
        moff = torch.arange(nmax + 1, device=dev, dtype=torch.int64) * m
        markets_host = mids.reshape(nmax, m).cpu().numpy()
        for mm in a.max_missing:
            histories = {}
            if has_new and {"excl", "excl_missing", "workaround"} & set(a.forms):
                best = eng.topk_markets(users, (moff, mids), 64, mm)[1].cpu().numpy()
                for model in a.models:
                    lists = []
                    for q in range(nmax):
                        fav = best[q][best[q] >= 0][:a.favourites] if model == "favourites" else np.zeros(0, np.int64)
                        lists.append(np.unique(np.concatenate([fav, rng.integers(0, I, a.history - len(fav))])))
                    histories[model] = lists
            for nQ in a.requests:
                uq, oq, iq = users[:nQ], moff[:nQ + 1], mids[:nQ * m]
                res = {"users": U, "dishes": I, "ingredients": R, "share": a.share, "max_missing": mm, "requests": nQ, "embed": E, "k": k,
                       "repeats": a.repeats}
                fns = {}
                if "old" in a.forms:
                    fns["old"] = lambda: eng.topk_markets(uq, (oq, iq), k, mm, return_counts=True)
                if has_new and "null" in a.forms:
                    fns["null"] = lambda: eng.topk_markets_excluding(uq, (oq, iq), None, k, mm, return_counts=True)
                t = timed(fns) if fns else {}
                res["shares_used"] = eng.get_option("market_shares_used")
                for model, lists in histories.items():
                    lq = lists[:nQ]
                    xo = np.zeros(nQ + 1, np.int64)
                    np.cumsum([len(x) for x in lq], out=xo[1:])
                    xoff, xids = torch.from_numpy(xo).to(dev), torch.from_numpy(np.concatenate(lq).astype(np.int32)).to(dev)
                    sets = [set(x.tolist()) for x in lq]
                    f2 = {}
                    if "excl" in a.forms:
                        f2["excl"] = lambda: eng.topk_markets_excluding(uq, (oq, iq), (xoff, xids), k, mm, return_counts=True)
                    if "excl_missing" in a.forms and mm > 0:
                        f2["excl_missing"] = lambda: eng.topk_markets_excluding(uq, (oq, iq), (xoff, xids), k, mm, return_counts=True, return_missing=True)

                    def workaround():
                        i64 = eng.topk_markets(uq, (oq, iq), 64, mm)[1].cpu().numpy()
                        out = np.full((nQ, k), -1, np.int64)
                        miss = np.full((nQ, k, max(mm, 1)), -1, np.int64)
                        present = np.zeros(R, bool)
                        for q in range(nQ):
                            keep = [d for d in i64[q].tolist() if d >= 0 and d not in sets[q]][:k]
                            out[q, :len(keep)] = keep
                            if mm > 0:
                                present[:] = False
                                present[markets_host[q]] = True
                                for j, d in enumerate(keep):
                                    seg = ids[off[d]:off[d + 1]]
                                    ab = seg[~present[seg]][:mm]
                                    miss[q, j, :len(ab)] = ab
                        return out, miss

                    if "workaround" in a.forms:
                        f2["workaround"] = workaround
                    if not f2:
                        continue
                    t2 = timed(f2)
                    for name, v in t2.items():
                        res["%s_%s_ms" % (model, name)], res["%s_%s_range_ms" % (model, name)] = v[0], v[1:]
                    if "workaround" in f2 and ("excl_missing" in f2 or "excl" in f2):
                        got = f2["excl_missing" if "excl_missing" in f2 else "excl"]()
                        w_ids, w_miss = workaround()
                        new_ids = got[1].cpu().numpy()
                        wrong = (w_ids != new_ids).any(1)
                        res["%s_workaround_wrong" % model] = round(float(wrong.mean()), 4)
                        if "excl_missing" in f2:                # where the ids agree the host re-walk names the same entries
                            assert np.array_equal(w_miss[~wrong], got[3].cpu().numpy()[~wrong]), "missing entries differ from the host re-walk"
                        res["%s_excluded_mean" % model] = round(float(np.mean([len(x) for x in lq])), 1)
                        res["%s_left_mean" % model] = round(float(got[2].cpu().numpy().mean()), 1)
                eng.check()
                for name, v in t.items():
                    res["%s_ms" % name], res["%s_range_ms" % name] = v[0], v[1:]
                res.update(stamp)
                print(json.dumps(res), flush=True)
        eng.close()
        del PM, RE, CE, eng, mids, moff
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
