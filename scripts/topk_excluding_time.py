"""Time ScoringEngine.topk_users_excluding against topk_users(k = K1) and catalogue_rank on the same engine and users.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks).  Three exclusion patterns:
    random20   20 uniformly random ids per user            -- practically nobody short: the first tier and its filter
    own16      every user's own unfiltered top 16          -- every user short: the exact scan alone
    own50of100 50 ids drawn from the user's own top 100    -- the mixture a trained model produces
One process, HIP events, warm-up first, the median of the repeats.  Prints one JSON line.

    python scripts/topk_excluding_time.py --users 65536 --dishes 100000 --embed 64 [--k 10] [--repeats 20]
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
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embed", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    U, I, C, E, k = a.users, a.dishes, 4, a.embed, a.k
    K1 = 10 if E == 128 else 16
    s = 1.0 / (E ** 0.5)
    PM = torch.randn((U, C + 1, E), generator=g, device=dev) * s
    RE = torch.randn((I, E), generator=g, device=dev) * s
    CE = torch.randn((C, E), generator=g, device=dev) * s
    _, cats = random_masks(torch, I, C, dev, g)
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=dev)
    eng.set_dish_categories(cats)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    items = torch.randint(0, I, (U,), generator=g, device=dev, dtype=torch.int32)

    def csr(ids2d):                                         # [U, n] device ids -> ascending segments of n
        ids2d = torch.sort(ids2d.to(torch.int32), dim=1).values.contiguous()
        off = torch.arange(U + 1, dtype=torch.int64, device=dev) * ids2d.shape[1]
        return off, ids2d.reshape(-1)

    # the user's own top 112: the unfiltered top 64, then three times the next 16 with what is known so far excluded
    _, top = eng.topk_users(users, 64)
    for _ in range(3):
        _, nxt = eng.topk_users_excluding(users, 16, csr(top))
        top = torch.cat([top, nxt], dim=1)
    eng.check()
    pick = torch.argsort(torch.rand((U, 100), generator=g, device=dev), dim=1)[:, :50]
    cases = {"random20": csr(torch.randint(0, I, (U, 20), generator=g, device=dev, dtype=torch.int32)),
             "own16": csr(top[:, :16]),
             "own50of100": csr(torch.gather(top[:, :100], 1, pick))}

    out_s = torch.empty((U, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((U, k), dtype=torch.int32, device=dev)
    k1_s = torch.empty((U, K1), dtype=torch.float32, device=dev)
    k1_i = torch.empty((U, K1), dtype=torch.int32, device=dev)
    ranks = torch.empty(U, dtype=torch.int32, device=dev)
    scores = torch.empty(U, dtype=torch.float32, device=dev)

    # the CSR is built once outside the timed region: the call itself (launches) is what is timed
    def excl_call(off, ids):
        def fn():
            rc = _native.lib().m2d_topk_users_excluding(eng._h, users.data_ptr(), U, k, off.data_ptr(), ids.data_ptr(), out_s.data_ptr(),
                                                        out_i.data_ptr(), _stream_ptr())
            _native.raise_for(rc, eng._h)
        return fn

    def topk_call():
        eng.topk_users_into(users, K1, k1_s, k1_i)

    def rank_call():
        rc = _native.lib().m2d_catalogue_rank(eng._h, users.data_ptr(), items.data_ptr(), U, None, None, ranks.data_ptr(),
                                              scores.data_ptr(), _stream_ptr())
        _native.raise_for(rc, eng._h)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        eng.check()
        return float(np.median(ts))

    res = {"users": U, "dishes": I, "embed": E, "k": k, "K1": K1,
           "topk_K1_ms": round(timed(topk_call), 4), "rank_ms": round(timed(rank_call), 4)}
    for name, (off, ids) in cases.items():
        res[name + "_ms"] = round(timed(excl_call(off, ids)), 4)
        res[name + "_short"] = eng.get_option("topk_excl_short")
        res[name + "_tiles_scanned"] = eng.get_option("topk_excl_tiles_scanned")
    res["random20_over_topk"] = round(res["random20_ms"] / res["topk_K1_ms"], 3)
    res["own16_over_rank"] = round(res["own16_ms"] / res["rank_ms"], 3)
    lib = os.path.join(ROOT, "foodrec_amd", "libm2d.so")
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    res["git_head"] = head or None
    res["libm2d_sha256"] = hashlib.sha256(open(lib, "rb").read()).hexdigest()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
