"""Time ScoringEngine.catalogue_rank against the default topk_users(k=10) on the same engine and users.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks), one uniformly random held-out dish per user.  One process,
HIP events, warm-up first, the median of the repeats.  Prints one JSON line.

    python scripts/rank_time.py --users 65536 --dishes 100000 --embed 64 [--excl 20] [--repeats 20]
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
    ap.add_argument("--excl", type=int, default=0, help="excluded ids per query (uniformly random)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    U, I, C, E = a.users, a.dishes, 4, a.embed
    s = 1.0 / (E ** 0.5)
    PM = torch.randn((U, C + 1, E), generator=g, device=dev) * s
    RE = torch.randn((I, E), generator=g, device=dev) * s
    CE = torch.randn((C, E), generator=g, device=dev) * s
    _, cats = random_masks(torch, I, C, dev, g)
    eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=dev)
    eng.set_dish_categories(cats)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    items = torch.randint(0, I, (U,), generator=g, device=dev, dtype=torch.int32)
    exclude = None
    if a.excl:
        rng = np.random.default_rng(a.seed)
        ids = np.sort(rng.integers(0, I, (U, a.excl)), axis=1).astype(np.int32)      # ascending per query; repeats count once
        off = np.arange(U + 1, dtype=np.int64) * a.excl
        exclude = (torch.from_numpy(off).to(dev), torch.from_numpy(ids.reshape(-1)).to(dev))

    # the CSR is built once outside the timed region: the call itself (launches) is what is timed
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    ranks = torch.empty(U, dtype=torch.int32, device=dev)
    scores = torch.empty(U, dtype=torch.float32, device=dev)
    off_p = exclude[0].data_ptr() if exclude else None
    ids_p = exclude[1].data_ptr() if exclude else None

    def rank_call():
        rc = _native.lib().m2d_catalogue_rank(eng._h, users.data_ptr(), items.data_ptr(), U, off_p, ids_p, ranks.data_ptr(),
                                              scores.data_ptr(), _stream_ptr())
        _native.raise_for(rc, eng._h)

    out_s = torch.empty((U, 10), dtype=torch.float32, device=dev)
    out_i = torch.empty((U, 10), dtype=torch.int32, device=dev)

    def topk_call():
        eng.topk_users_into(users, 10, out_s, out_i)

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

    t_topk = timed(topk_call)
    t_rank = timed(rank_call)
    lib = os.path.join(ROOT, "foodrec_amd", "libm2d.so")
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    print(json.dumps({"users": U, "dishes": I, "embed": E, "excl_per_query": a.excl, "rank_ms": round(t_rank, 4),
                      "topk10_ms": round(t_topk, 4), "ratio": round(t_rank / t_topk, 3),
                      "rank_tiles_scanned": eng.get_option("rank_tiles_scanned"), "rank_resolved": eng.get_option("rank_resolved"),
                      "git_head": head or None, "libm2d_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest()}))


if __name__ == "__main__":
    main()
