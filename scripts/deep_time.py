"""Time the deep retrieval lists (DESIGN.md sections 4.11, 8.8): m2d_select_deep alone, the whole catalogue call, the two-stage head form.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks).  One process, HIP events, warm-up first, the median of the
repeats and their range; the calls of a comparison alternate.  Prints one JSON line per measurement.
    select     m2d_select_deep over a resident [R, W] block of the engine's own scores (m2d_select_probe) at k = 64 / 256 / 1024,
               against torch.topk(block, k, sorted=True) on the same tensor and, at k = 64, m2d_topk_mlp_select; "clear": the medians
               differ by more than the reference's own range
    equal      the same block filled with one value at k = 1024, beside the normal-table time
    catalogue  topk_users_deep for --users x --dishes at every --embeds and k = 64 / 1024; the selection's share: the selection
               launches of a call timed alone over the same block shapes, over the call's time
    head       topk_users_mlp_deep(candidates = 64 / 256 / 1024) against topk_users_mlp(candidates = 64), --head-users users

    python scripts/deep_time.py --parts select equal
    python scripts/deep_time.py --parts catalogue --embeds 64 128 200
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["select", "equal", "catalogue", "head"])
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--head-users", type=int, default=8192)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--embeds", type=int, nargs="+", default=[64, 128, 200])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr

    dev = torch.device("cuda", 0)
    U, I, C = a.users, a.dishes, 4

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
        return {name: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)) for name, v in ts.items()}

    def emit(res, t):
        for name, v in t.items():
            res[name + "_ms"], res[name + "_range_ms"] = v[0], v[1:]
        print(json.dumps(res), flush=True)

    def engine(E, head=False):
        g = torch.Generator(device=dev)
        g.manual_seed(a.seed)
        s = 1.0 / (E ** 0.5)
        PM = torch.randn((U, C + 1, E), generator=g, device=dev) * s
        RE = torch.randn((I, E), generator=g, device=dev) * s
        CE = torch.randn((C, E), generator=g, device=dev) * s
        _, cats = random_masks(torch, I, C, dev, g)
        eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=dev)
        eng.set_dish_categories(cats)
        if head:
            rng, K = np.random.default_rng(a.seed), (C + 1) * E
            w = lambda *shape: (rng.standard_normal(shape) * 4.0 / np.sqrt(shape[0])).astype(np.float32)      # noqa: E731
            eng.set_mlp_head(w(K, 256), w(256) / 40, w(256, 64), w(64) / 40, w(64), 0.25)
        return eng, torch.randperm(U, generator=g, device=dev).to(torch.int32)

    def probe(eng, block, k, form, out):
        rc = _native.lib().m2d_select_probe(eng._h, block.data_ptr(), block.shape[0], block.shape[1], k, form, out[0].data_ptr(),
                                            out[1].data_ptr(), _stream_ptr())
        _native.raise_for(rc, eng._h)

    def outs(rows, k):
        return torch.empty((rows, k), dtype=torch.float32, device=dev), torch.empty((rows, k), dtype=torch.int32, device=dev)

    if "select" in a.parts or "equal" in a.parts:
        eng, users = engine(64)
        for R, W in ((64, min(65536, I)), (41, I)):
            block = eng.score_slate(users[:R], torch.arange(W, dtype=torch.int32, device=dev))
            if "select" in a.parts:
                for k in (64, 256, 1024):
                    o = outs(R, k)
                    fns = {"deep": lambda: probe(eng, block, k, 0, o), "torch_topk": lambda: torch.topk(block, k, dim=1, sorted=True)}
                    if k == 64:
                        fns["old_select"] = lambda: probe(eng, block, k, 1, o)
                    t = timed(fns)
                    res = {"part": "select", "rows": R, "W": W, "k": k, "repeats": a.repeats}
                    for ref in [n for n in fns if n != "deep"]:
                        spread = t[ref][2] - t[ref][1]
                        res["deep_over_" + ref] = round(t["deep"][0] / t[ref][0], 3)
                        res["verdict_vs_" + ref] = "faster" if t[ref][0] - t["deep"][0] > spread else (
                            "SLOWER" if t["deep"][0] - t[ref][0] > spread else "within the reference's spread")
                    emit(res, t)
            if "equal" in a.parts:
                o = outs(R, 1024)
                flat = torch.full_like(block, 0.25)
                emit({"part": "equal", "rows": R, "W": W, "k": 1024, "repeats": a.repeats},
                     timed({"equal_rows": lambda: probe(eng, flat, 1024, 0, o), "normal_rows": lambda: probe(eng, block, 1024, 0, o)}))
        eng.close()
        del eng
        torch.cuda.empty_cache()

    if "catalogue" in a.parts:
        for E in a.embeds:
            eng, users = engine(E)
            W = min(I, 1 << 22, 65536)
            R = max(1, (1 << 22) // W)
            blocks = (U + R - 1) // R
            for k in (64, 1024):
                t = timed({"topk_users_deep": lambda: eng.topk_users_deep(users, k)})
                eng.check()
                sel = 0.0                                    # the call's selection launches, timed alone on blocks of the same shapes
                for d0 in range(0, I, W):
                    Wc = min(W, I - d0)
                    block = eng.score_slate(users[:R], torch.arange(d0, d0 + Wc, dtype=torch.int32, device=dev))
                    o = outs(R, k)
                    sel += timed({"s": lambda: probe(eng, block, k, 0, o)})["s"][0]
                res = {"part": "catalogue", "users": U, "dishes": I, "embed": E, "k": k, "repeats": a.repeats, "kernel": eng.last_kernel(),
                       "selection_ms": round(sel * blocks, 2)}
                res["selection_share"] = round(sel * blocks / t["topk_users_deep"][0], 3)
                res["tflops_of_the_call"] = round(2.0 * (C + 1) * E * U * I / (t["topk_users_deep"][0] * 1e-3) / 1e12, 1)
                emit(res, t)
            eng.close()
            del eng
            torch.cuda.empty_cache()

    if "head" in a.parts:
        eng, users = engine(64, head=True)
        users = users[:a.head_users]
        fns = {"topk_users_mlp_c64": lambda: eng.topk_users_mlp(users, 10, 64)}
        for K1 in (64, 256, 1024):
            fns["deep_c%d" % K1] = (lambda K1: lambda: eng.topk_users_mlp_deep(users, 10, None, K1))(K1)
        t = timed(fns)
        eng.check()
        emit({"part": "head", "users": a.head_users, "dishes": I, "embed": 64, "k": 10, "repeats": a.repeats}, t)
        eng.close()


if __name__ == "__main__":
    main()
