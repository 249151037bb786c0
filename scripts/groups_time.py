"""Time household retrieval: topk_groups against the torch composition a caller would write without it.

Bench-style tables (N(0, 1/E), uniformly random non-empty masks).  One process, HIP events, warm-up first, the median of the
repeats and their range; the calls of a comparison alternate.  Prints one JSON line per measurement.
    catalogue  topk_groups(mode) for --groups x --members over --dishes at every --embeds and --ks, against `composition`:
               score_slate over dish ranges into a [Gb M, W] block, torch.amin / torch.mean over the member axis, torch.topk, a merge
               with the list so far -- chunked to the call's own scratch budget (2^22 pairs) and to 2^24; the better one counts.
               The call is timed at its default budget and at "deep_chunk_pairs" = 2^24, so each budget has its own pair
    slate      the slate form (among = --slate dishes) against the same composition over one range
    trace      a few topk_groups calls and nothing else worth a trace: run it under `rocprofv3 --kernel-trace --stats` and read
               m2d_group_reduce's share of the call's kernels and its bytes per second (cnt W 4 bytes read, W 4 written per group)

    python scripts/groups_time.py --parts catalogue --groups 8192 65536 --members 2 4 --embeds 64
    python scripts/groups_time.py --parts slate
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["catalogue", "slate"])
    ap.add_argument("--groups", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--members", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--dishes", type=int, default=100000)
    ap.add_argument("--slate", type=int, default=1024)
    ap.add_argument("--embeds", type=int, nargs="+", default=[64, 200])
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--modes", nargs="+", default=["least"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import numpy as np
    import torch

    import foodrec_amd
    from benchlib.common import random_masks

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
        return {name: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)) for name, v in ts.items()}

    def engine(E):
        g = torch.Generator(device=dev)
        g.manual_seed(a.seed)
        s = 1.0 / (E ** 0.5)
        PM = torch.randn((U, C + 1, E), generator=g, device=dev) * s
        RE = torch.randn((I, E), generator=g, device=dev) * s
        CE = torch.randn((C, E), generator=g, device=dev) * s
        _, cats = random_masks(torch, I, C, dev, g)
        eng = foodrec_amd.ScoringEngine(PM, RE, CE, coef=0.99, device=dev)
        eng.set_dish_categories(cats)
        return eng, g

    def composition(eng, members, mode, k, pairs, slate=None):
        """what a caller writes without the call: score_slate per block of whole groups and dish range, a torch reduction over the
        member axis, torch.topk, a merge with the list so far"""
        nG, M = members.shape
        total = I if slate is None else slate.numel()
        W = min(total, 65536)
        Gb = max(1, pairs // (M * W))
        out_s, out_i = [], []
        for g0 in range(0, nG, Gb):
            blk = members[g0:g0 + Gb]
            n = blk.shape[0]
            best_s = best_i = None
            for d0 in range(0, total, W):
                Wc = min(W, total - d0)
                ids = torch.arange(d0, d0 + Wc, dtype=torch.int32, device=dev) if slate is None else slate[d0:d0 + Wc]
                S = eng.score_slate(blk.reshape(-1), ids).view(n, M, Wc)
                G = S.amin(1) if mode == "least" else S.amax(1) if mode == "most" else S.mean(1)
                s, c = torch.topk(G, min(k, Wc), dim=1)
                i = ids[c]
                if best_s is not None:
                    s, c = torch.topk(torch.cat((best_s, s), 1), k, dim=1)
                    i = torch.cat((best_i, i), 1).gather(1, c)
                best_s, best_i = s, i
            out_s.append(best_s)
            out_i.append(best_i)
        return torch.cat(out_s), torch.cat(out_i)

    def compare(eng, part, members, mode, k, E, slate=None):
        # each budget is timed with the option set OUTSIDE the events: the call against the composition of the same budget, alternating
        t = timed({"topk_groups": lambda: eng.topk_groups(members, k, mode, None, slate),
                   "composition_p22": lambda: composition(eng, members, mode, k, 1 << 22, slate)})
        eng.set_option("deep_chunk_pairs", 1 << 24)
        t.update(timed({"topk_groups_p24": lambda: eng.topk_groups(members, k, mode, None, slate),
                        "composition_p24": lambda: composition(eng, members, mode, k, 1 << 24, slate)}))
        eng.set_option("deep_chunk_pairs", 1 << 22)
        eng.check()
        best = min(("composition_p22", "composition_p24"), key=lambda n: t[n][0])
        spread = t[best][2] - t[best][1]
        res = {"part": part, "groups": members.shape[0], "members": members.shape[1], "dishes": I if slate is None else slate.numel(),
               "embed": E, "k": k, "mode": mode, "repeats": a.repeats, "better_composition": best,
               "call_over_composition": round(t["topk_groups"][0] / t[best][0], 3),
               "call_over_composition_at_p22": round(t["topk_groups"][0] / t["composition_p22"][0], 3),
               "call_over_composition_at_p24": round(t["topk_groups_p24"][0] / t["composition_p24"][0], 3)}
        res["verdict"] = "faster" if t[best][0] - t["topk_groups"][0] > spread else (
            "SLOWER" if t["topk_groups"][0] - t[best][0] > spread else "within the composition's spread")
        for name, v in t.items():
            res[name + "_ms"], res[name + "_range_ms"] = v[0], v[1:]
        print(json.dumps(res), flush=True)

    for E in a.embeds:
        eng, g = engine(E)
        for nG in a.groups:
            for M in a.members:
                members = torch.randint(0, U, (nG, M), generator=g, device=dev, dtype=torch.int32)
                for mode in a.modes:
                    if "catalogue" in a.parts:
                        for k in a.ks:
                            compare(eng, "catalogue", members, mode, k, E)
                    if "slate" in a.parts:
                        slate = torch.sort(torch.randperm(I, generator=g, device=dev)[:a.slate]).values.to(torch.int32)
                        compare(eng, "slate", members, mode, a.ks[0], E, slate)
                    if "trace" in a.parts:
                        for _ in range(3):
                            eng.topk_groups(members, a.ks[0], mode)
                        torch.cuda.synchronize()
                        eng.check()
                        W = min(I, 65536)
                        print(json.dumps({"part": "trace", "groups": nG, "members": M, "embed": E, "k": a.ks[0], "mode": mode, "calls": 3,
                                          "reduce_bytes_per_call": nG * (M + 1) * I * 4, "ranges": (I + W - 1) // W,
                                          "blocks": (nG + max(1, (1 << 22) // (M * W)) - 1) // max(1, (1 << 22) // (M * W))}), flush=True)
        eng.close()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
