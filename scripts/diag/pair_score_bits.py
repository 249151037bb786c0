"""Float32 bit patterns of the pair-score kernels on seeded inputs, to compare two builds of m2d_score.hip word for word: every lane
width (E / 4 <= 8, 16, 32, 64, partial and full), throughput and latency form, both mask feeds, the load options, the bf16 mirror, the
ingredient table, the derived U_high table, the C != 4 throughput form and the generic kernel; the kernel name of every case as well.
    python scripts/diag/pair_score_bits.py OUT.npz           run the cases on this build, store them
    python scripts/diag/pair_score_bits.py A.npz B.npz       compare two stored runs"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import numpy as np

if len(sys.argv) == 3:
    a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
    assert sorted(a.files) == sorted(b.files), "the two runs hold different cases"
    cases = [k for k in a.files if k != "kernels"]
    words = sum(a[k].size for k in cases)
    diff = sum(int((a[k] != b[k]).sum()) for k in cases)
    names = int((a["kernels"] != b["kernels"]).sum())
    for k in cases:
        if not np.array_equal(a[k], b[k]):
            print("differs:", k, int((a[k] != b[k]).sum()), "of", a[k].size)
    print("%d cases, %d pairs, %d differing words, %d differing kernel names" % (len(cases), words, diff, names))
    sys.exit(1 if diff or names else 0)

import torch
from foodrec_amd import ScoringEngine
from helpers import random_case

U, I = 700, 300
DEFAULTS = {"prefetch": 2, "nt_loads": 1, "skip_masked": 1, "pm_bf16": 0, "user_high_table": 0}
out, kernels = {}, []


def run(tag, C, E, B, opts=(), ingredients=False):
    PM, RE, CE, users, items, cats = random_case(U, I, C, E, B, seed=10 * E + C)
    rng = np.random.default_rng(E + C)
    eng = ScoringEngine(PM, RE, CE)
    eng.set_dish_categories(rng.integers(0, 2, (I, C)).astype(np.float32))
    if ingredients:
        off = np.zeros(I + 1, np.int32)
        off[1:] = np.cumsum(rng.integers(1, 7, I))
        eng.set_ingredients((rng.standard_normal((300, E)) / np.sqrt(E)).astype(np.float32), off, rng.integers(0, 300, off[-1]).astype(np.int32))
    for name, value in {**DEFAULTS, **dict(opts)}.items():
        eng.set_option(name, value)
    u, d, m = (torch.as_tensor(x, device="cuda") for x in (users, items, cats))
    for feed in ("pair", "dish"):
        if ingredients:
            s = eng.score_pairs_ingredients(u, d, m if feed == "pair" else None)
        else:
            s = eng.score_pairs(u, d, m) if feed == "pair" else eng.score_pairs_bydish(u, d)
        eng.check()
        key = "%s_C%d_E%d_B%d_%s" % (tag, C, E, B, feed)
        out[key] = s.cpu().numpy().view(np.uint32)
        kernels.append(key + "=" + eng.last_kernel())


FORMS = [("default", ()), ("pf1", (("prefetch", 1), ("nt_loads", 0))), ("pf4", (("prefetch", 4), ("nt_loads", 0))),
         ("noskip", (("skip_masked", 0),)), ("bf16", (("pm_bf16", 1),))]
for E in (24, 32, 48, 64, 100, 128, 200, 256):
    for B in (20011, 301):
        for tag, opts in FORMS:
            run(tag, 4, E, B, opts)
        run("ing", 4, E, B, ingredients=True)
for E in (64, 200):
    run("uh", 4, E, (1 << 18) + 77, (("user_high_table", 1),))
for C, E in ((3, 64), (6, 36), (8, 16), (2, 128), (7, 200)):
    for B in (20011, 300):
        for nt in (0, 1):
            run("nt%d" % nt, C, E, B, (("nt_loads", nt),))
for C, E in ((4, 6), (9, 64)):
    for B in (20011, 300):
        run("generic", C, E, B)
np.savez_compressed(sys.argv[1], kernels=np.array(sorted(kernels)), **out)
print("%d cases, %d pairs; kernels: %s" % (len(out), sum(v.size for v in out.values()), sorted({k.split("=")[1] for k in kernels})))
