"""Every output word of catalogue_rank and topk_users_excluding on seeded inputs, to compare two builds of the ranking scans
(m2d_catalogue_rank.hip, m2d_catalogue_excl.hip) word for word: ranks, held-out scores, list ids and list score words as integers.
Bench-style N(0, 1/E) tables, random non-empty masks plus a few empty-mask dishes; E = 32, 48, 64, 128, 200 (the three one-lane
widths, a padded row width, the 16-lane forms); 3 001 dishes; 40 and 5 000 queries / users (below and above the n > 64 sort, 512
shares and few); the rank call without and with exclusion lists and without its score output; the excluding call at k = 1, 10, 16
under topk_excl_tier 0 and 2 with lists of 0 and 20 ids, every user's own top 16, and one segment longer than the LDS copy holds;
one shape on a user_base shard.  The diagnostic counters are stored apart ("diag:<counter>:<case>"): the record sort places records with
atomics, so a wave's membership, and with it some tile counts, may differ between two runs of ONE build.
    python scripts/diag/rank_bits.py OUT.npz               run the cases on this build, store them
    python scripts/diag/rank_bits.py A.npz B.npz [A2.npz]  compare two stored runs; with A2, a second run of A's build, only the
                                                           counters that A2 reproduces in every case are compared"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

if len(sys.argv) >= 3:
    a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
    assert sorted(a.files) == sorted(b.files), "the two runs hold different cases"
    cases = [k for k in a.files if not k.startswith("diag:")]
    diags = [k for k in a.files if k.startswith("diag:")]
    diff = 0
    for k in cases:
        d = int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else max(a[k].size, b[k].size)
        if d:
            print("differs:", k, d, "of", a[k].size)
        diff += d
    a2 = np.load(sys.argv[3]) if len(sys.argv) > 3 else a
    bad = 0
    for name in sorted({k.split(":")[1] for k in diags}):   # a counter is compared if the first build reproduces it in every case
        mine = [k for k in diags if k.split(":")[1] == name]
        wobble = sum(int(a[k] != a2[k]) for k in mine)
        moved = sum(int(a[k] != b[k]) for k in mine)
        print("counter %-24s %3d cases, %3d differ between the first build's two runs, %3d between the builds%s"
              % (name, len(mine), wobble, moved, "" if wobble else "  (compared)"))
        bad += 0 if wobble else moved
    print("%d cases, %d words, %d differing words; %d differing values of the counters compared" % (len(cases), sum(a[k].size for k in cases), diff, bad))
    sys.exit(1 if diff or bad else 0)

import torch
from foodrec_amd import ScoringEngine, _native
from foodrec_amd.ops import _stream_ptr

I = 3001
dev = torch.device("cuda", 0)
out = {}


def csr(lists):                                             # ascending id lists -> device (offsets, ids): taken as they are, checked by the kernels
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return torch.from_numpy(off).to(dev), torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(dev)


def run(E, n, user_base=0):
    rng = np.random.default_rng(1000 * E + n)
    s = 1.0 / np.sqrt(E)
    PM = (rng.standard_normal((n, 5, E)) * s).astype(np.float32)
    RE = (rng.standard_normal((I, E)) * s).astype(np.float32)
    CE = (rng.standard_normal((4, E)) * s).astype(np.float32)
    pat = rng.integers(1, 16, I)
    pat[rng.choice(I, 7, replace=False)] = 0                # a few empty-mask dishes (NaN scores, ranked last)
    cats = ((pat[:, None] >> np.arange(4)) & 1).astype(np.float32)
    eng = ScoringEngine(PM, RE, CE, coef=0.99, device=dev, user_base=user_base)
    eng.set_dish_categories(cats)
    users = torch.from_numpy((rng.permutation(n) + user_base).astype(np.int32)).to(dev)
    items = torch.from_numpy(rng.integers(0, I, n).astype(np.int32)).to(dev)
    tag = "E%d_n%d%s" % (E, n, "_base" if user_base else "")

    def keep(key, counters, **arrays):
        eng.check()
        for name, t in arrays.items():
            out["%s_%s_%s" % (tag, key, name)] = t.cpu().numpy().view(np.int32)
        for c in counters:
            out["diag:%s:%s_%s" % (c, tag, key)] = np.array(eng.get_option(c), np.int64)

    random20 = [np.unique(rng.integers(0, I, 20)) for _ in range(n)]
    for key, excl in (("none", None), ("x20", random20)):
        ranks, scores = eng.catalogue_rank(users, items, excl)
        keep("rank_" + key, ("rank_tiles_scanned", "rank_resolved"), ranks=ranks, scores=scores)
    ranks = torch.full((n,), -1, dtype=torch.int32, device=dev)   # the native call without its score output
    _native.raise_for(_native.lib().m2d_catalogue_rank(eng._h, users.data_ptr(), items.data_ptr(), n, None, None, ranks.data_ptr(), None,
                                                       _stream_ptr()), eng._h)
    keep("rank_noscores", ("rank_tiles_scanned", "rank_resolved"), ranks=ranks)

    _, own = eng.topk_users_excluding(users, 16, None)
    own16 = [np.sort(r[r >= 0]) for r in own.cpu().numpy()]
    long1 = list(random20)
    long1[n // 2] = np.unique(rng.integers(0, I, 200))      # one segment past the LDS copy: searched in HBM
    lists = (("x0", csr([np.zeros(0, np.int32)] * n)), ("x20", csr(random20)), ("own16", csr(own16)), ("long", csr(long1)))
    for tier in (0, 2):
        eng.set_option("topk_excl_tier", tier)
        for k in (1, 10, 16):
            for key, excl in lists:
                sc, ids = eng.topk_users_excluding(users, k, excl)
                keep("excl_t%d_k%d_%s" % (tier, k, key), ("topk_excl_short", "topk_excl_tiles_scanned"), scores=sc, ids=ids)


for E in (32, 48, 64, 128, 200):
    for n in (40, 5000):
        run(E, n)
run(64, 5000, user_base=100000)
np.savez_compressed(sys.argv[1], **out)
print("%d arrays, %d words" % (sum(not k.startswith("diag:") for k in out), sum(v.size for k, v in out.items() if not k.startswith("diag:"))))
