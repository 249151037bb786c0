"""Inputs, references and the list comparison of the head-retrieval tests (tests/test_topk_mlp_cpu.py, tests/test_gpu_topk_mlp.py).

Everything here is the oracle's, in float64: the tables of a recipe, the head scores of every (test user, dish) pair, the two
conditions on the inputs ("the head matters", "the list is decidable") and the comparison of a returned list with the reference.
Nothing here imports the engine.  References are computed once per recipe and shared (lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

from helpers import TOL, mlp_head

COEF = 0.5          # at 0.99 the sharp share drops to 0.19 - 0.33 (the head's own tests run at 0.5 for the same reason)
MIN_SHARE = 0.9     # of the users: lists that differ from the base lists; sharp lists

# name -> (U, I, C, E, H1, H2, test users, k, seed).  The table rows ARE the users: U of them, the first `test users` are asked.
RECIPES = {
    "pc": (48, 1000, 4, 64, 256, 64, 37, 10, 14),           # producer / consumer form
    "gather": (48, 333, 4, 32, 256, 64, 48, 16, 2),         # padded gather form: K = 160
    "generic": (48, 333, 4, 8, 32, 16, 48, 64, 3),          # generic kernel
    "e128": (8, 257, 4, 128, 256, 64, 5, 1, 4),
    "pc5000": (24, 5000, 4, 64, 256, 64, 24, 10, 5),        # three dish ranges at chunk 2 048: 2 048, 2 048, 904
    "ties": (48, 2200, 4, 64, 256, 64, 48, 16, 6),          # dish d + 2048 copies dish d, d < 64
    "nan40": (16, 40, 4, 64, 256, 64, 16, 16, 7),           # 30 dishes with an empty mask
    "stage3000": (3000, 1000, 4, 64, 256, 64, 3000, 10, 8), # two-stage, K1 = 64
    "i33": (40, 33, 4, 64, 256, 64, 40, 10, 9),             # two-stage, K1 = I
    "ing": (48, 500, 4, 64, 256, 64, 48, 10, 10),           # ingredient table set
}
# the recipes whose inputs must meet both conditions over the whole catalogue, at the recipe's k -- "generic" at k = 10: with 64 of
# 333 dishes listed, 65 neighbouring gaps all above 2 b are met by 0.44 of the users, whatever the seed (0.96 - 1.00 at k = 10, the
# k the condition was laid down with); its k = 64 lists are still compared user by user, exact ids for those sharp at 64
CONDITIONED = {"pc": 10, "gather": 16, "generic": 10, "e128": 1, "pc5000": 10, "ing": 10, "i33": 10}
TIE_COPIES, TIE_SHIFT = 64, 2048


def bound(x):
    return TOL * np.maximum(1.0, np.abs(x))


@functools.lru_cache(maxsize=None)
def recipe(name):
    """Tables standard normal times 0.5, Bernoulli(0.5) masks with at least one category set, helpers.mlp_head at scale 4."""
    U, I, C, E, H1, H2, nU, k, seed = RECIPES[name]
    rng = np.random.default_rng(1000 + seed)
    r = types.SimpleNamespace(name=name, U=U, I=I, C=C, E=E, H1=H1, H2=H2, k=k, coef=COEF)
    r.PM = (rng.standard_normal((U, C + 1, E)) * 0.5).astype(np.float32)
    r.RE = (rng.standard_normal((I, E)) * 0.5).astype(np.float32)
    r.CE = (rng.standard_normal((C, E)) * 0.5).astype(np.float32)
    r.cats = (rng.random((I, C)) < 0.5).astype(np.float32)
    r.cats[r.cats.sum(1) == 0, 0] = 1
    r.head = mlp_head((C + 1) * E, H1, H2, rng, scale=4.0)
    r.users = np.arange(nU, dtype=np.int32)
    r.ing = r.H = None
    if name == "ties":
        r.RE[TIE_SHIFT:TIE_SHIFT + TIE_COPIES] = r.RE[:TIE_COPIES]
        r.cats[TIE_SHIFT:TIE_SHIFT + TIE_COPIES] = r.cats[:TIE_COPIES]
    if name == "nan40":
        r.cats[rng.permutation(I)[:30]] = 0
    if name == "ing":
        from oracle import m2d_oracle as oracle
        R = 60
        ING = (rng.standard_normal((R, E)) * 0.5).astype(np.float32)
        lens = rng.integers(1, 12, I)
        off = np.zeros(I + 1, np.int32)
        off[1:] = np.cumsum(lens)
        ids = rng.integers(0, R, off[-1]).astype(np.int32)
        r.ing, r.H = (ING, off, ids), oracle.dish_high_vectors(ING, off, ids)
    return r


def head_scores(r, users, items=None, tables=None, head=None):
    """float64 oracle head scores: [len(users), I], or [len(users), n] for items [len(users), n]."""
    from oracle import m2d_oracle as oracle
    PM, RE, CE = tables if tables is not None else (r.PM, r.RE, r.CE)
    head = head if head is not None else r.head
    users = np.asarray(users)
    items = np.broadcast_to(np.arange(r.I), (len(users), r.I)) if items is None else np.asarray(items)
    step = max(1, 65536 // items.shape[1])       # z is [pairs, K] float64: 64 Ki pairs at a time
    out = [oracle.inference_mlp(PM, RE, CE, r.cats, *head, np.repeat(users[j:j + step], items.shape[1]), items[j:j + step].reshape(-1),
                                coef=r.coef, dish_high=r.H).reshape(-1, items.shape[1]) for j in range(0, len(users), step)]
    return np.concatenate(out)


def base_scores(r, users, items=None):
    """float64 scores without the head (the reference score; the ingredient score when the table is set): sum_k z[k], the
    factored form the head's own definition starts from (oracle.inference_mlp)."""
    from oracle import m2d_oracle as oracle
    Dt = oracle.dish_vectors(r.RE, r.CE, r.cats, r.coef, np.float64)
    if r.H is not None:
        Dt[:, :r.E] = np.float64(oracle.blend_coefficients(r.coef)[0]) * r.H
    with np.errstate(invalid="ignore"):
        full = r.PM[np.asarray(users)].reshape(len(users), -1).astype(np.float64) @ Dt.T
    return full if items is None else np.take_along_axis(full, np.asarray(items, dtype=np.int64), axis=1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The recipe's [test users, I] head scores (read-only)."""
    r = recipe(name)
    ref = head_scores(r, r.users)
    ref.setflags(write=False)
    return ref


def order(scores, ids):
    """oracle.topk_catalogue's lexsort rule over one user's candidates: score descending, ties to the lower id, NaN last by id."""
    nan = np.isnan(scores)
    return np.lexsort((ids, -np.where(nan, -np.inf, scores), nan))


def ranked(ref, ids=None):
    """Per user (sorted scores, sorted ids) of ref [n, m]; ids [n, m] or None (the column is the id)."""
    ss, ii = [], []
    for j in range(ref.shape[0]):
        idj = np.arange(ref.shape[1]) if ids is None else np.asarray(ids[j])
        o = order(ref[j], idj)
        ss.append(ref[j][o])
        ii.append(idj[o])
    return np.asarray(ss), np.asarray(ii)


def sharp_users(sorted_scores, k):
    """Every neighbouring pair of the first k + 1 reference scores differs by more than 2 b (fewer where there are no k + 1)."""
    s = sorted_scores[:, :k + 1]
    with np.errstate(invalid="ignore"):
        gap = s[:, :-1] - s[:, 1:]
        return np.all(gap > 2 * np.maximum(bound(s[:, :-1]), bound(s[:, 1:])), axis=1)


def conditions(ref, base, k, ids=None):
    """(share of users whose head top-k id set differs from the base's, share of sharp users)."""
    rs, ri = ranked(ref, ids)
    _, bi = ranked(base, ids)
    differ = np.array([set(a[:k]) != set(b[:k]) for a, b in zip(ri, bi)])
    return float(differ.mean()), float(sharp_users(rs, k).mean())


def assert_conditions(ref, base, k, ids=None, what=""):
    differ, sharp = conditions(ref, base, k, ids)
    assert differ >= MIN_SHARE, "%s: the head changes %.2f of the lists only: inputs refused" % (what, differ)
    assert sharp >= MIN_SHARE, "%s: %.2f of the users are sharp only: inputs refused" % (what, sharp)
    return differ, sharp


def compare_lists(got_s, got_i, ref, k, ids=None, what=""):
    """What a list comparison asserts, for every user (ref [n, m] oracle scores of the m candidates, ids [n, m] or the column):
      (a) position by position |got_score[j] - ref_sorted_score[j]| <= b, NaN where the reference is NaN;
      (b) every listed id is a candidate and its reference score is at least the reference's k-th score - 2 b;
      (c) the listed scores do not increase, equal scores come in ascending id, NaN entries last in ascending id;
    and for sharp users the ids are the reference's.  Returns the sharp mask."""
    got_s, got_i = np.asarray(got_s, dtype=np.float64), np.asarray(got_i, dtype=np.int64)
    n = ref.shape[0]
    assert got_s.shape == (n, k) and got_i.shape == (n, k), (what, got_s.shape, got_i.shape)
    rs, ri = ranked(ref, ids)
    sharp = sharp_users(rs, k)
    for j in range(n):
        tag = "%s user row %d" % (what, j)
        want, g = rs[j, :k], got_s[j]
        # (a)
        assert np.array_equal(np.isnan(g), np.isnan(want)), "%s: NaN positions %s vs %s" % (tag, np.isnan(g), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(g[ok] - want[ok]) <= bound(want[ok])), "%s: scores %s vs %s" % (tag, g, want)
        # (b)
        idj = np.arange(ref.shape[1]) if ids is None else np.asarray(ids[j])
        col = {int(d): c for c, d in enumerate(idj)}
        assert all(int(d) in col for d in got_i[j]), "%s: id outside the candidates: %s" % (tag, got_i[j])
        assert len(set(got_i[j].tolist())) == k, "%s: an id is listed twice: %s" % (tag, got_i[j])
        mine = np.array([ref[j][col[int(d)]] for d in got_i[j]])
        kth = want[k - 1]
        if not np.isnan(kth):
            assert not np.isnan(mine).any() and np.all(mine >= kth - 2 * bound(kth)), "%s: listed %s, k-th %r" % (tag, mine, kth)
        # (c)
        for a in range(k - 1):
            sa, sb, ia, ib = g[a], g[a + 1], got_i[j, a], got_i[j, a + 1]
            if np.isnan(sa):
                assert np.isnan(sb) and ia < ib, "%s: NaN entries not last in ascending id at %d" % (tag, a)
            elif not np.isnan(sb):
                assert sa > sb or (sa == sb and ia < ib), "%s: order broken at %d: (%r, %d) (%r, %d)" % (tag, a, sa, ia, sb, ib)
        if sharp[j]:
            assert np.array_equal(got_i[j], ri[j, :k]), "%s: sharp user, ids %s vs %s" % (tag, got_i[j], ri[j, :k])
    return sharp


def chunk_geometry(nU, I, P, candidates=0):
    """(dish range width, user rows per block, head launches) of a call at "topk_mlp_chunk_pairs" = P (include/m2d.h)."""
    W = candidates if candidates else min(I, P)
    R = min(max(1, P // W), nU)
    blocks = -(-nU // R)
    return W, R, blocks * (1 if candidates else -(-I // W))
