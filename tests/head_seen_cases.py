"""Recipes, references and stand-ins of the seen-dish tests under the MLP head (tests/test_head_seen_cases_cpu.py,
tests/test_gpu_head_seen.py).

The exact reference of a list or a rank is the order's key rule applied on the host to a [users, I] matrix of score WORDS (float32 on
the GPU: the engine's own score_pairs_mlp words; float64 oracle scores in the CPU file) over the dishes not excluded.  The stand-ins
are the same functions with one mistake switched on.  Nothing here imports the engine."""
import functools
import types

import numpy as np

import topk_mlp_cases as tc
from helpers import mlp_head

MIN_SHARE = tc.MIN_SHARE

# name -> (U, I, C, E, H1, H2, test users, k, seed): topk_mlp_cases' form; the names it has are its recipes
RECIPES = {
    "w255": (8, 255, 4, 64, 256, 64, 8, 10, 21),            # one 64-thread block, a partial last step
    "w256": (8, 256, 4, 64, 256, 64, 8, 10, 22),            # ... a whole one
    "w257": (8, 257, 4, 64, 256, 64, 8, 10, 23),            # the 256-thread block, a second step of one dish
    "w16385": (3, 16385, 4, 32, 256, 64, 3, 10, 24),        # the 1 024-thread block
    "base600": (64, 600, 4, 64, 256, 64, 64, 10, 25),       # two-stage: stage 1 in the ranking arithmetic
}
LIST_RECIPES = ("pc", "gather", "generic", "ing", "pc5000", "ties", "w255", "w256", "w257", "w16385", "base600")
FAMILIES = {"pc": "m2d_mlp_pc_bf16x3", "gather": "m2d_mlp_mfma_bf16x3", "generic": "m2d_mlp_generic", "ing": "m2d_mlp_pc_bf16x3"}
EDGE_IDS = (0, 63, 64, 65, 255, 256, 257)                   # and I - 1
RANGE_IDS = (2047, 2048, 4095, 4096, 4999)                  # pc5000 at chunk 2 048: ranges of 2 048, 2 048, 904
# the k of the list cases: at 10 MIN_SHARE of every family recipe's users are sharp over the dishes left, from the oracle alone
# (tests/test_head_seen_cases_cpu.py; "gather" at 16, 333 dishes less its three best: 0.875 - 0.90 whatever the seed)
LIST_K = 10


@functools.lru_cache(maxsize=None)
def recipe(name):
    if name in tc.RECIPES:
        return tc.recipe(name)
    U, I, C, E, H1, H2, nU, k, seed = RECIPES[name]
    rng = np.random.default_rng(1000 + seed)
    r = types.SimpleNamespace(name=name, U=U, I=I, C=C, E=E, H1=H1, H2=H2, k=k, coef=tc.COEF)
    r.PM = (rng.standard_normal((U, C + 1, E)) * 0.5).astype(np.float32)
    r.RE = (rng.standard_normal((I, E)) * 0.5).astype(np.float32)
    r.CE = (rng.standard_normal((C, E)) * 0.5).astype(np.float32)
    r.cats = (rng.random((I, C)) < 0.5).astype(np.float32)
    r.cats[r.cats.sum(1) == 0, 0] = 1
    r.head = mlp_head((C + 1) * E, H1, H2, rng, scale=4.0)
    r.users = np.arange(nU, dtype=np.int32)
    r.ing = r.H = None
    return r


@functools.lru_cache(maxsize=None)
def reference(name):
    """[test users, I] float64 oracle head scores (read-only)."""
    r = recipe(name)
    ref = tc.head_scores(r, r.users)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def exclusions(name, extra=20):
    """Per test user: the oracle's three best dishes, the edge ids (EDGE_IDS, I - 1; RANGE_IDS where the catalogue has them) for
    every other user, and `extra` random others; each list in random order with one id repeated.  Read-only tuple of tuples."""
    r, ref = recipe(name), reference(name)
    rng = np.random.default_rng([77, r.I])
    _, ri = tc.ranked(ref)
    out = []
    for j in range(len(r.users)):
        x = list(ri[j, :3]) + list(rng.choice(r.I, min(extra, r.I), replace=False))
        if j % 2 == 0:
            x += [d for d in EDGE_IDS + RANGE_IDS + (r.I - 1,) if d < r.I]
        x = [int(d) for d in x]
        x.append(x[0])
        out.append(tuple(int(d) for d in rng.permutation(x)))
    return tuple(out)


WINDOW_DISHES = (2048, 4096, 0, 64, 1088, 4992)             # pc5000: the first ids of the ranges at chunk 2 048, other multiples of 64


def front_exclusions(words, dishes=WINDOW_DISHES):
    """Per user j: dish d = dishes[j % len] and every dish in front of it in the order of words[j].  The correct list then starts
    behind d; a window that loses the excluded id d lists d first -- whatever d scored."""
    order = filtered_lists(words, None, words.shape[1])[1]
    out = []
    for j in range(words.shape[0]):
        d = dishes[j % len(dishes)]
        out.append(tuple(int(x) for x in order[j][:int(np.flatnonzero(order[j] == d)[0]) + 1]))
    return out


def csr(lists):
    """ascending, distinct per segment: (offsets int64[n + 1], ids int32)"""
    segs = [np.unique(np.asarray(x, dtype=np.int64)) for x in lists]
    off = np.zeros(len(segs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in segs])
    return off, (np.concatenate(segs) if segs else np.zeros(0)).astype(np.int32)


def _order(scores, ids, ties_high=False):
    """the key rule: score descending, -0 / +0 and equal scores to the lower id, NaN after every -inf in id order"""
    nan = np.isnan(scores)
    return np.lexsort((-ids if ties_high else ids, -np.where(nan, -np.inf, scores), nan))


def filtered_lists(words, excl, k, wrong=None, range_w=2048):
    """Rows of the first k (word, id) of the order over the dishes not excluded, NaN / -1 where fewer remain.  `wrong`: a stand-in --
    "ignore" (no exclusions), "mult64" (an excluded id at a multiple of 64 stays), "range_first" (one at the first id of a dish range
    of `range_w` stays), "ties_high" (equal scores to the higher id)."""
    n, I = words.shape
    out_s = np.full((n, k), np.nan, dtype=words.dtype)
    out_i = np.full((n, k), -1, dtype=np.int32)
    for j in range(n):
        x = np.unique(np.asarray(excl[j], dtype=np.int64)) if excl is not None else np.zeros(0, np.int64)
        if wrong == "ignore":
            x = x[:0]
        elif wrong == "mult64":
            x = x[x % 64 != 0]
        elif wrong == "range_first":
            x = x[x % range_w != 0]
        keep = np.ones(I, bool)
        keep[x] = False
        ids = np.flatnonzero(keep)
        o = _order(words[j][ids], ids, wrong == "ties_high")[:k]
        out_s[j, :len(o)] = words[j][ids][o]
        out_i[j, :len(o)] = ids[o]
    return out_s, out_i


def ranks(words, rows, held, excl, wrong=None):
    """For query q = (row rows[q] of `words`, held-out dish held[q], excluded excl[q]): the dishes of the catalogue, not excluded and
    not the held-out one, that precede it.  `wrong`: "count_held" (the held-out dish counts itself when its key ties: it is compared
    with <=), "count_excluded" (excluded dishes count), "ties_high"."""
    out = np.zeros(len(rows), np.int64)
    I = words.shape[1]
    ids = np.arange(I)
    for q, (j, p) in enumerate(zip(rows, held)):
        s = words[j]
        sp = s[p]
        nan, pn = np.isnan(s), np.isnan(sp)
        with np.errstate(invalid="ignore"):
            tie = (nan & pn) | (s == sp)
            before = (~nan & pn) | (s > sp) | (tie & ((ids > p) if wrong == "ties_high" else (ids < p)))
        if wrong == "count_held":
            before[p] = True
        else:
            before[p] = False
        if excl is not None and wrong != "count_excluded":
            x = np.asarray(excl[q], dtype=np.int64)
            before[x[x != p]] = False
        out[q] = before.sum()
    return out


def two_stage(cand, head_words, k, wrong=None):
    """Stage 2 on the host: cand [n, K1] ids with -1 in empty slots, head_words [n, K1] the words of those pairs (an empty slot's is
    the pair on dish 0's).  `wrong` = "keep_minus1": an empty slot keeps its score and is listed as id -1."""
    n, K1 = cand.shape
    out_s = np.full((n, k), np.nan, dtype=head_words.dtype)
    out_i = np.full((n, k), -1, dtype=np.int32)
    for j in range(n):
        ok = np.flatnonzero(cand[j] >= 0) if wrong != "keep_minus1" else np.arange(K1)
        o = ok[_order(head_words[j][ok], cand[j][ok].astype(np.int64))][:k]
        out_s[j, :len(o)] = head_words[j][o]
        out_i[j, :len(o)] = cand[j][o]
    return out_s, out_i


def held_out(ref_row, excl_row, rng, n_random=3):
    """Held-out dishes of one user: the remaining order's first (rank 0) and last dish, an excluded dish (its own id in X: ignored),
    and a few behind at least one excluded dish."""
    I = len(ref_row)
    keep = np.ones(I, bool)
    keep[np.asarray(excl_row, dtype=np.int64)] = False
    ids = np.flatnonzero(keep)
    o = ids[_order(ref_row[ids], ids)]
    return [int(o[0]), int(o[-1]), int(excl_row[0])] + [int(d) for d in rng.choice(o[len(o) // 2:], n_random, replace=False)]


def share_excluded_in_topk(ref, excl, k):
    _, ri = tc.ranked(ref)
    return float(np.mean([bool(set(ri[j, :k].tolist()) & set(excl[j])) for j in range(ref.shape[0])]))


def share_excluded_precedes(ref, rows, held, excl):
    """queries where an excluded dish (other than the held-out one) precedes the held-out dish"""
    plain = ranks(ref, rows, held, None)
    return float(np.mean(plain > ranks(ref, rows, held, excl)))


def rank_brackets(ref, rows, held, excl):
    """[lo, hi] per query from oracle scores: #{ref > s_p + 2 b} and #{ref >= s_p - 2 b} over the remaining dishes other than p;
    a NaN held-out score: every non-NaN remaining dish, plus (hi) every NaN one."""
    lo, hi = [], []
    for q, (j, p) in enumerate(zip(rows, held)):
        keep = np.ones(ref.shape[1], bool)
        keep[np.asarray(excl[q], dtype=np.int64)] = False
        keep[p] = False
        s, sp = ref[j][keep], ref[j][p]
        if np.isnan(sp):
            lo.append(int((~np.isnan(s)).sum()))
            hi.append(len(s))
        else:
            b = 2 * tc.bound(sp)
            with np.errstate(invalid="ignore"):
                lo.append(int((s > sp + b).sum()))
                hi.append(int((s >= sp - b).sum()))
    return np.asarray(lo), np.asarray(hi)
