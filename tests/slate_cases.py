"""Inputs, references, bounds and stand-ins of the slate-scoring tests (tests/test_slate_cases_cpu.py, tests/test_gpu_slate.py):
m2d_score_slate / m2d_topk_slate, the [users x slate] score matrix and the k best dishes of a slate per user.

Everything here is the oracle's, in float64: the tables of a recipe, the scores of every (user, slate dish), the rounding bound of an
f32 fused-multiply-add chain over the factored operands, the ranking order, and the comparisons the GPU file applies.  Nothing here
imports the engine.  Recipes and references are computed once and shared (lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

import seen_dish_cases as sd
from derived_table_cases import WIDTHS
from topk_mlp_cases import order

# the kernel's tile constants, restated
BM = 128            # m2d_slate.hip: constexpr int SL_BM = 128 (users of a block's tile)
BN = 128            # m2d_slate.hip: BN = 64 * TN, TN = 2 (dishes of a block's tile) ...
BN_SMALL = 64       # ... and TN = 1 for slates of up to 64 dishes (launch_scores: TN = nD <= 64 ? 1 : 2)
KC = 32             # m2d_slate.hip: constexpr int SL_KC = 32 (floats of K per LDS stage; Dt_s rows are K rounded up to it)

COEF = 0.5          # lists: at 0.99 almost no user is sharp (topk_mlp_cases.COEF)
MIN_SHARP = 0.7
U_ROUND = 2.0 ** -24
NU_EDGES = (1, 31, 32, 33, BM - 1, BM, BM + 1, 2 * BM + 5)
ND_EDGES = (1, 31, 32, 33, BN_SMALL - 1, BN_SMALL, BN_SMALL + 1, BN - 1, BN, BN + 1, 2 * BN + 3)


def bits(x):
    """float32 words with -0 folded onto +0: a chain that starts at +0 never ends in -0 where the exact sum is 0"""
    return (np.asarray(x, np.float32) + np.float32(0)).view(np.int32)


# ---- exact tables ----------------------------------------------------------------------------------------------------------------
EXACT_SLATE = 300


@functools.lru_cache(maxsize=None)
def exact_recipe(E):
    """seen_dish_cases.launch_recipe(E) -- exact tables, U = 32, I = 600, four empty-mask dishes -- with a slate of 300 ascending ids
    that holds the four, and the users in a shuffled order with repeats."""
    r = sd.launch_recipe(E)
    rng = np.random.default_rng(500 + E)
    rest = np.setdiff1d(np.arange(r.I), sd.LAUNCH_EMPTY)
    slate = np.sort(np.concatenate([np.asarray(sd.LAUNCH_EMPTY), rng.choice(rest, EXACT_SLATE - 4, replace=False)])).astype(np.int32)
    users = np.concatenate([rng.permutation(r.U), rng.integers(0, r.U, 8)]).astype(np.int32)
    x = types.SimpleNamespace(E=E, U=r.U, I=r.I, coef=r.coef, PM=r.PM, RE=r.RE, CE=r.CE, cats=r.cats, S=r.S, slate=slate, users=users)
    x.ref = r.S[users][:, slate]                              # float64; every value a float32
    x.ref.setflags(write=False)
    return x


def exact_lists(ref, slate, k, higher_id=False, positions=False):
    """(scores [n, k], ids [n, k]) of the oracle ranking over the slate.  Stand-ins: `higher_id` resolves equal scores to the higher
    id; `positions` ranks columns 0 .. nD - 1 instead of the slate's ids (and lists those)."""
    ids = np.arange(len(slate)) if positions else np.asarray(slate, np.int64)
    ss, ii = [], []
    for row in ref:
        nan = np.isnan(row)
        o = np.lexsort((-ids if higher_id else ids, -np.where(nan, -np.inf, row), nan))[:k]
        ss.append(row[o])
        ii.append(ids[o])
    return np.asarray(ss), np.asarray(ii)


# ---- normal tables: float64 reference and the rounding bound -----------------------------------------------------------------------
def gamma(n):
    return n * U_ROUND / (1.0 - n * U_ROUND)


def reference_and_bound(PM, RE, CE, cats, coef, users, slate):
    """(ref64 [nU, nD], bound [nU, nD]) for float masks cats [I, C] (any non-negative weights).

    ref64 = <flatten(PM[u]), Dt[d]> in float64 (oracle.dish_vectors; a and 1 - a the float32 words the graph holds).
    bound = gamma_n T(u, d), n = K + C + 4, the standard bound of an f32 fma chain of K terms over operands that carry C + 3 roundings
    of their own (the sum over c of m_c CE_c: C, the division by n_d, the products with a / b and with m_c / n_d):
      T = (|a| / n_d) sum_e |U_high,e| sum_c |m_c CE_c,e| + (|b| / n_d) sum_c sum_e |m_c U_low,c,e RE_d,e|.
    Derived, not measured.  A dish with n_d = 0 is NaN in both."""
    from oracle import m2d_oracle as oracle
    C, E = CE.shape
    a, b = (np.float64(x) for x in oracle.blend_coefficients(coef))
    users, slate = np.asarray(users, np.int64), np.asarray(slate, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        Dt = oracle.dish_vectors(RE, CE, cats, coef, np.float64)[slate]
        P = np.asarray(PM, np.float64)[users]                                 # [nU, C + 1, E]
        ref = P.reshape(len(users), -1) @ Dt.T
        m = np.asarray(cats, np.float64)[slate]                               # [nD, C]
        nd = m.sum(1)
        hi = np.abs(P[:, 0]) @ (np.abs(m) @ np.abs(np.asarray(CE, np.float64))).T          # [nU, nD]
        r = np.abs(np.asarray(RE, np.float64)[slate])                         # [nD, E]
        lo = np.einsum("uce,dc,de->ud", np.abs(P[:, 1:]), np.abs(m), r)
        T = (abs(a) * hi + abs(b) * lo) / nd
    K = (C + 1) * E
    return ref, gamma(K + C + 4) * T


def assert_within(got, ref, bound, what=""):
    """NaN where the reference is NaN, |got - ref| <= bound elsewhere; returns the largest err / bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ (%d vs %d)" % (what, np.isnan(got).sum(), nan.sum())
    err = np.abs(got - ref)[~nan]
    lim = bound[~nan]
    bad = err > lim
    assert not bad.any(), "%s: %d of %d outside the bound, worst err %.3e at bound %.3e" % (
        what, int(bad.sum()), bad.size, err[bad].max(), lim[bad][err[bad].argmax()])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(lim > 0, err / lim, 0.0))) if err.size else 0.0


@functools.lru_cache(maxsize=None)
def normal_recipe(E, C=4, U=48, I=300, nD=150, weighted=False, seed=0):
    """Normal tables (N(0, 1 / E)), 0/1 masks with a category set -- or weights from {0, 0.5, 1, 2} -- three dishes with an empty mask
    inside the slate, users shuffled with repeats.  The reference depends on the blend: reference_and_bound(r..., coef)."""
    rng = np.random.default_rng(11000 + 131 * E + 7 * C + seed)
    r = types.SimpleNamespace(E=E, C=C, U=U, I=I)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, U, I, E, C)
    if weighted:
        r.cats = rng.choice(np.array([0, 0.5, 1, 2], np.float32), (I, C))
        r.cats[r.cats.sum(1) == 0, 0] = 2.0
    else:
        r.cats = sd.masks(rng, I, C)
    r.slate = np.sort(rng.choice(I, nD, replace=False)).astype(np.int32)
    r.cats[r.slate[[0, nD // 2, nD - 1]]] = 0.0
    r.users = np.concatenate([rng.permutation(U), rng.integers(0, U, 5)]).astype(np.int32)
    for a in (r.PM, r.RE, r.CE, r.cats, r.slate, r.users):
        a.setflags(write=False)
    return r


# ---- lists on normal tables ------------------------------------------------------------------------------------------------------------
LIST_U, LIST_I = 256, 2000
LIST_SLATES = ((33, 16), (97, 10), (300, 10))              # (slate size, k) up to E = 128
LIST_K_WIDE = 5                                             # E >= 256: k = 16 / 10 / 10 leaves 0.53 / 0.68 / 0.72 of the users sharp, k = 5
                                                            # 0.88 - 0.91 (E = 200 keeps its k: 0.73 / 0.78 / 0.79)
LIST_WIDTHS = (4, 32, 64, 128, 200, 256)
GENERIC_SHAPES = ((3, 8), (6, 20), (4, 6), (4, 260))        # (C, E) the MFMA kernel does not take


def list_k(E, k):
    return min(k, LIST_K_WIDE) if E >= 256 else k


@functools.lru_cache(maxsize=None)
def list_recipe(E, nD, k, C=4, U=LIST_U, I=LIST_I):
    """Normal tables at blend 0.5, every user asked once, a slate of nD ascending ids: ref64, the bound, and the sharp users."""
    rng = np.random.default_rng(21000 + 131 * E + nD + 7 * C)
    r = types.SimpleNamespace(E=E, C=C, U=U, I=I, k=k, coef=COEF)
    r.PM, r.RE, r.CE = sd.normal_tables(rng, U, I, E, C)
    r.cats = sd.masks(rng, I, C)
    r.slate = np.sort(rng.choice(I, nD, replace=False)).astype(np.int32)
    r.users = np.arange(U, dtype=np.int32)
    r.ref, r.bound = reference_and_bound(r.PM, r.RE, r.CE, r.cats, COEF, r.users, r.slate)
    r.sharp = sharp_users(r.ref, r.bound, r.slate, k)
    for a in (r.PM, r.RE, r.CE, r.cats, r.slate, r.users, r.ref, r.bound, r.sharp):
        a.setflags(write=False)
    return r


def _sorted(ref, bound, slate):
    ids = np.asarray(slate, np.int64)
    o = np.stack([order(row, ids) for row in ref])
    return np.take_along_axis(ref, o, 1), np.take_along_axis(bound, o, 1), ids[o]


def sharp_users(ref, bound, slate, k):
    """every neighbouring gap among the first k + 1 reference scores exceeds twice the larger of the two dishes' bounds: no
    arithmetic inside the bound can swap two of them, or the k-th with the first one left out"""
    s, b, _ = _sorted(ref, bound, slate)
    s, b = s[:, :k + 1], b[:, :k + 1]
    with np.errstate(invalid="ignore"):
        return np.all(s[:, :-1] - s[:, 1:] > 2 * np.maximum(b[:, :-1], b[:, 1:]), axis=1)


def compare_lists(got_s, got_i, ref, bound, slate, k, what=""):
    """topk_mlp_cases.compare_lists' conditions with the derived bound: per user, B = the largest bound over the slate's dishes,
      (a) position by position |got_score[j] - ref_sorted_score[j]| <= B, NaN where the reference is NaN;
      (b) every listed id is a slate dish, none twice, and its reference score is at least the reference's k-th score - 2 B;
      (c) the listed scores do not increase, equal scores come in ascending id, NaN entries last in ascending id;
    and for sharp users the ids are the reference's.  Returns the sharp mask."""
    got_s, got_i = np.asarray(got_s, np.float64), np.asarray(got_i, np.int64)
    n = ref.shape[0]
    assert got_s.shape == (n, k) and got_i.shape == (n, k), (what, got_s.shape, got_i.shape)
    rs, _, ri = _sorted(ref, bound, slate)
    sharp = sharp_users(ref, bound, slate, k)
    col = {int(d): c for c, d in enumerate(np.asarray(slate))}
    for j in range(n):
        tag = "%s user row %d" % (what, j)
        B = np.nanmax(bound[j])
        want, g = rs[j, :k], got_s[j]
        assert np.array_equal(np.isnan(g), np.isnan(want)), "%s: NaN positions %s vs %s" % (tag, np.isnan(g), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(g[ok] - want[ok]) <= B), "%s: scores %s vs %s (bound %.3e)" % (tag, g, want, B)
        assert all(int(d) in col for d in got_i[j]), "%s: id outside the slate: %s" % (tag, got_i[j])
        assert len(set(got_i[j].tolist())) == k, "%s: an id is listed twice: %s" % (tag, got_i[j])
        mine = np.array([ref[j][col[int(d)]] for d in got_i[j]])
        kth = want[k - 1]
        if not np.isnan(kth):
            assert not np.isnan(mine).any() and np.all(mine >= kth - 2 * B), "%s: listed %s, k-th %r" % (tag, mine, kth)
        for a in range(k - 1):
            sa, sb, ia, ib = g[a], g[a + 1], got_i[j, a], got_i[j, a + 1]
            if np.isnan(sa):
                assert np.isnan(sb) and ia < ib, "%s: NaN entries not last in ascending id at %d" % (tag, a)
            elif not np.isnan(sb):
                assert sa > sb or (sa == sb and ia < ib), "%s: order broken at %d: (%r, %d) (%r, %d)" % (tag, a, sa, ia, sb, ib)
        if sharp[j]:
            assert np.array_equal(got_i[j], ri[j, :k]), "%s: sharp user, ids %s vs %s" % (tag, got_i[j], ri[j, :k])
    return sharp


# ---- stand-ins: what a subtly wrong kernel would return ----------------------------------------------------------------------------------
def standin_no_last_chunk(PM, RE, CE, cats, coef, users, slate):
    """(a) the contraction without its last K chunk of KC floats (the whole K where it is shorter: the chunk is the only one)"""
    from oracle import m2d_oracle as oracle
    K = PM.shape[1] * PM.shape[2]
    last = (K - 1) // KC * KC
    with np.errstate(invalid="ignore", divide="ignore"):
        Dt = oracle.dish_vectors(RE, CE, cats, coef, np.float64)[np.asarray(slate, np.int64)]
        P = np.asarray(PM, np.float64)[np.asarray(users, np.int64)].reshape(len(users), -1)
        return P[:, :last] @ Dt[:, :last].T


def standin_re_stride(PM, RE, CE, cats, coef, users, slate):
    """(b) the slate's rows read at Recipe_Embedding's stride E instead of the slate table's own: row j of Dt_s then holds floats
    [j E, j E + K) of the table laid out with rows of Kp floats"""
    from oracle import m2d_oracle as oracle
    E = RE.shape[1]
    K = PM.shape[1] * E
    Kp = -(-K // KC) * KC
    with np.errstate(invalid="ignore", divide="ignore"):
        Dt = oracle.dish_vectors(RE, CE, cats, coef, np.float64)[np.asarray(slate, np.int64)]
        flat = np.zeros((len(slate) + 1 + K // Kp, Kp))
        flat[:len(slate), :K] = Dt
        flat = flat.reshape(-1)
        wrong = np.stack([flat[j * E:j * E + K] for j in range(len(slate))])
        return np.asarray(PM, np.float64)[np.asarray(users, np.int64)].reshape(len(users), -1) @ wrong.T


def changed_share(a, b):
    """share of the elements that differ (NaN equal to NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    return float((~((a == b) | (np.isnan(a) & np.isnan(b)))).mean())
