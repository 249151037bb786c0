"""Recipes, the numpy restatement and the stand-ins of the profile tests (tests/test_profile_cases_cpu.py,
tests/test_gpu_profiles.py): m2d_compose_profiles and the calls served from its rows.

A profile q = (u_q, y_q) has the memory block, in this order of operations,

    ysum = sum_l y_l                      label order, weights != 0 only
    g_k  = fma(y_l, GM[l][k], g_k)        label order, weights != 0 only, from 0
    M_k  = base_k + alpha * (g_k / ysum)  one rounded product, one rounded sum
    base = PM[u_q - user_base] for u_q >= 0, zeros for a guest (-1)

`restate` states it in float64 (the reference of every comparison) or float32 (what the kernel computes, up to the fma: numpy has
none, the float32 restatement rounds the float64 value of y * r + g, which is the fma's value except under double rounding).
Nothing here imports the engine.  Cases are computed once and shared (lru_cache); callers do not write into them."""
import functools
import types

import numpy as np

MAXM = 4            # m2d_profiles.hip: constexpr int MAXM = 4 (mask words of 64 labels: L <= 256, a plain loop beyond)
KEEP = 5            # m2d_profiles.hip: constexpr int KEEP = 5 (columns a lane keeps in registers: 320 columns, more are computed twice)
U2 = 2.0 ** -24     # unit roundoff of float32

STANDINS = ("count_divisor", "ignore_weights", "alpha_on_base", "drop_labels_64", "labels_of_request_0", "fused")


def _case(**kw):
    r = types.SimpleNamespace(**kw)
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def restate(PM, GM, labels, users, alpha, dtype=np.float64, user_base=0, standin=None):
    """rows [n, (C+1) E] in `dtype`.  users: None (all guests) or ids, -1 = a guest.  `standin`: what a subtly wrong kernel would
    return --
      "count_divisor"        the sum is divided by the number of non-zero labels, not by their weight sum;
      "ignore_weights"       every non-zero weight counts as 1;
      "alpha_on_base"        alpha multiplies the base as well: alpha * (base + g / ysum);
      "drop_labels_64"       labels from 64 on are never read (one mask word);
      "labels_of_request_0"  every request is composed from request 0's labels;
      "fused"                product and sum in one rounding: fma(alpha, g / ysum, base)."""
    assert standin is None or standin in STANDINS
    t = np.dtype(dtype).type
    n, L = labels.shape
    W = GM.shape[1] * GM.shape[2]
    G = GM.reshape(L, W)
    P = PM.reshape(PM.shape[0], W)
    out = np.zeros((n, W), dtype)
    a = t(alpha)
    for q in range(n):
        y = labels[0 if standin == "labels_of_request_0" else q]
        nz = np.flatnonzero(y != 0)
        if standin == "drop_labels_64":
            nz = nz[nz < 64]
        w = np.ones(len(nz), dtype) if standin == "ignore_weights" else y[nz].astype(dtype)
        ysum, g = t(0), np.zeros(W, dtype)
        for wl, l in zip(w, nz):
            ysum = t(ysum + wl)
            g = (np.float64(wl) * G[l].astype(np.float64) + g.astype(np.float64)).astype(dtype)       # the fma
        if standin == "count_divisor":
            ysum = t(len(nz))
        u = -1 if users is None else int(users[q])
        base = np.zeros(W, dtype) if u == -1 else P[u - user_base].astype(dtype)
        with np.errstate(all="ignore"):
            mean = (g / ysum).astype(dtype)
            if standin == "alpha_on_base":
                out[q] = (a * (base + mean).astype(dtype)).astype(dtype)
            elif standin == "fused":
                out[q] = (np.float64(a) * mean.astype(np.float64) + base.astype(np.float64)).astype(dtype)
            else:
                out[q] = (base + (a * mean).astype(dtype)).astype(dtype)
    return out


def bound(PM, GM, labels, users, alpha, user_base=0):
    """(2 m + 4) 2^-24 (|base_k| + |alpha| sum_l |y_l GM[l][k]| / ysum), m the request's number of non-zero labels: the gamma-bound of
    the op sequence -- m fma's and m - 1 adds of ysum, a division, a product, a sum, and the float64 reference's own error far below
    one of those units.  float64 [n, (C+1) E]."""
    n, L = labels.shape
    W = GM.shape[1] * GM.shape[2]
    G = np.abs(GM.reshape(L, W).astype(np.float64))
    P = np.abs(PM.reshape(PM.shape[0], W).astype(np.float64))
    out = np.zeros((n, W))
    for q in range(n):
        y = labels[q].astype(np.float64)
        m = int((y != 0).sum())
        u = -1 if users is None else int(users[q])
        base = 0.0 if u == -1 else P[u - user_base]
        out[q] = (2 * m + 4) * U2 * (base + abs(float(alpha)) * (np.abs(y) @ G) / y.sum())
    return out


def bound_conditions(labels, alpha):
    """what the bound assumes: weights >= 0 with a positive sum in every request (no cancellation in ysum), finite alpha"""
    return bool((labels >= 0).all() and (labels.sum(1) > 0).all() and np.isfinite(alpha))


# ---- recipes ------------------------------------------------------------------------------------------------------------------------
# weight patterns whose sum is a power of two (division by ysum is then exact), weights in {1/2, 1, 2}
PATTERNS = ((1.0,), (2.0,), (0.5,), (0.5, 0.5), (1.0, 1.0), (2.0, 2.0), (1.0, 0.5, 0.5), (2.0, 1.0, 1.0), (2.0, 1.0, 0.5, 0.5),
            (2.0, 2.0, 2.0, 2.0), (0.5, 0.5, 0.5, 0.5, 1.0, 1.0), (2.0, 2.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5))
EXACT_ALPHAS = (0.0, 0.25, 1.0)
N_KNOWN = 9         # rows of Personal_Memory in every recipe

#              L    E   C  n (None: 32 CUs + 3)  users     user_base
EXACT_SHAPES = ((1, 4, 4, 1, "null", 0),
                (63, 6, 4, 4, "mixed", 0),
                (64, 60, 3, 5, "mixed", 0),
                (65, 64, 4, 5, "mixed", 7000),
                (95, 68, 4, 4, "known", 0),
                (256, 200, 4, 5, "mixed", 0),
                (257, 256, 4, 4, "mixed", 7000),
                (257, 6, 3, 5, "null", 0),
                (64, 70, 4, 4, "mixed", 0),          # scalar path, 350 columns: past the KEEP x 64 a lane keeps
                (95, 256, 5, 4, "mixed", 0),         # float4 path, 384 columns: the same
                (95, 64, 4, None, "mixed", 0))
NORMAL_SHAPES = ((95, 64, 4, 5, "mixed", 0),
                 (257, 200, 4, 4, "mixed", 7000),
                 (65, 6, 3, 5, "null", 0),
                 (130, 68, 4, 5, "known", 0))
NORMAL_ALPHA = 0.01


def second_trip_requests(num_cu):
    """one wave per request, m2d_blocks_for(h, n, 4): at most 8 blocks of 4 waves per CU -- three requests more take a second trip"""
    return 32 * num_cu + 3


def _users(rng, n, mode, user_base):
    if mode == "null":
        return None
    u = rng.integers(user_base, user_base + N_KNOWN, n).astype(np.int32)
    if mode == "mixed":
        u[1::2] = -1
        if n == 1:
            u[0] = -1
    return u


def _positions(rng, q, L, m):
    """m distinct labels of request q; request 0 takes the last label and, past one mask word, label 64"""
    pos = rng.choice(L, size=m, replace=False)
    if q == 0:
        forced = [L - 1] + ([64] if L > 64 and m > 1 and L - 1 != 64 else [])
        rest = [p for p in pos if p not in forced]
        pos = np.asarray((forced + rest)[:m])
    return np.sort(pos)


@functools.lru_cache(maxsize=None)
def exact_case(L, E, C, n, mode, user_base, which=0):
    """dyadic tables (sixteenths and thirty-seconds), weights in {0, 1/2, 1, 2} with a power-of-two sum, dyadic alpha: every
    operation is exact in float32, so float32 == float64 and the kernel has one right answer per word"""
    rng = np.random.default_rng([L, E, C, n, user_base, which])
    W = (C + 1) * E
    PM = (rng.integers(-32, 33, (N_KNOWN, C + 1, E)) / 32.0).astype(np.float32)
    GM = (rng.integers(-16, 17, (L, C + 1, E)) / 16.0).astype(np.float32)
    labels = np.zeros((n, L), np.float32)
    fits = [p for p in PATTERNS if len(p) <= L]
    for q in range(n):
        p = fits[(q + which) % len(fits)]
        labels[q, _positions(rng, q, L, len(p))] = rng.permutation(p)
    users = _users(rng, n, mode, user_base)
    alpha = EXACT_ALPHAS[(which + L + E) % len(EXACT_ALPHAS)]
    return _case(PM=PM, GM=GM, labels=labels, users=users, alpha=alpha, user_base=user_base, L=L, E=E, C=C, n=n, W=W)


@functools.lru_cache(maxsize=None)
def normal_case(L, E, C, n, mode, user_base, alpha=NORMAL_ALPHA):
    """normal tables, non-negative weights (zeros, and uniform in (0, 2]), distinct per request; request 0 holds a label past every
    mask-word edge the shape has"""
    rng = np.random.default_rng([L, E, C, n, user_base, 77])
    PM = rng.standard_normal((N_KNOWN, C + 1, E)).astype(np.float32)
    GM = rng.standard_normal((L, C + 1, E)).astype(np.float32)
    labels = np.zeros((n, L), np.float32)
    for q in range(n):
        m = int(min(L, 2 + (3 * q) % 7))
        labels[q, _positions(rng, q, L, m)] = (2.0 - rng.uniform(0.0, 1.9, m)).astype(np.float32)
    users = _users(rng, n, mode, user_base)
    if users is not None and mode == "known":
        users = ((np.arange(n) * 2) % N_KNOWN + user_base).astype(np.int32)      # distinct: the Write_Memory witness adds once per user
    return _case(PM=PM, GM=GM, labels=labels, users=users, alpha=alpha, user_base=user_base, L=L, E=E, C=C, n=n, W=(C + 1) * E)


def aimed_at(standin):
    """the normal cases a stand-in has to be caught by (bound test), or for "fused" the witness cases (bit test)"""
    if standin == "drop_labels_64":
        return [s for s in NORMAL_SHAPES if s[0] > 64]
    if standin == "alpha_on_base":
        return [s for s in NORMAL_SHAPES if s[4] != "null"]
    if standin == "fused":
        return [s for s in NORMAL_SHAPES if s[4] == "known"]
    return list(NORMAL_SHAPES)


# ---- served calls: a catalogue with 0/1 masks and recipes -------------------------------------------------------------------------------
CATALOGUES = (255, 256, 257, 16385)
SERVED_E, SERVED_L, SERVED_N, SERVED_R = 64, 95, 5, 40
SERVED_KS = (1, 10, 16, 64)
EXCL_LENS = (0, 1, 65, 0, 1)
COEF = 0.99


@functools.lru_cache(maxsize=None)
def served_case(I):
    """normal tables of E = 64, C = 4; every dish in one to three categories; recipes of one to six of 40 ingredients; five profiles
    (guests and known users mixed), their markets and their exclusion lists of 0, 1 and 65 dishes"""
    rng = np.random.default_rng([I, 5])
    C, E, L, n = 4, SERVED_E, SERVED_L, SERVED_N
    PM = rng.standard_normal((N_KNOWN, C + 1, E)).astype(np.float32)
    RE = rng.standard_normal((I, E)).astype(np.float32)
    CE = rng.standard_normal((C, E)).astype(np.float32)
    GM = rng.standard_normal((L, C + 1, E)).astype(np.float32)
    cats = (rng.random((I, C)) < 0.4).astype(np.float32)
    cats[np.arange(I), rng.integers(0, C, I)] = 1.0
    lens = rng.integers(1, 7, I)
    off = np.zeros(I + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    ids = rng.integers(0, SERVED_R, off[-1]).astype(np.int32)
    labels = np.zeros((n, L), np.float32)
    for q in range(n):
        m = 2 + q
        labels[q, rng.choice(L, m, replace=False)] = (2.0 - rng.uniform(0.0, 1.9, m)).astype(np.float32)
    users = np.asarray([3, -1, 0, -1, 8], np.int32)
    markets = [np.sort(rng.choice(SERVED_R, size=m, replace=False)).astype(np.int32) for m in (40, 25, 12, 30, 0)]
    exclude = [np.sort(rng.choice(I, size=m, replace=False)).astype(np.int32) for m in EXCL_LENS]
    return _case(PM=PM, RE=RE, CE=CE, GM=GM, cats=cats, off=off, ids=ids, labels=labels, users=users, markets=markets, exclude=exclude,
                 alpha=0.5, I=I, C=C, E=E, L=L, n=n, R=SERVED_R)
