"""Inputs, the numpy restatement and the wrong-kernel stand-ins of the household-retrieval tests (tests/test_group_cases_cpu.py,
tests/test_gpu_groups.py; build-defined, no reference counterpart).

A group's word for a dish is defined on the words m2d_score_slate writes for its members (include/m2d.h): `group_words` restates it on
a float32 matrix of member words -- float32 arithmetic, member order, key-half comparison (deep_cases.keys' high word) with the first
occurrence winning -- and `group_words_loop` is the same rule as a plain Python loop over single words.  Lists are
deep_cases.key_lists over the restated words.  Nothing here imports the engine.  Recipes are computed once and shared (lru_cache);
callers do not write into them."""
import functools
import struct
import types

import numpy as np

import deep_cases as dc
import seen_dish_cases as sd

LEAST, MEAN, MOST = 0, 1, 2                  # include/m2d.h: M2D_GROUP_LEAST / _MEAN / _MOST
MODES = {"least": LEAST, "mean": MEAN, "most": MOST}
MAX_MEMBERS = 64                             # include/m2d.h: M2D_GROUP_MAX_MEMBERS
GR_COLS = 4                                  # m2d_groups.hip: constexpr int GR_COLS = 4 (columns a thread of m2d_group_reduce owns)
STANDINS = ("div_M", "forget_last", "filler", "next_group", "last_tie", "float_least", "float_row0", "excl_row")

MEMBER_COUNTS = (1, 2, 3, 8, 64)
SLATE_SIZES = (1, 3, 4, 5, 63, 64, 65, 129, 1300)             # the vector and tail paths (nD % 4), the slate kernel's TN switch at 64
LIST_SIZES = (255, 256, 257, 1300, 16385)
LIST_KS = (1, 10, 64, 65, 1024)


def rank_half(w):
    """tkm_key's high word of score words (uint32): a smaller value ranks better, NaN is all ones, -0 and +0 are equal"""
    return (dc.keys(np.asarray(w, np.uint32), 0) >> np.uint64(32)).astype(np.uint32)


def counts(members):
    """cnt[g]: the leading entries >= 0 of every row"""
    m = np.asarray(members, np.int64)
    return np.where((m < 0).any(1), (m < 0).argmax(1), m.shape[1])


def group_words(S, members, mode, user_base=0, standin=None):
    """uint32 [nG, nD]: the group words of `members` int [nG, M] (-1 padding) over the float32 matrix S [U, nD] of member words,
    row u the words of user user_base + u.  `standin`: one of STANDINS[:7] -- what a subtly wrong reduce kernel would return."""
    assert standin in (None,) + STANDINS[:7]
    S = np.ascontiguousarray(S, np.float32)
    m = np.asarray(members, np.int64)
    nG, M = m.shape
    cnt = counts(m)
    out = np.zeros((nG, S.shape[1]), np.uint32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for g in range(nG):
            ids = [int(x) for x in m[g, :cnt[g]]]
            if standin == "forget_last" and len(ids) > 1:
                ids = ids[:-1]
            if standin == "filler":                              # every slot is read; a filler slot holds the group's first member
                ids = ids + [ids[0]] * (M - len(ids))
            if standin == "next_group" and cnt[g] == M and g + 1 < nG:
                ids = ids + [int(m[g + 1, 0])]                   # the scratch row behind the group's last is the next group's first
            rows = S[np.asarray(ids) - user_base]
            if mode == MEAN:
                acc = rows[0].copy()
                for j in range(1, len(ids)):
                    acc = (acc + rows[j]).astype(np.float32)
                div = M if standin == "div_M" else len(ids)
                out[g] = dc.words((acc / np.float32(div)).astype(np.float32) if div > 1 else acc)
                continue
            if standin == "float_least" and mode == LEAST:       # a float minimum from +inf: NaN never wins
                acc = np.full(S.shape[1], np.inf, np.float32)
                for j in range(len(ids)):
                    acc = np.where(rows[j] < acc, rows[j], acc)
                out[g] = dc.words(acc)
                continue
            if standin == "float_row0":                          # floats compared from row 0 on: a NaN neither wins nor yields
                acc = rows[0].copy()
                for j in range(1, len(ids)):
                    acc = np.where(rows[j] < acc if mode == LEAST else rows[j] > acc, rows[j], acc)
                out[g] = dc.words(acc)
                continue
            w = dc.words(rows)
            best, rank = w[0].copy(), rank_half(w[0])
            for j in range(1, len(ids)):
                r = rank_half(w[j])
                take = (r > rank) if mode == LEAST else (r < rank)
                if standin == "last_tie":
                    take |= r == rank
                best, rank = np.where(take, w[j], best), np.where(take, r, rank)
            out[g] = best
    return out


def _rank_one(word):
    f = struct.unpack("<f", struct.pack("<I", word))[0]
    if f != f:
        return 0xFFFFFFFF
    b = 0 if f == 0 else word
    return b if b & 0x80000000 else (~(b | 0x80000000)) & 0xFFFFFFFF


def group_words_loop(member_words, mode):
    """One group, one dish, as include/m2d.h words it: `member_words` the members' uint32 words in member order -> the group's word.
    A plain Python loop: float32 scalars for the sum and the one division, integer comparisons for the order."""
    ws = [int(w) for w in member_words]
    if mode == MEAN:
        if len(ws) == 1:
            return ws[0]
        f = [np.uint32(w).view(np.float32) for w in ws]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = f[0]
            for x in f[1:]:
                acc = np.float32(acc + x)
            return int(np.float32(acc / np.float32(len(ws))).view(np.uint32))
    best = ws[0]
    for w in ws[1:]:
        if (mode == LEAST and _rank_one(w) > _rank_one(best)) or (mode == MOST and _rank_one(w) < _rank_one(best)):
            best = w
    return best


def same_words(got, want, mode):
    """Word equality; under MEAN a NaN is compared as a NaN (its payload is the adder's own: numpy's and the device's may differ)"""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    if mode != MEAN:
        return np.array_equal(got, want)
    gn, wn = np.isnan(got.view(np.float32)), np.isnan(want.view(np.float32))
    return np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn])


# ---- members ---------------------------------------------------------------------------------------------------------------------------
def member_matrix(U, nG, M, seed=0, user_base=0):
    """int32 [nG, M]: group g has 1 + (g mod M) members drawn from [0, U) -- every count from 1 to M, so fillers everywhere --, -1
    behind them; every fifth group of two or more repeats its first member as its second"""
    rng = np.random.default_rng(900 + 31 * M + nG + seed)
    m = np.full((nG, M), -1, np.int32)
    for g in range(nG):
        c = 1 + g % M
        m[g, :c] = rng.integers(0, U, c)
        if c >= 2 and g % 5 == 3:
            m[g, 1] = m[g, 0]
    return m + np.where(m >= 0, user_base, 0).astype(np.int32)


def words_groups(M):
    """groups of a reduction-word call at M members: past one count cycle, and a partial last block at deep_chunk_pairs = 2 048"""
    return M + 6 if M > 8 else 2 * M + 5


@functools.lru_cache(maxsize=None)
def words_recipe(tables, E):
    """tables of the reduction-word cases, I = 1 300: exact (float32 = float64, many equal words and zeros) or normal; an all-zero
    user (every word +0: equal words in every group that holds it) and the empty-mask dishes of deep_cases.nan_dishes (NaN columns)"""
    r = dc.exact_recipe(E, 1300) if tables == "exact" else dc.normal_recipe(E, head=False)
    out = types.SimpleNamespace(E=E, I=r.I, U=r.U, coef=r.coef, RE=r.RE, CE=r.CE, cats=r.cats)
    out.PM = r.PM.copy()
    out.PM[1] = 0.0
    out.PM.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_matrix(tables, E):
    """float32 [U, I]: the recipe's score matrix restated on the host -- what the CPU file evaluates conditions and stand-ins on (the
    GPU file takes the engine's own m2d_score_slate words instead)"""
    r = words_recipe(tables, E)
    S = sd.score_matrix(r.PM, r.RE, r.CE, r.cats, r.coef, np.float32)
    S.setflags(write=False)
    return S


def slate_of(I, nD):
    """an ascending slate of nD of I dishes that holds dish 5 (an empty mask: a NaN column) where nD allows"""
    if nD == I:
        return np.arange(I, dtype=np.int32)
    rng = np.random.default_rng(70 + nD)
    s = set(rng.choice(I, nD, replace=False).tolist())
    if nD >= 3 and 5 not in s:
        s.remove(next(iter(s)))
        s.add(5)
    return np.asarray(sorted(s), np.int32)


# ---- zeros of both signs, infinities -------------------------------------------------------------------------------------------------
SIGN_USERS = {"neg": 0, "pos": 1, "zero": 2, "huge": 3, "plain": 4}


@functools.lru_cache(maxsize=None)
def sign_recipe():
    """Finite tables on which the slate kernels' chain from +0 ends in zeros of BOTH signs and in infinities.  Dishes 0 .. 3 hold
    +1e-30 everywhere (and so does Category_Embedding): against user `neg` (-1e-30 everywhere) every product is a negative number below
    the smallest subnormal and rounds to -0, and -0 + -0 stays -0; against user `pos` every product rounds to +0; user `zero` is
    all zeros (+0).  Dishes 4 and 5 hold -64 / +64 in turn, dishes 6 and 7 +64: user `huge` (3e38 everywhere) overflows on them -- to -inf on
    4 and 5, +inf on 6 and 7: the sign of the first product that overflows, because a fused multiply-add adds the EXACT product
    (-inf + 2.4e39 is -inf, never NaN; a NaN in one member alone comes from an overflowing DISH VECTOR instead: nan_recipe).  r.S: the expected words,
    the float32 fma chain in increasing k over oracle.dish_vectors restated in float64 (exact products, one rounding a step)."""
    from oracle import m2d_oracle as oracle
    E, I = 64, 8
    r = types.SimpleNamespace(E=E, I=I, U=5, coef=0.5)
    r.PM = np.zeros((5, 5, E), np.float32)
    r.PM[0], r.PM[1], r.PM[3], r.PM[4] = -1e-30, 1e-30, 3e38, 0.25
    r.RE = np.full((I, E), 1e-30, np.float32)
    r.RE[4:] = 64.0
    r.RE[4:6, ::2] = -64.0                                   # dishes 4, 5: the first low-level product is negative
    r.CE = np.full((4, E), 1e-30, np.float32)
    r.cats = np.ones((I, 4), np.float32)
    r.cats[1], r.cats[5] = (1, 0, 0, 0), (1, 0, 1, 0)
    with np.errstate(all="ignore"):
        Dt = oracle.dish_vectors(r.RE, r.CE, r.cats, r.coef, np.float32).astype(np.float64)
        P = r.PM.reshape(5, -1).astype(np.float64)
        acc = np.zeros((5, I), np.float32)
        for k in range(P.shape[1]):
            acc = (acc.astype(np.float64) + P[:, k:k + 1] * Dt[None, :, k]).astype(np.float32)
    r.S = acc
    for a in (r.PM, r.RE, r.CE, r.cats, r.S):
        a.setflags(write=False)
    return r


def sign_members():
    """groups over sign_recipe's users: -0 against +0 in both member orders (and against the all-zero user), the overflowing user
    with and without finite company, a group of five"""
    u = SIGN_USERS
    rows = [[u["neg"], u["pos"]], [u["pos"], u["neg"]], [u["neg"], u["zero"], u["pos"]], [u["zero"], u["neg"]], [u["huge"], u["plain"]],
            [u["plain"], u["huge"], u["neg"]], [u["neg"]], [u["pos"], u["plain"], u["neg"], u["huge"], u["zero"]]]
    m = np.full((len(rows), 5), -1, np.int32)
    for g, row in enumerate(rows):
        m[g, :len(row)] = row
    return m


NAN_USERS = {"zero": 0, "plain": 1, "neg": 2, "opp": 3, "plain2": 4}
NAN_MULTI = (0, 1, 2, 3, 6, 7)               # nan_recipe's dishes with two or more categories; 4 and 5 have one


@functools.lru_cache(maxsize=None)
def nan_recipe():
    """Finite tables that the calls accept and on which ONE member's word is a NaN while the others' are not.  The refusal of
    non-finite values looks at the tables; the dish vectors are derived: Category_Embedding holds 3e38 in its first two columns, so
    the category sum of a dish with two or more categories overflows and the dish vector holds +inf there.  Against such a dish
    user `zero` (all zeros) scores fma(0, inf, .) = NaN, user `opp` (+0.25 and -0.25 in those two columns) +inf - inf = NaN, users
    `plain` / `plain2` (+0.25 in both) +inf, user `neg` (-0.25) -inf; against the single-category dishes 4 and 5 every word is finite.
    r.S: the float32 fma chain in increasing k, restated as in sign_recipe (NaN payloads are numpy's)."""
    from oracle import m2d_oracle as oracle
    rng = np.random.default_rng(123)
    E, I = 64, 8
    r = types.SimpleNamespace(E=E, I=I, U=5, coef=0.5)
    f = lambda shape: (rng.integers(-16, 17, shape) / 16.0).astype(np.float32)      # noqa: E731
    r.PM, r.RE, r.CE = f((5, 5, E)), f((I, E)), f((4, E))
    r.CE[:, :2] = 3e38
    r.PM[0] = 0.0
    r.PM[1, 0, :2] = r.PM[4, 0, :2] = 0.25
    r.PM[2, 0, :2] = -0.25
    r.PM[3, 0, :2] = (0.25, -0.25)
    r.cats = np.zeros((I, 4), np.float32)
    for d, pat in enumerate(((1, 1, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1), (1, 0, 0, 0), (0, 0, 1, 0), (1, 1, 1, 0), (0, 0, 1, 1))):
        r.cats[d] = pat
    with np.errstate(all="ignore"):
        Dt = oracle.dish_vectors(r.RE, r.CE, r.cats, r.coef, np.float32).astype(np.float64)
        P = r.PM.reshape(5, -1).astype(np.float64)
        acc = np.zeros((5, I), np.float32)
        for k in range(P.shape[1]):
            acc = (acc.astype(np.float64) + P[:, k:k + 1] * Dt[None, :, k]).astype(np.float32)
    r.S = acc
    for a in (r.PM, r.RE, r.CE, r.cats, r.S):
        a.setflags(write=False)
    return r


def nan_members():
    """groups over nan_recipe's users: a NaN member behind and in front of a +inf one, between -inf and +inf, two NaN members alone,
    the infinities without a NaN, a group of one, all five"""
    u = NAN_USERS
    rows = [[u["plain"], u["zero"]], [u["zero"], u["plain"]], [u["neg"], u["opp"], u["plain"]], [u["zero"], u["opp"]], [u["neg"], u["plain"]],
            [u["plain"]], [u["opp"], u["neg"], u["zero"], u["plain"], u["plain2"]], [u["plain2"], u["plain"], u["opp"]]]
    m = np.full((len(rows), 5), -1, np.int32)
    for g, row in enumerate(rows):
        m[g, :len(row)] = row
    return m


# ---- lists ---------------------------------------------------------------------------------------------------------------------------
def list_members(U, nG=12, M=4, seed=0, user_base=0):
    return member_matrix(U, nG, M, seed=seed + 1, user_base=user_base)


def list_ks(I):
    return sorted({min(k, I) for k in LIST_KS})


def group_lists(S, members, mode, k, lists=None, user_base=0, standin=None, block=None):
    """(score words, ids) of m2d_topk_groups restated: deep_cases.key_lists over the restated group words.  standin "excl_row": group
    g0 + g of a block of `block` groups leaves out lists[g] -- row g of the block -- instead of lists[g0 + g]."""
    w = group_words(S, members, mode, user_base, None if standin == "excl_row" else standin)
    if lists is not None and standin == "excl_row":
        lists = [lists[g % block] for g in range(len(lists))]
    return dc.key_lists(w.view(np.float32), k, lists)


@functools.lru_cache(maxsize=None)
def normal_words(E=64):
    """float32 restatement of the normal list recipe's score matrix (what the CPU conditions are evaluated on)"""
    r = dc.normal_recipe(E, head=False)
    S = sd.score_matrix(r.PM, r.RE, r.CE, r.cats, r.coef, np.float32)
    S.setflags(write=False)
    return r, S


def exclusion_lists(I, nG, best, W=dc.RANGE_W):
    """per-group segments of 0 / 1 / 65 / 300 ids, cycling; a segment starts with the group's two best dishes where the size allows and
    the larger ones hold ids on both sides of every range edge (a multiple of W)"""
    rng = np.random.default_rng(77 + I + nG)
    edge = sorted({d for e in range(W, I, W) for d in (e - 2, e + 1) if d < I})
    out = []
    for g in range(nG):
        size = (0, 1, 65, 300)[g % 4]
        own = [int(best[g][0])] if size == 1 else [int(best[g][0]), int(best[g][1])] + edge if size >= 65 else []
        own = list(dict.fromkeys(own))[:size]
        rest = rng.choice(np.setdiff1d(np.arange(I), own), size - len(own), replace=False).tolist()
        out.append(sorted(own + rest))
    return out
