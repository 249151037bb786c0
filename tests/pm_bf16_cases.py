"""Inputs and CPU-side arithmetic of the "pm_bf16" tests (tests/test_gpu_pm_bf16.py, tests/test_pm_bf16_cpu.py).

The option serves pair scores from a bf16 mirror of Personal_Memory.  Its contract is exact: the mirror is the round-to-nearest-even
image of the table, and a score is what the f32 kernels return on an engine built from the rounded table, bit for bit.  What is
needed on the CPU side is therefore the rounding itself (`round_bf16`, checked against torch's conversion in the CPU file), tables on
which rounding SHOWS (`scaled_case`), and the condition that it does (`visible_share`).
"""
import functools

import numpy as np

from helpers import TOL, random_case

# The share of the non-NaN pairs whose float64 score on the unrounded table lies more than two assert_scores_close bounds away from
# the one on the rounded table.  A condition on the INPUTS of a comparison: a kernel that read the f32 table fails the oracle check
# on the rounded table at those pairs.
VISIBLE = 0.85

E_GRID = [4, 12, 36, 64, 128, 200, 256]
COEFS = [0.99, 0.5, 1.25]
U, I, C = 257, 300, 4
B_GRID = [1, 63, 64, 65, 8192, 8193]


def bf16_bits(x):
    """float32 -> the uint16 bf16 pattern, round to nearest, ties to even, in the integer form: add 0x7fff and the lowest kept bit,
    shift.  Subnormals are rounded, -0 and +-inf kept, finite values past the bf16 range become +-inf; NaN -> 0x7fc0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7fffffff) > 0x7f800000, np.uint16(0x7fc0), r)


def from_bits(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x):
    """x rounded to bf16 and widened again: the float32 table the mirror stands for."""
    return from_bits(bf16_bits(x)).reshape(np.shape(x))


def f32_from_u32(*patterns):
    return np.array(patterns, dtype=np.uint32).view(np.float32)


# value -> what it must round to (both as float32).  NaN is compared by isnan.
PLANTED = np.concatenate([
    np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, 3.4e38, -3.4e38], dtype=np.float32),
    np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], dtype=np.float32),          # ties: -> 1.0 (even), -> 1.015625 (even)
    f32_from_u32(0x7f7f7fff, 0xff7f7fff),                                    # the largest magnitudes that still round to the bf16 maximum
    f32_from_u32(0x7f7f8000),                                                # the tie above it: to even, which is inf
    np.array([np.nan], dtype=np.float32)])
# (1e-40 is the subnormal 0x000116c2: it rounds to the bf16 subnormal 0x0001, not to 0)
PLANTED_ROUNDED = f32_from_u32(0x00000000, 0x80000000, 0x00010000, 0x80010000, 0x7f800000, 0xff800000, 0x7f800000, 0xff800000,
                               0x3f800000, 0x3f820000, 0x7f7f0000, 0xff7f0000, 0x7f800000, 0x7fc00000)


def plant(PM, seed=0):
    """PLANTED scattered over a copy of PM: the first and the last element, and random places."""
    out = PM.copy()
    flat = out.reshape(-1)
    rng = np.random.default_rng(seed)
    pos = rng.choice(flat.size - 2, len(PLANTED) - 2, replace=False) + 1
    flat[0], flat[-1] = PLANTED[6], PLANTED[9]
    flat[pos] = np.delete(PLANTED, [6, 9])
    return out


def scaled_case(Ux, Ix, Cx, E, B, seed, zero_rows=True):
    """helpers.random_case with every table multiplied by sqrt(E) (entries of order 1) and Personal_Memory by a further 8: a score is
    then of order 8 sqrt(E) and bf16's 2^-9 relative rounding of its user rows moves it by a few hundred assert_scores_close bounds."""
    PM, RE, CE, users, items, cats = random_case(Ux, Ix, Cx, E, B, seed, zero_rows=zero_rows)
    s = np.float32(np.sqrt(E))
    return (PM * (8 * s)).astype(np.float32), (RE * s).astype(np.float32), (CE * s).astype(np.float32), users, items, cats


def dish_masks(Ix, Cx, seed):
    """Masks by dish: random 0/1 patterns, a few of them empty (NaN scores) and a few weighted."""
    rng = np.random.default_rng(seed)
    m = ((rng.integers(0, 2 ** Cx, Ix)[:, None] >> np.arange(Cx)[None, :]) & 1).astype(np.float32)
    m[::7] *= rng.uniform(0.5, 2.0, (len(m[::7]), Cx)).astype(np.float32)
    return m


@functools.lru_cache(maxsize=None)
def grid_case(E, coef):
    """One (E, coef) recipe of the score grid: tables, 8193 pairs with per-pair masks, masks by dish, and the float64 references on
    the rounded and on the unrounded table for both mask feeds.  Every B of the grid is a prefix of these pairs."""
    import types
    from oracle import m2d_oracle as oracle
    PM, RE, CE, users, items, cats = scaled_case(U, I, C, E, max(B_GRID), 100 + E)
    by_dish = dish_masks(I, C, 200 + E)
    PMr = round_bf16(PM)
    refs = {}
    for feed, m in (("pair", cats), ("dish", by_dish[items])):
        refs[feed] = (oracle.inference_f64(PMr, RE, CE, users, items, m, coef), oracle.inference_f64(PM, RE, CE, users, items, m, coef))
    for a in (PM, RE, CE, users, items, cats, by_dish, PMr):
        a.setflags(write=False)
    return types.SimpleNamespace(PM=PM, PMr=PMr, RE=RE, CE=CE, users=users, items=items, cats=cats, by_dish=by_dish, refs=refs, coef=coef, E=E)


def visible_share(ref_rounded, ref_unrounded):
    """The share of the non-NaN pairs at which the two references are more than two assert_scores_close bounds apart."""
    ok = ~np.isnan(ref_rounded) & ~np.isnan(ref_unrounded)
    bound = TOL * np.maximum(1.0, np.abs(ref_rounded[ok]))
    return float(np.mean(np.abs(ref_unrounded[ok] - ref_rounded[ok]) > 2 * bound))


def option_error_bound(PM, RE, CE, users, items, cats, coef):
    """The documented bound of the option on |score(rounded) - score(unrounded)|, per pair:
        2^-8 (|a| sum|high-level terms| + |b| sum|low-level terms|) / n
    Every term is (mask weight) x (a Personal_Memory value) x (a Category_Embedding / Recipe_Embedding value); RNE moves the
    Personal_Memory factor by at most 2^-9 of itself, so the sums move by at most 2^-9 of the sums of the terms' magnitudes; a
    factor 2 of slack.  (Values that rounding sends to inf, or subnormals, are outside it; the recipes hold neither.)"""
    from oracle import m2d_oracle as oracle
    a32, b32 = oracle.blend_coefficients(coef)
    PMd, REd, CEd, m = (np.asarray(x, np.float64) for x in (PM, RE, CE, cats))
    um = PMd[users]
    high = np.abs(m[:, :, None] * um[:, :1, :] * CEd[None, :, :]).sum(axis=(1, 2))
    low = np.abs(m[:, :, None] * um[:, 1:, :] * REd[items][:, None, :]).sum(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 ** -8 * (abs(float(a32)) * high + abs(float(b32)) * low) / np.abs(m.sum(axis=1))
