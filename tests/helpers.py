"""Shared test helpers.  The oracle is the checker here and nowhere else."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star tolerance: scores match "within 1e-4 fp32"; stated as absolute-or-relative because
# |score| grows with E and table magnitude ("Reduction order").
TOL = 1e-4

# high_level_score_coefficient values the parity tests run beside the reference's default 0.99 (Train_recommender.py:61-62;
# `1 - coef` is taken in float32, Model_Recommender.py:17, :96): low level only, an even blend, a heavier low level than the
# default, high level only (every dish of a mask pattern then scores the same), and a NEGATIVE low-level weight.
COEFS = [0.0, 0.5, 0.9, 1.0, 1.25]


def assert_scores_close(got, ref, tol=TOL, what=""):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), "%s: NaN positions differ (%d vs %d)" % (what, nan_g.sum(), nan_r.sum())
    ok = ~nan_r
    err = np.abs(got[ok] - ref[ok])
    bound = tol * np.maximum(1.0, np.abs(ref[ok]))
    assert np.all(err <= bound), "%s: max err %.3e (bound %.1e)" % (what, err.max(), tol)
    return float(err.max()) if err.size else 0.0


def assert_scores_match_nonfinite(got, ref, tol=TOL, what=""):
    """assert_scores_close for results that may hold +-inf as well (tables with inf in them): NaN at the same pairs, the
    same infinities, the finite scores within the tolerance."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN positions differ (%d vs %d)" % (what, np.isnan(got).sum(), np.isnan(ref).sum())
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), "%s: infinities differ" % what
    fin = np.isfinite(ref)
    return assert_scores_close(got[fin], ref[fin], tol, what)


def score_cases():
    return sorted(glob.glob(os.path.join(GOLDEN, "score_*.npz")))


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def random_case(U, I, C, E, B, seed, zero_rows=True):
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(E)
    PM = (rng.standard_normal((U, C + 1, E)) * s).astype(np.float32)
    RE = (rng.standard_normal((I, E)) * s).astype(np.float32)
    CE = (rng.standard_normal((C, E)) * s).astype(np.float32)
    users = rng.integers(0, U, B).astype(np.int32)
    items = rng.integers(0, I, B).astype(np.int32)
    cats = rng.integers(0, 2, (B, C)).astype(np.float32)
    if not zero_rows:
        cats[cats.sum(1) == 0, 0] = 1.0
    return PM, RE, CE, users, items, cats


def write_case(U, I, C, E, L, B, seed, weighted=False):
    """Inputs of one Write_Memory call: random_case's tables and pairs, a General_Memory, +-1 write signs and labels
    (every pair has at least one).  `weighted`: label weights from {0, 0.5, 1, 2} and each pair's mask scaled by
    uniform(0.5, 2) -- the placeholders are float, the kernels multiply by them."""
    PM, RE, CE, users, items, cats = random_case(U, I, C, E, B, seed, zero_rows=False)
    rng = np.random.default_rng(seed + 1000)
    GM = (rng.standard_normal((L, C + 1, E)) / 4).astype(np.float32)
    sign = np.where(rng.random(B) < 0.6, 1.0, -1.0).astype(np.float32)
    if weighted:
        y = rng.choice(np.array([0, 0, 0, 0.5, 1, 2], np.float32), (B, L))
        cats = (cats * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32)
    else:
        y = (rng.random((B, L)) < 0.2).astype(np.float32)
    y[y.sum(1) == 0, 0] = 1
    return PM, RE, CE, GM, users, items, cats, sign, y


def containment_case(U, I, C, E, L, B, seed, bad=np.inf, zero=0.0):
    """write_case with one non-finite element: Recipe_Embedding[5, 3] = `bad`.  Dish 5 is written by pair 7 alone, whose mask
    is [1, zero, 1, zero] (C = 4), whose one label is 4 and whose user, U - 1, no other pair of the batch has."""
    PM, RE, CE, GM, users, items, cats, sign, y = write_case(U, I, C, E, L, B, seed)
    items[items == 5] = 6
    users[users == U - 1] = 0
    users[7], items[7] = U - 1, 5
    cats[7] = [1.0, zero, 1.0, zero]
    y[7] = 0
    y[7, 4] = 1
    RE[5, 3] = bad
    return PM, RE, CE, GM, users, items, cats, sign, y


# ---- the MLP head (tests/test_gpu_mlp.py, tests/test_mlp_checks_cpu.py, tests/test_gpu_readers_after_writers.py) ---------
# The share of pairs that must move by more than 10 bounds when one 32-value k-period of one block is lost.  A condition on
# the INPUTS of a comparison (tables, masks, head, blend), evaluated with the oracle alone; not a tolerance on any kernel.
MLP_VISIBLE = 0.8


def mlp_head(K, H1, H2, rng, scale=1.0):
    """A random head (W1, b1, W2, b2, w3, b3); scale 4 makes the head's share of the score a large one."""
    W1 = (rng.standard_normal((K, H1)) * scale / np.sqrt(K)).astype(np.float32)
    b1 = (rng.standard_normal(H1) * 0.1).astype(np.float32)
    W2 = (rng.standard_normal((H1, H2)) * scale / np.sqrt(H1)).astype(np.float32)
    b2 = (rng.standard_normal(H2) * 0.1).astype(np.float32)
    w3 = (rng.standard_normal(H2) * scale / np.sqrt(H2)).astype(np.float32)
    return W1, b1, W2, b2, w3, 0.25


def mlp_periods(E):
    """The k-periods of one block of E values: whole periods of 32, a remainder joined to the last one (E < 32: one period).
    The kernels that walk a block period by period exist for E % 32 == 0 only; elsewhere a lost period has no counterpart in
    the code and the remainder alone (8 values of E = 200) would measure the table scale, not the inputs' visibility."""
    n = max(1, E // 32)
    return [(32 * p, 32 * (p + 1) if p < n - 1 else E) for p in range(n)]


def mlp_visibility(PM, RE, CE, cats, head, users, items, coef, dish_high=None, detail=False):
    """How visible a lost k-period is in the scores of these pairs, in float64 with the oracle's expressions only.

    For every block b in 0 .. C and every period of that block (mlp_periods): that period of PM[:, b] zeroed -- which is what
    a stale pattern byte, a skipped ring stage or a z set from another tile does to a score -- and the share of the AFFECTED
    pairs whose score moves by more than 10 TOL max(1, |ref|).  Affected: every pair with a finite score for block 0, those
    with cats[d, b - 1] != 0 for a low-level block (elsewhere the block's z is zero whatever the user row holds).  Returns the
    minimum share over (block, period); `detail`: the whole {(block, period): share}.  Block 0 is skipped when an ingredient
    table (`dish_high`) replaces it.

    Zeroing PM[:, b, lo:hi] zeroes z there, and layer 1 is linear in z: the altered score comes from the pre-activations
    minus that period's product instead of from a second pass over all K (test_mlp_checks_cpu.py checks the identity
    against oracle.inference_mlp on altered tables)."""
    from oracle import m2d_oracle as oracle
    W1, b1, W2, b2, w3 = (np.asarray(x, np.float64) for x in head[:5])
    b3 = float(head[5])
    PMd = np.asarray(PM, np.float64)
    cats = np.asarray(cats).reshape(len(RE), -1)
    C, E = cats.shape[1], PMd.shape[2]
    users = np.asarray(users, np.int64); items = np.asarray(items, np.int64)
    Dt = oracle.dish_vectors(RE, CE, cats, coef, np.float64)
    if dish_high is not None:
        Dt[:, :E] = np.float64(oracle.blend_coefficients(coef)[0]) * np.asarray(dish_high, np.float64)
    with np.errstate(invalid="ignore"):
        z = PMd[users].reshape(len(users), -1) * Dt[items]
        pre1 = z @ W1 + b1
        tail = lambda pre: np.maximum(np.maximum(pre, 0) @ W2 + b2, 0) @ w3 + b3
        base = z.sum(axis=1)
        ref = base + tail(pre1)
    finite = np.isfinite(ref)
    out = {}
    for b in range(C + 1):
        if b == 0 and dish_high is not None:
            continue
        aff = finite if b == 0 else finite & (cats[items, b - 1] != 0)
        if not aff.any():
            continue
        thr = 10.0 * TOL * np.maximum(1.0, np.abs(ref[aff]))
        for p, (lo, hi) in enumerate(mlp_periods(E)):
            ks = slice(b * E + lo, b * E + hi)
            zz = z[aff, ks]
            alt = base[aff] - zz.sum(axis=1) + tail(pre1[aff] - zz @ W1[ks])
            out[(b, p)] = float(np.mean(np.abs(alt - ref[aff]) > thr))
    assert out, "mlp_visibility: no pair with a finite score"
    return out if detail else min(out.values())


def mlp_case(PM, RE, CE, cats, head, users, items, coef, dish_high=None):
    """What assert_mlp_scores compares against: tables, masks by dish, head, the pairs (GLOBAL user ids into PM) and the blend.
    `cache`: references by pick, so that tests which share a case compute each once."""
    import types
    return types.SimpleNamespace(PM=PM, RE=RE, CE=CE, cats=cats, head=head, users=np.asarray(users), items=np.asarray(items),
                                 coef=coef, dish_high=dish_high, cache={})


def assert_mlp_scores(got, case, pick=None, what=""):
    """Scores of the MLP head against oracle.inference_mlp (float64) (`got`: one score per pair of the case; `pick`: the
    positions compared, all of them if None), under assert_scores_close's bound -- AND the condition that makes
    that bound mean something for the low-level blocks: on at most 2 048 of the compared pairs, evenly spaced,
    mlp_visibility >= MLP_VISIBLE.  At the default blend 0.99 the C low-level blocks carry weight 0.01 and a kernel that loses
    a whole period of one stays inside the bound for a third to two thirds of the pairs it touches; such
    inputs are refused here whatever the kernel returned.  Returns (max error, visibility)."""
    from oracle import m2d_oracle as oracle
    got = np.asarray(got)
    users, items = case.users, case.items
    if pick is not None:
        pick = np.asarray(pick, np.int64)
        got, users, items = got[pick], users[pick], items[pick]
    key = None if pick is None else (pick.shape[0], hash(pick.tobytes()))
    if key not in case.cache:
        ref = oracle.inference_mlp(case.PM, case.RE, case.CE, case.cats, *case.head, users, items, coef=case.coef,
                                   dish_high=case.dish_high)
        n = len(users)
        sub = np.arange(n) if n <= 2048 else np.linspace(0, n - 1, 2048).astype(np.int64)
        vis = mlp_visibility(case.PM, case.RE, case.CE, case.cats, case.head, users[sub], items[sub], case.coef, case.dish_high)
        case.cache[key] = (ref, vis)
    ref, vis = case.cache[key]
    err = assert_scores_close(got, ref, what=what)
    assert vis >= MLP_VISIBLE, "%s: visibility %.2f < %.1f -- at these inputs (blend %g) a lost k-period stays inside the bound" % (
        what, vis, MLP_VISIBLE, case.coef)
    return err, vis


# ---- training step (tests/test_gpu_train.py, tests/test_train_oracle.py) ------------------------------------------------
# |got - ref| <= rho |ref - ini| + phi max(1, |ref|).  (rho, phi): 4 x what the float32-mode oracle needs against the float64
# one over every case of the training tests -- the measured maxima and the procedure are in test_gpu_train.py's docstring.
TRAIN_RHO, TRAIN_PHI = 5.8e-3, 6.5e-7                # sgd, adagrad, rmsprop
TRAIN_RHO_ADAM, TRAIN_PHI_ADAM = 1.0e-3, 4.5e-6      # adam: m / (sqrt(v) + eps) magnifies the last bits of gradients that cancel
TRAIN_SLOT_RHO, TRAIN_SLOT_PHI = 7.2e-4, 1.4e-6      # optimizer slots, phi on the slot's own scale (assert_train_slots)
TRAIN_PARTS = ("PM high", "PM low", "RE", "CE")


def train_parts(tables):
    """The four gradient paths of a step as views of (Personal_Memory, Recipe_Embedding, Category_Embedding)."""
    PM, RE, CE = tables
    return (("PM high", PM[:, :1, :]), ("PM low", PM[:, 1:, :]), ("RE", RE), ("CE", CE))


def train_batches(U, I, C, B, steps, seed, fractional=False, distinct=False, user_base=0):
    """`steps` batches of B pairs: a quarter of the pairs on one user and three eighths on one dish (duplicate ids: their rows
    must be summed), 0/1 masks with one pair's halved (masks are weights).  `fractional`: a few labels of 0.25 / 0.75.
    `distinct`: ids drawn without replacement apart from a hot block of 64 pairs (needs U, I >= B)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        if distinct:
            users = rng.permutation(U)[:B].astype(np.int32)
            items = rng.permutation(I)[:B].astype(np.int32)
            users[:64] = users[0]
            items[32:96] = items[32]
        else:
            users = rng.integers(0, U, B).astype(np.int32)
            items = rng.integers(0, I, B).astype(np.int32)
            users[: B // 4] = users[0]
            items[B // 8: B // 2] = items[B // 8]
        cats = rng.integers(0, 2, (B, C)).astype(np.float32)
        cats[cats.sum(1) == 0, rng.integers(0, C)] = 1.0
        cats[B // 3] *= 0.5
        labels = rng.integers(0, 2, B).astype(np.float32)
        if fractional:
            labels[1::7] = 0.25
            labels[B // 2] = 0.75
        out.append((users + np.int32(user_base), items, cats, labels))
    return out


def train_bound(ref, ini, learner, rho=None, phi=None):
    rho = (TRAIN_RHO_ADAM if learner == "adam" else TRAIN_RHO) if rho is None else rho
    phi = (TRAIN_PHI_ADAM if learner == "adam" else TRAIN_PHI) if phi is None else phi
    return rho * np.abs(ref - ini) + phi * np.maximum(1.0, np.abs(ref))


def train_visibility(ref, ini, learner, rho=None, phi=None):
    """Per part: the share of the elements the oracle moved that moved by more than 10 times their bound (None: none moved)."""
    out = {}
    for (name, r), (_, i) in zip(train_parts(ref), train_parts(ini)):
        r = np.asarray(r, np.float64); i = np.asarray(i, np.float64)
        moved = r != i
        out[name] = float((np.abs(r - i)[moved] > 10.0 * train_bound(r, i, learner, rho, phi)[moved]).mean()) if moved.any() else None
    return out


def assert_train_tables(got, ref, ini, learner, visible=TRAIN_PARTS, rho=None, phi=None, what=""):
    """Tables after some training steps against the float64 restatement's.  got / ref / ini: (Personal_Memory,
    Recipe_Embedding, Category_Embedding) as the engine left them, as the oracle left them, as both started.

    Per part (Personal_Memory's high row, its low rows, Recipe_Embedding, Category_Embedding):
      * |got - ref| <= rho |ref - ini| + phi max(1, |ref|), element by element;
      * what the oracle did not move is bit-equal to `ini` -- element by element for sgd / adagrad / rmsprop (a zero gradient
        is an exact zero), whole rows for adam (TF 1.x Adam moves every element of a row that has history);
      * for the parts named in `visible`: at least 90 % of the moved elements moved by more than 10 bounds, so an engine that
        halves, doubles, drops or misplaces that part's gradient cannot pass.  Asserted on ref and ini alone."""
    vis = train_visibility(ref, ini, learner, rho, phi)
    stats = {}
    for (name, g), (_, r), (_, i) in zip(train_parts(got), train_parts(ref), train_parts(ini)):
        g = np.asarray(g); r = np.asarray(r, np.float64); i32 = np.asarray(i); i = i32.astype(np.float64)
        assert g.shape == r.shape == i.shape, (what, name, g.shape, r.shape)
        moved = r != i
        if name in visible:
            assert vis[name] is None or vis[name] >= 0.9, "%s %s: only %.2f of the moved elements are visible" % (what, name, vis[name])
        still = ~moved if learner != "adam" else np.broadcast_to(~moved.any(axis=-1, keepdims=True), moved.shape)
        assert np.array_equal(g[still], i32[still].astype(g.dtype)), "%s %s: %d elements the oracle left alone changed" % (
            what, name, int((g[still] != i32[still]).sum()))
        err = np.abs(g.astype(np.float64) - r)
        bound = train_bound(r, i, learner, rho, phi)
        bad = err > bound
        assert not bad.any(), "%s %s: %d of %d outside the bound, worst err %.3e (moved %.3e, bound %.3e)" % (
            what, name, int(bad.sum()), bad.size, err[bad].max(), np.abs(r - i)[bad][err[bad].argmax()], bound[bad][err[bad].argmax()])
        stats[name] = {"moved": int(moved.sum()), "visible": vis[name], "err": float(err.max())}
    return stats


TRAIN_SLOT_INIT = {"adam": (0.0, 0.0), "adagrad": (0.1,), "rmsprop": (1.0, 0.0), "sgd": ()}


def assert_train_slots(got, ref, learner, rho=None, phi=None, what=""):
    """Optimizer slots against the oracle's, [table][slot]: adam m, v (start at 0); adagrad's accumulator (0.1); rmsprop's rms
    (1) and momentum (0).  The same form of bound on the slot's OWN scale -- Adam's v is g^2, 1e-9 to 3e-6, and a floor of
    phi max(1, |ref|) would let a v that was never written pass:

        |got - ref| <= rho |ref - ini| + phi S,     S = max(|ini|, max |ref| over that slot of that table)

    and what the oracle left at its initial value is bit-equal to it.  TRAIN_SLOT_RHO / TRAIN_SLOT_PHI: 4 x what the float32
    oracle needs, measured like the tables' pair over the same cases."""
    rho = TRAIN_SLOT_RHO if rho is None else rho
    phi = TRAIN_SLOT_PHI if phi is None else phi
    for tb, (gs, rs) in enumerate(zip(got, ref)):
        assert len(gs) == len(rs) == len(TRAIN_SLOT_INIT[learner]), (what, tb)
        for sl, (g, r, v0) in enumerate(zip(gs, rs, TRAIN_SLOT_INIT[learner])):
            g = np.asarray(g, np.float64).reshape(np.shape(r)); r = np.asarray(r, np.float64)
            i = np.full_like(r, np.float64(np.float32(v0)))
            still = (r == v0) | (r == i)                    # (the float64 oracle starts adagrad at the double 0.1)
            assert np.array_equal(g[still], i[still]), "%s slot %d of table %d: values the oracle left alone changed" % (what, sl, tb)
            err = np.abs(g - r)
            bound = rho * np.abs(r - i) + phi * max(abs(float(np.float32(v0))), float(np.abs(r).max()))
            bad = err > bound
            assert not bad.any(), "%s slot %d of table %d: %d of %d outside the bound, worst err %.3e (bound there %.3e)" % (
                what, sl, tb, int(bad.sum()), bad.size, err[bad].max(), bound[bad][err[bad].argmax()])


def _train_lr(B, E=0):
    """sgd / adagrad / rmsprop move a row by about lr * g, and g falls with 1 / B and with the table scale 1 / sqrt(E)."""
    return (0.5 if B <= 128 else 8.0) * (8.0 if E >= 512 and B <= 128 else 1.0)


def train_lr(lr, learner):
    """Adam moves every element by about lr whatever the gradient: it keeps the small rate."""
    return 0.01 if learner == "adam" else lr


ALL_LEARNERS = ("adam", "sgd", "adagrad", "rmsprop")
# test_train_steps_match_restatement's shapes (U, I, C, E, B, "variant" option)
TRAIN_SHAPES = [(300, 100, 4, 32, 128, 0), (64, 40, 4, 200, 8, 0), (50, 30, 3, 6, 257, 0), (2000, 500, 4, 64, 4096, 0),
                (300, 100, 4, 32, 128, 14), (64, 40, 4, 200, 1000, 0), (64, 40, 4, 200, 1000, 14)]
FUSED, NINE = "m2d_train_grad_fused", "m2d_train_grad"


def train_launch_cases(cus=256):
    """The cases of test_gpu_train.py::test_train_launches_that_never_ran, by name.  `cus`: the device's compute units (the
    grad kernel's grid stops at 8 blocks = 32 waves per unit).  Every case: blend 0.5, lr by batch size (see
    assert_train_tables: what makes every gradient path visible), three steps of every learner unless it says otherwise."""
    W = 32 * cus
    case = lambda U, I, C, E, B, kernel, **kw: dict(dict(U=U, I=I, C=C, E=E, B=B, kernel=kernel, form=0, steps=3, learners=ALL_LEARNERS,
                                                         coef=0.5, lr=_train_lr(B, E), distinct=False, user_base=0, then_fused=False), **kw)
    return {
        # rows that are no multiple of 4 floats in the nine-launch form: m2d_train_apply<*, 1>
        "vec1_re_ce": case(50, 30, 3, 6, 1100, NINE),
        "vec1_all": case(40, 30, 4, 7, 257, NINE, form=14),
        # 16 C E bytes above 48 KiB: dCE through global atomics, no m2d_train_reduce_ce, the fused form refused
        "ce_global_b200": case(600, 200, 4, 772, 200, NINE),
        "ce_global_b1100": case(600, 200, 4, 772, 1100, NINE),
        "ce_global_c13": case(600, 200, 13, 250, 300, NINE),
        # the fused form at its LDS limit, and the first E past it
        "fused_lds_limit": case(300, 100, 4, 768, 128, FUSED),
        "past_lds_limit": case(300, 100, 4, 772, 128, NINE, steps=1),
        # waves of the grad kernel own 2 or 3 pairs
        "pairs_per_wave": case(3000, 700, 3, 6, 2 * W + 77, NINE),
        "pairs_per_wave_e64": case(3000, 700, 4, 64, 2 * W + 77, NINE, learners=("sgd", "adam"), steps=2, lr=32.0),
        # more rows than waves: m2d_train_apply<true, 4> over all users; <false, 4> and both cleanups over the claimed rows
        "adam_rows_loop": case(W + 1500, 300, 4, 8, 1100, NINE, learners=("adam",), then_fused=True),
        "claimed_rows_loop": case(3 * W, 3 * W, 4, 8, 2 * W + 77, NINE, learners=("sgd", "adagrad"), steps=2, distinct=True,
                                  then_fused=True, lr=32.0),
        # one user-range shard
        "shard_nine": case(300, 100, 4, 32, 1100, NINE, user_base=7000),
        "shard_fused": case(300, 100, 4, 32, 128, FUSED, user_base=7000),
    }


def train_visible_cases():
    """test_train_steps_every_path_visible: every shape of TRAIN_SHAPES at blend 0.5, three at 0 (no high-level gradient: the
    high row and Category_Embedding stay bit-equal), one at 1.25 (a negative low-level weight) and two at the default 0.99."""
    out = [(s, 0.5) for s in TRAIN_SHAPES]
    out += [(TRAIN_SHAPES[0], 0.0), (TRAIN_SHAPES[2], 0.0), (TRAIN_SHAPES[4], 0.0), (TRAIN_SHAPES[0], 1.25)]
    out += [(TRAIN_SHAPES[0], 0.99), (TRAIN_SHAPES[3], 0.99)]      # the default blend: the high row and CE visible, the rest compared
    return [s + (c, _train_lr(s[4], s[3]) * (4.0 if c > 1 else 1.0)) for s, c in out]


def train_visible_parts(coef, learner, lr):
    """The parts on which a case must meet assert_train_tables' visibility condition.  Adam moves every element by about lr:
    all four.  The others move a row by lr * g: at the default blend the low-level gradient is 1 / 100 of the high-level one and
    only the high row and Category_Embedding can be visible; at lr = 0.01 (the cases kept from before the condition) those two
    meet it on some shapes and not on others (the high row 0.63 at (300, 100, 4, 32, 128)), so it is not asserted there."""
    if learner == "adam":
        return TRAIN_PARTS
    if lr <= 0.01:
        return ()
    return ("PM high", "CE") if coef == 0.99 else TRAIN_PARTS


def run_train_oracle(spec, learner, dtype=np.float64, cls=None):
    """The oracle's side of one case of train_launch_cases: (initial tables, batches, state after the steps, [(loss, norm)])."""
    from oracle import train_oracle as T
    U, I, C, E, B = (spec[k] for k in "UICEB")
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=U + E)
    ini = (PM * 3, RE * 3, CE * 3)
    batches = train_batches(U, I, C, B, spec["steps"], seed=B, fractional=True, distinct=spec["distinct"])
    if spec["then_fused"]:
        batches += train_batches(U, I, C, 64, 1, seed=B + 1, fractional=True)
    st = (cls or T.TrainState)(*ini, learner, train_lr(spec["lr"], learner), coef=spec["coef"], dtype=dtype)
    outs = [st.step(*b) for b in batches]
    return ini, batches, st, outs


# ---- non-finite tables (tests/test_nonfinite_cases_cpu.py, tests/test_gpu_nonfinite.py) ---------------------------------
NONFINITE_TABLES = ("U_high", "U_low", "RE", "CE")
NONFINITE_COLS = ("first", "last")
NONFINITE_VALUES = (np.inf, -np.inf, np.nan)
NONFINITE_U, NONFINITE_I = 400, 300
# E of the C = 4 pair kernels: partial lane groups (E / 4 of 8 / 16 / 32 / 64 lanes) and full ones
NONFINITE_E_PARTIAL, NONFINITE_E_FULL = (24, 48, 100, 200), (32, 64, 128, 256)
_NONFINITE_BASE = {}


def nonfinite_patterns(C, rng):
    """The 20 masks of the hand-built pairs: all categories, four weighted masks with every weight non-zero, the empty mask,
    then 14 more 0/1 patterns (C = 4: with the first one, all 15 non-empty ones).  The masks a +-inf score needs come first, so
    that 64 pairs that cycle through the list hold them in pairs 0..7 and in pairs 56..63."""
    full = 2 ** C - 1
    rest = list(range(1, full)) if full - 1 <= 14 else [1 << c for c in range(C)] + [int(x) for x in rng.choice(
        np.setdiff1d(np.arange(1, full), 1 << np.arange(C)), 14 - C, replace=False)]
    rest = (rest * 14)[:14]                                        # C = 3 has 6 of them: repeated
    bits = lambda p: (p >> np.arange(C) & 1).astype(np.float32)
    out = [bits(full)] + [rng.uniform(0.5, 2.0, C).astype(np.float32) for _ in range(4)] + [bits(0)] + [bits(p) for p in rest]
    return np.stack(out)


def _nonfinite_base(C, E, B, seed, U, I):
    key = (C, E, B, seed, U, I)
    if key not in _NONFINITE_BASE:
        PM, RE, CE, users, items, cats = random_case(U, I, C, E, B, seed)
        rng = np.random.default_rng(seed + 7919)
        u, d, c = int(rng.integers(0, U)), int(rng.integers(0, I)), int(rng.integers(0, C))
        for e in (1, E - 1):                                       # one-signed partners of the element that is poisoned:
            CE[:, e] = np.abs(CE[:, e])                            # U_high[u, e] = inf -> sum_c m_c CE_c[e] inf is inf, not inf - inf
            PM[u, 1:, e] = np.abs(PM[u, 1:, e])                    # RE[d, e] = inf -> sum_c m_c U_low[u, c, e] inf likewise
        pat = nonfinite_patterns(C, rng)
        n = min(64, B)
        users[:n] = u
        items[:n] = d                                              # (U_high / U_low / CE: any dish would do)
        cats[:n] = pat[np.arange(n) % len(pat)]
        users[n:n + 8] = u                                         # other pairs of the poisoned user and of the poisoned dish
        items[n + 8:n + 16] = d
        for a in (PM, RE, CE, users, items, cats):
            a.setflags(write=False)
        _NONFINITE_BASE[key] = (PM, RE, CE, users, items, cats, u, d, c, {})
        if len(_NONFINITE_BASE) > 4:                               # (tests walk the shapes one after another)
            del _NONFINITE_BASE[next(iter(_NONFINITE_BASE))]
    return _NONFINITE_BASE[key]


def nonfinite_case(C, E, B, table, col, value, seed, U=NONFINITE_U, I=NONFINITE_I, ref_on=None, dish_cats=None):
    """random_case(U, I, C, E, B, seed) with ONE table element set to `value` (+inf, -inf or NaN), and the float64 reference.

    table: "U_high" (PM[u, 0, e]), "U_low" (PM[u, 1 + c, e]), "RE" (RE[d, e]), "CE" (CE[c, e]) for one user u, dish d and
    category c drawn from the seed.  col: "first" -- e = 1, inside the float4 column that the idle lanes of a partial lane group
    read again -- or "last", e = E - 1.

    The first 64 pairs are (u, d) under nonfinite_patterns' 20 masks in turn: the pairs of the first and of the last lane group of
    a wavefront hold the masks whose score is +-inf.  So that it is +-inf and not inf - inf, the partner factors are one-signed
    at e = 1 and e = E - 1 in the clean tables already: |CE[:, e]| (U_high) and |PM[u, 1:, e]| (RE).  The rest of the batch is
    random_case's, with 8 more pairs of u and 8 more of d.

    Returns a namespace: PM, RE, CE (poisoned), PM0, RE0, CE0 (clean), users, items, cats, u, d, c, e, ref (float64,
    oracle.inference_f64 on the poisoned tables), ref0 (on the clean ones), touched (pairs that read the poisoned element's
    row).  ref_on: pair indices; ref / ref0 / touched then cover those pairs only (large batches).  dish_cats [I, C]: the masks
    come from this table by dish instead (`score_pairs_bydish`; the hand-built pairs then all carry dish d's mask)."""
    import types
    from oracle import m2d_oracle as oracle
    assert table in NONFINITE_TABLES and col in NONFINITE_COLS
    PM0, RE0, CE0, users, items, cats, u, d, c, cache = _nonfinite_base(C, E, B, seed, U, I)
    if dish_cats is not None:
        cats = np.asarray(dish_cats, np.float32).reshape(I, C)[items]
    e = 1 if col == "first" else E - 1
    PM, RE, CE = PM0, RE0, CE0
    if table in ("U_high", "U_low"):
        PM = PM0.copy(); PM[u, 0 if table == "U_high" else 1 + c, e] = value
    elif table == "RE":
        RE = RE0.copy(); RE[d, e] = value
    else:
        CE = CE0.copy(); CE[c, e] = value
    sel = np.arange(B) if ref_on is None else np.asarray(ref_on, np.int64)
    rkey = (None if ref_on is None else sel.tobytes(), None if dish_cats is None else np.asarray(dish_cats, np.float32).tobytes())
    if rkey not in cache:
        ref0 = oracle.inference_f64(PM0, RE0, CE0, users[sel], items[sel], cats[sel])
        ref0.setflags(write=False)
        cache[rkey] = ref0
    ref0 = cache[rkey]
    touched = {"U_high": users[sel] == u, "U_low": users[sel] == u, "RE": items[sel] == d, "CE": np.ones(len(sel), bool)}[table]
    ref = ref0.copy()
    t = sel[touched]
    ref[touched] = oracle.inference_f64(PM, RE, CE, users[t], items[t], cats[t])
    return types.SimpleNamespace(PM=PM, RE=RE, CE=CE, PM0=PM0, RE0=RE0, CE0=CE0, users=users, items=items, cats=cats,
                                 u=u, d=d, c=c, e=e, ref=ref, ref0=ref0, touched=touched, table=table, col=col, value=value)


def nonfinite_case_conditions(case):
    """What a case must hold to be worth a launch (the float64 reference alone): see test_nonfinite_cases_cpu.py."""
    ref, ref0 = case.ref, case.ref0
    by_poison = np.isnan(ref) & np.isfinite(ref0)
    assert by_poison.sum() >= 8, (case.table, case.col, case.value, int(by_poison.sum()))
    assert np.array_equal(ref[~case.touched], ref0[~case.touched], equal_nan=True)
    if np.isinf(case.value):
        assert np.isinf(ref).sum() >= 8, (case.table, case.col, case.value, int(np.isinf(ref).sum()))
        n = min(64, len(ref))
        assert np.isinf(ref[:8]).any() and np.isinf(ref[n - 8:n]).any()     # first and last lane group of the hand-built wave
    if case.table != "CE":
        assert np.isfinite(ref).mean() >= 0.5


def c4_lane_standin(PM, RE, CE, users, items, cats, coef=0.99, zero_idle_hs=True):
    """numpy stand-in of one lane group of the C = 4 pair kernels (m2d_score.hip): LPP = 8 / 16 / 32 / 64 lanes, lane j holds
    float4 column j of every row, lanes with j >= E / 4 read column 0 again with cef = 0; their `ls` is zeroed, their `hs` is
    zeroed or kept (`zero_idle_hs`); the group's sum is the xor butterfly.  float32 throughout (products and sums rounded
    separately where the kernel uses fma: far inside the 1e-4 bound)."""
    from oracle import m2d_oracle as oracle
    C, E = CE.shape
    assert C == 4 and E % 4 == 0 and E <= 256
    E4 = E // 4
    LPP = 8 if E4 <= 8 else 16 if E4 <= 16 else 32 if E4 <= 32 else 64
    j = np.arange(LPP)
    idle = j >= E4
    col = (np.where(idle, 0, j)[:, None] * 4 + np.arange(4)[None, :])                  # [LPP, 4] element index
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ub = PM[users][:, :, col]                                                      # [B, C + 1, LPP, 4]
        ib = RE[items][:, col]                                                         # [B, LPP, 4]
        cef = np.where(idle[None, :, None], f(0), CE[:, col])                          # [C, LPP, 4]
        m = cats.astype(f)
        hs = np.zeros((len(users), LPP), f); ls = np.zeros_like(hs)
        for c in range(C):
            dc = m[:, c, None, None] * cef[None, c]
            dm = m[:, c, None, None] * ub[:, c + 1]
            for q in range(4):
                hs = (hs + ub[:, 0, :, q] * dc[:, :, q]).astype(f)
                ls = (ls + ib[:, :, q] * dm[:, :, q]).astype(f)
        ls[:, idle] = 0
        if zero_idle_hs:
            hs[:, idle] = 0
        off = LPP // 2
        while off >= 1:
            hs = (hs + hs[:, j ^ off]).astype(f)
            ls = (ls + ls[:, j ^ off]).astype(f)
            off //= 2
        n = ((m[:, 0] + m[:, 1]) + (m[:, 2] + m[:, 3])).astype(f)
        a, b = oracle.blend_coefficients(coef)
        return (a * (hs[:, 0] / n) + b * (ls[:, 0] / n)).astype(f)
