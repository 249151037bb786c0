"""CPU checks of the training-step restatement (oracle/train_oracle.py).

TensorFlow is not in the image and the reference has no training fixture, so the restatement is PARITY UNPINNED.
What can be pinned on CPU: the analytic gradients against autograd over the op-for-op torch graph
(oracle/torch_graph.py), the sigmoid-CE formula against torch's, and the update rules' fixed points."""
import numpy as np
import pytest
import torch

from helpers import random_case
from oracle import torch_graph
from oracle import train_oracle as T


def _batch(seed, U=40, I=30, C=4, E=12, B=64):
    PM, RE, CE, users, items, cats = random_case(U, I, C, E, B, seed, zero_rows=False)
    rng = np.random.default_rng(seed + 1)
    cats = cats * rng.choice([1.0, 0.5, 2.0], size=cats.shape).astype(np.float32)      # masks are weights, not only 0/1
    cats[cats.sum(1) == 0, 1] = 1.0
    labels = rng.integers(0, 2, B).astype(np.float32)
    users[:8] = users[0]                                                               # duplicate ids in the batch
    items[4:12] = items[4]
    return PM * 4, RE * 4, CE * 4, users, items, cats, labels


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gradients_match_autograd_over_the_graph(seed):
    PM, RE, CE, users, items, cats, labels = _batch(seed)
    s, loss, dUM, dIt, dCE = T.loss_and_gradients(PM, RE, CE, users, items, cats, labels)
    tp, tr, tc = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (PM, RE, CE))
    logits = torch_graph.inference(tp, tr, tc, torch.tensor(users), torch.tensor(items), torch.tensor(cats, dtype=torch.float64))
    tl = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.tensor(labels, dtype=torch.float64))
    tl.backward()
    assert abs(loss - tl.item()) < 1e-12
    # torch_graph blends with float32 coefficients, as the reference does; so does the oracle
    np.testing.assert_allclose(s, logits.detach().numpy(), rtol=1e-12, atol=1e-12)
    gPM = np.zeros_like(PM, dtype=np.float64); np.add.at(gPM, users, dUM)
    gRE = np.zeros_like(RE, dtype=np.float64); np.add.at(gRE, items, dIt)
    np.testing.assert_allclose(gPM, tp.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(gRE, tr.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dCE, tc.grad.numpy(), rtol=1e-10, atol=1e-14)


def test_learner_names_follow_the_reference_switch():
    assert T.learner_code("Adam") == T.ADAM and T.learner_code("adagrad") == T.ADAGRAD
    assert T.learner_code("RMSProp") == T.RMSPROP
    assert T.learner_code("sgd") == T.SGD and T.learner_code("momentum") == T.SGD      # the else branch (:234-235)


def test_clip_uses_per_pair_rows_and_leaves_small_gradients_alone():
    PM, RE, CE, users, items, cats, labels = _batch(3)
    st = T.TrainState(PM, RE, CE, "sgd", lr=0.5)
    _, _, dUM, dIt, dCE = T.loss_and_gradients(PM, RE, CE, users, items, cats, labels)
    loss, norm = st.step(users, items, cats, labels)
    assert norm == pytest.approx(np.sqrt((dUM ** 2).sum() + (dIt ** 2).sum() + (dCE ** 2).sum()))
    assert norm < 5.0                                       # scale = 5 * min(1/norm, 1/5) = 1: plain SGD
    gRE = np.zeros_like(RE, dtype=np.float64); np.add.at(gRE, items, dIt)
    np.testing.assert_allclose(st.RE, RE - 0.5 * gRE, rtol=1e-12, atol=1e-15)
    # blow the gradient up: the update is rescaled to global norm 5 over the per-pair rows
    big = T.TrainState(PM * 300, RE * 300, CE * 300, "sgd", lr=1.0)
    _, _, dUM, dIt, dCE = T.loss_and_gradients(big.PM, big.RE, big.CE, users, items, cats, labels)
    ce0 = big.CE.copy()
    _, norm = big.step(users, items, cats, labels)
    assert norm > 5.0
    np.testing.assert_allclose(big.CE, ce0 - dCE * (5.0 / norm), rtol=1e-10, atol=1e-12)


def test_adam_moves_every_row_and_first_step_is_lr_sized():
    PM, RE, CE, users, items, cats, labels = _batch(4)
    st = T.TrainState(PM, RE, CE, "adam", lr=0.001)
    st.step(users, items, cats, labels)
    touched = np.zeros(len(PM), bool); touched[users] = True
    d = np.abs(st.PM - PM)
    assert np.all(d[~touched] == 0)                         # m = v = 0 there: 0 / (0 + eps)
    hit = d[touched][:, 0, :]                               # the high-level row always has a gradient
    assert np.all(hit > 0.0009) and np.all(hit < 0.0011)    # lr_t m / (sqrt(v) + eps) ~ lr at t = 1
    # second step: rows untouched now, but with history, still move (TF 1.x Adam's sparse path is dense)
    before = st.PM.copy()
    other = np.resize(np.setdiff1d(np.arange(len(PM)), users), len(users)).astype(np.int32)
    st.step(other, items, cats, labels)
    only_first = touched.copy(); only_first[other] = False
    assert np.all(np.abs(st.PM - before)[only_first][:, 0, :] > 0)


@pytest.mark.parametrize("learner", ["adagrad", "rmsprop"])
def test_sparse_learners_touch_only_the_batch_rows(learner):
    PM, RE, CE, users, items, cats, labels = _batch(5)
    st = T.TrainState(PM, RE, CE, learner, lr=0.01)
    st.step(users, items, cats, labels)
    touched = np.zeros(len(RE), bool); touched[items] = True
    assert np.all(st.RE[~touched] == RE[~touched])
    assert np.all(np.abs(st.RE - RE)[touched].max(1) > 0)
    if learner == "adagrad":
        assert np.all(st.slots[1][0][~touched] == np.float64(0.1))
    else:
        assert np.all(st.slots[1][0][~touched] == 1.0)      # rms slot starts at one


def test_float32_mode_tracks_float64():
    PM, RE, CE, users, items, cats, labels = _batch(6)
    a, b = T.TrainState(PM, RE, CE, "adam"), T.TrainState(PM, RE, CE, "adam", dtype=np.float32)
    for _ in range(3):
        la, _ = a.step(users, items, cats, labels)
        lb, _ = b.step(users, items, cats, labels)
        assert abs(la - lb) < 1e-5
    assert np.abs(a.PM - b.PM).max() < 2e-5


@pytest.mark.parametrize("learner", ["sgd", "adagrad"])
def test_two_steps_match_torch_optim_where_the_rules_coincide(learner):
    """torch.optim.SGD and torch.optim.Adagrad(initial_accumulator_value=0.1, eps=0) apply the same formulas as the
    TF 1.x optimizers for these two learners (dense autograd gradients sum duplicate rows, as TF's
    _apply_sparse_duplicate_indices does; rows with a zero gradient do not move under either rule).  Adam and
    RMSProp differ between the libraries (epsilon placement, slot initial values) and are not compared."""
    PM, RE, CE, users, items, cats, labels = _batch(7)
    lr = 0.05
    st = T.TrainState(PM, RE, CE, learner, lr=lr)
    tp, tr, tc = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (PM, RE, CE))
    opt = (torch.optim.SGD([tp, tr, tc], lr=float(np.float32(lr))) if learner == "sgd" else
           torch.optim.Adagrad([tp, tr, tc], lr=float(np.float32(lr)), initial_accumulator_value=0.1, eps=0.0))
    for step in range(2):
        u = np.roll(users, step * 3); d = np.roll(items, step * 5)
        ref_loss, norm = st.step(u, d, cats, labels)
        assert norm < 5.0                                   # no clipping in this case: torch has none here
        opt.zero_grad()
        logits = torch_graph.inference(tp, tr, tc, torch.tensor(u), torch.tensor(d), torch.tensor(cats, dtype=torch.float64))
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.tensor(labels, dtype=torch.float64))
        loss.backward()
        opt.step()
        assert abs(loss.item() - ref_loss) < 1e-12
    for got, ref in ((st.PM, tp), (st.RE, tr), (st.CE, tc)):
        np.testing.assert_allclose(got, ref.detach().numpy(), rtol=1e-9, atol=1e-12)


# ---- the table comparison of the GPU tests (helpers.assert_train_tables): what it lets through and what it does not ----------
import functools

import helpers as H


class _RecipeEmbeddingNeverWritten(T.TrainState):
    def step(self, *batch, **kw):
        keep = self.RE.copy()
        out = super().step(*batch, **kw)
        self.RE[...] = keep
        return out


class _LowRowsOneCategoryOff(T.TrainState):
    """What a step adds to the low-level rows of category 0 lands on category 1's rows."""
    def step(self, *batch, **kw):
        before = self.PM.copy()
        out = super().step(*batch, **kw)
        delta = self.PM[:, 1, :] - before[:, 1, :]
        self.PM[:, 1, :] = before[:, 1, :]
        self.PM[:, 2, :] += delta
        return out


class _DuplicatesOverwritten(T.TrainState):
    """A row's gradient is its LAST pair's, not the sum over its pairs (sgd / adagrad / rmsprop).  `quiet_only`: the high
    row, the one path the earlier bound could see, is still summed."""
    quiet_only = False

    def step(self, users, items, categories, labels, apply=True):
        dt = self.dtype
        _, loss, dUM, dIt, dCE = T.loss_and_gradients(self.PM, self.RE, self.CE, users, items, categories, labels, self.coef, dt)
        norm = np.sqrt((dUM ** 2).sum() + (dIt ** 2).sum() + (dCE ** 2).sum())
        scale = self.clip * np.minimum(1.0 / norm, 1.0 / self.clip)
        for ids, vals, var, slots in ((users, dUM, self.PM, self.slots[0]), (items, dIt, self.RE, self.slots[1]),
                                      (None, dCE, self.CE, self.slots[2])):
            if ids is None:
                idx, g = slice(None), vals * scale
            else:
                idx = np.unique(ids)
                g = np.zeros((int(np.max(ids)) + 1,) + vals.shape[1:], dt)
                g[np.asarray(ids, np.int64)] = vals * scale             # the last writer wins
                if self.quiet_only and vals.ndim == 3:
                    g[:, 0, :] = 0
                    np.add.at(g[:, 0, :], np.asarray(ids, np.int64), vals[:, 0, :] * scale)
                g = g[idx]
            if self.rule == T.ADAGRAD:
                slots[0][idx] += g * g
                var[idx] -= self.lr * g / np.sqrt(slots[0][idx])
            elif self.rule == T.RMSPROP:
                slots[0][idx] += (g * g - slots[0][idx]) * (1 - dt(np.float32(0.9)))
                slots[1][idx] = self.lr * g / np.sqrt(slots[0][idx] + dt(np.float32(1e-10)))
                var[idx] -= slots[1][idx]
            else:
                assert self.rule == T.SGD
                var[idx] -= self.lr * g
        return loss, norm


class _QuietDuplicatesOverwritten(_DuplicatesOverwritten):
    quiet_only = True


STAND_INS = [_RecipeEmbeddingNeverWritten, _LowRowsOneCategoryOff, _DuplicatesOverwritten, _QuietDuplicatesOverwritten]
LINEAR = ("sgd", "adagrad", "rmsprop")
DETECTED = "outside the bound|left alone changed"           # (a visibility failure speaks of `ref` alone: it is no detection)


@functools.lru_cache(maxsize=None)
def _launch_case(name, learner, dtype=np.float64, cls=None):
    return H.run_train_oracle(H.train_launch_cases()[name], learner, dtype, cls)


@functools.lru_cache(maxsize=None)
def _shape_case(shape, coef, lr, learner, dtype=np.float64, cls=None):
    U, I, C, E, B, _ = shape
    PM, RE, CE, *_ = random_case(U, I, C, E, 1, seed=U + E)
    ini = (PM * 3, RE * 3, CE * 3)
    st = (cls or T.TrainState)(*ini, learner, lr, coef=coef, dtype=dtype)
    for b in H.train_batches(U, I, C, B, 3, seed=B):
        st.step(*b)
    return ini, st


def _tables(st):
    return (st.PM, st.RE, st.CE)


def test_duplicates_overwritten_stand_in_is_the_oracle_without_duplicates():
    PM, RE, CE, users, items, cats, labels = _batch(8)
    users, items = np.arange(len(users), dtype=np.int32) % len(PM), (np.arange(len(users), dtype=np.int32) * 7) % len(RE)
    keep = np.unique(users, return_index=True)[1]
    keep = keep[np.unique(items[keep], return_index=True)[1]]
    batch = [x[keep] for x in (users, items, cats, labels)]
    for learner in LINEAR:
        a, b = T.TrainState(PM, RE, CE, learner, 0.1), _DuplicatesOverwritten(PM, RE, CE, learner, 0.1)
        assert a.step(*batch) == b.step(*batch)
        for x, y in zip(_tables(a), _tables(b)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("name", sorted(H.train_launch_cases()))
def test_float32_oracle_passes_the_table_comparison_launch_cases(name):
    """TRAIN_RHO / TRAIN_PHI are 4 x what the float32-mode restatement needs: it passes on every case the GPU tests run, the
    visibility condition included."""
    for learner in H.train_launch_cases()[name]["learners"]:
        ini, _, ref, outs = _launch_case(name, learner)
        _, _, got, outs32 = _launch_case(name, learner, np.float32)
        H.assert_train_tables(_tables(got), _tables(ref), ini, learner, H.train_visible_parts(0.5, learner, 1.0), what="%s %s" % (name, learner))
        H.assert_train_slots(got.slots, ref.slots, learner, what="%s %s" % (name, learner))
        for (l64, n64), (l32, n32) in zip(outs, outs32):
            assert abs(l32 - l64) <= 1e-5 * max(1.0, abs(l64)) and abs(n32 - n64) <= 1e-5 * max(1.0, n64)


# (the "variant" = 14 shapes are left out: the option picks the launches, the oracle's case is the same)
@pytest.mark.parametrize("shape,coef,lr", [(c[:6], c[6], c[7]) for c in H.train_visible_cases() if c[5] != 14] +
                         [(s, 0.99, 0.01) for s in H.TRAIN_SHAPES if s[5] != 14])
def test_float32_oracle_passes_the_table_comparison_restatement_cases(shape, coef, lr):
    for learner in H.ALL_LEARNERS:
        rate = H.train_lr(lr, learner)
        ini, ref = _shape_case(shape, coef, rate, learner)
        _, got = _shape_case(shape, coef, rate, learner, np.float32)
        H.assert_train_tables(_tables(got), _tables(ref), ini, learner, H.train_visible_parts(coef, learner, lr), what=learner)
        H.assert_train_slots(got.slots, ref.slots, learner, what=learner)
        if coef == 0.0:                                     # no high-level gradient: nothing to compare but the bits
            assert np.array_equal(got.CE, ini[2]) and np.array_equal(got.PM[:, 0], ini[0][:, 0])


def _old_bound_passes(got, ref, learner, lr=0.01, steps=3):
    """test_train_steps_match_restatement's table check before this comparison replaced it."""
    tol = 1e-3 * lr * steps if learner in ("adam", "rmsprop") else 1e-5
    for g, r in zip(got, ref):
        bound = tol * np.maximum(1.0, np.abs(r)) if learner in ("sgd", "adagrad") else tol
        if not np.all(np.abs(g - r) <= bound):
            return False
    return True


@pytest.mark.parametrize("stand_in", STAND_INS, ids=lambda c: c.__name__.strip("_"))
def test_stand_ins_fail_the_table_comparison_and_passed_the_old_bound(stand_in):
    """Wrong engines.  Each fails helpers.assert_train_tables on every sgd / adagrad / rmsprop case the GPU tests run -- and
    passed the bound those tests had before (1e-5 max(1, |ref|); 3e-5 for rmsprop) on the cases they had before: at the
    default blend 0.99 and lr 0.01 that bound is wider than anything a step does to Recipe_Embedding or to a low-level row.
    Two limits of that second half, as measured: overwriting the duplicates of the HIGH row too moves it by 1e-4 to 3e-3
    and the earlier bound did catch that (asserted), so the stand-in that passed it overwrites on the quiet paths only; and
    adagrad's first steps are lr g / sqrt(0.1 + g^2), about 3 lr g: below 1000 pairs its quiet rows move by 1.1e-5 to 3.1e-5,
    just over the earlier 1e-5, so those cases are left out of the second half."""
    for name, spec in H.train_launch_cases().items():
        for learner in (l for l in spec["learners"] if l in LINEAR):
            ini, _, ref, _ = _launch_case(name, learner)
            _, _, got, _ = _launch_case(name, learner, np.float64, stand_in)
            with pytest.raises(AssertionError, match=DETECTED):
                H.assert_train_tables(_tables(got), _tables(ref), ini, learner, H.train_visible_parts(spec["coef"], learner, spec["lr"]),
                                      what=name)
    for case in H.train_visible_cases():
        if case[5] == 14:
            continue
        for learner in LINEAR:
            ini, ref = _shape_case(case[:6], case[6], case[7], learner)
            _, got = _shape_case(case[:6], case[6], case[7], learner, np.float64, stand_in)
            with pytest.raises(AssertionError, match=DETECTED):
                H.assert_train_tables(_tables(got), _tables(ref), ini, learner, H.train_visible_parts(case[6], learner, case[7]),
                                      what=str(case))
    for shape in H.TRAIN_SHAPES:
        if shape[5] == 14:
            continue
        for learner in LINEAR:
            ini, ref = _shape_case(shape, 0.99, 0.01, learner)
            _, got = _shape_case(shape, 0.99, 0.01, learner, np.float64, stand_in)
            if stand_in is _DuplicatesOverwritten:
                assert not _old_bound_passes(_tables(got), _tables(ref), learner), (shape, learner)
            elif learner != "adagrad" or shape[4] >= 1000:
                assert _old_bound_passes(_tables(got), _tables(ref), learner), (shape, learner)


@pytest.mark.parametrize("name", sorted(H.train_launch_cases()))
def test_a_slot_never_written_or_moved_twice_as_far_fails_the_slot_comparison(name):
    """helpers.assert_train_slots on every launch case: the float32 oracle's slots pass (asserted above); with any ONE slot of
    any one table left at its initial value, or moved twice as far from it, they do not -- Adam's v, which is g^2, included."""
    for learner in (l for l in H.train_launch_cases()[name]["learners"] if l != "sgd"):
        _, _, ref, _ = _launch_case(name, learner)
        _, _, good, _ = _launch_case(name, learner, np.float32)
        for tb in range(3):
            for sl, v0 in enumerate(H.TRAIN_SLOT_INIT[learner]):
                for wrong in (np.full_like(good.slots[tb][sl], v0), np.float32(v0) + 2 * (good.slots[tb][sl] - np.float32(v0))):
                    got = [[wrong if (t, k) == (tb, sl) else x for k, x in enumerate(row)] for t, row in enumerate(good.slots)]
                    with pytest.raises(AssertionError, match="outside the bound"):
                        H.assert_train_slots(got, ref.slots, learner, what="%s %s" % (name, learner))
