"""Readers after writers, the whole matrix: EVERY reader call of the engine after EVERY call that writes what the readers see
(writer_cases.py: one reader table -- stream_cases.ROWS' readers and the menu family's four engine calls --, one writer table).
test_gpu_readers_after_writers.py states the pattern and holds the first ten readers to it with the kernel each is there for; a
reader added to the engine joins the matrix HERE, through stream_cases.ROWS or a row of writer_cases (tests/test_writer_cases_cpu.py
fails until it does).

One test per (engine kind, writer):

    snapshot (every reader of the kind: this warms every cache) -> the writer's step, check() -> snapshot -> the same snapshot on a
    FRESH engine built from the written engine's own tables and masks, the head and the recipes it was given

  * the written engine equals the fresh one bit for bit, reader by reader: ids as integers, scores as 32-bit words;
  * the fresh engine's answers are right against the float64 restatement on those tables, a sample of rows per reader
    (writer_cases.sample_rows); the menu rows against their features' restatements over the fresh engine's own score words;
  * each reader changed (beyond _assert_changed's thresholds), stayed bit-equal, or refuses on both engines with a ValueError that
    names the call -- as writer_cases.expected says from the restatement alone.

A writer of several steps is read after every step.  Then: set_ingredients on a warmed engine and clear_ingredients again; the menu
family once more with launches cut into ranges and user blocks; and on a side stream behind a blocker the late tables and the
writers, each followed by every reader of the kind with no synchronisation and no check() between them.
"""
import numpy as np
import pytest

import deep_cases as dc
import stream_cases as st
import test_gpu_stream_order as so
import writer_cases as wc
from helpers import assert_scores_close, assert_train_tables
from test_gpu_stream_order import _dev, _host, _late, blocker  # noqa: F401  (blocker: the module's calibrated fixture)

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = dict(so.DEFAULTS, pm_bf16=0, deep_chunk_pairs=1 << 22)
# calls that wait for the stream by design go last in a chain on a side stream: the host-array call, cookable_dishes' count (and the
# market call built on it), catalogue_rank(head=False)'s host-sorted lists, and the menu family -- the first call after a write to
# the masks builds the signature index, a call with a slate reads the slate's segment sizes
WAITS = ("score_pairs_host", "cookable_dishes", "topk_market", "catalogue_rank", "_topk_menu", "_plan_menus", "_plan_groups",
         "_topk_menu_filtered")


# ---- engines, requests, snapshots -------------------------------------------------------------------------------------------------
def _engine(s, prepare=None):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(*s.tabs, coef=s.coef, user_base=s.user_base)
    eng.set_dish_categories(s.cats)
    if s.skind == "mlp":
        eng.set_mlp_head(*s.head)
    if s.ing is not None:
        eng.set_ingredients(*s.ing)
    if s.skind == "market":
        eng.set_recipes(*s.recipes, st.R_INGREDIENTS)
    if prepare is not None:
        prepare(eng)
    eng.check()
    assert all(eng.get_option(k) == v for k, v in OPTION_DEFAULTS.items()), {k: eng.get_option(k) for k in OPTION_DEFAULTS}
    return eng


def _state_of(eng, s):
    """the state a fresh engine is built from: the written engine's OWN tables and masks, the head and recipes it was given"""
    cats = eng.dish_cats.cpu().numpy().copy()
    assert np.array_equal(cats, s.cats)
    return wc._with(s, tabs=tuple(x.cpu().numpy().copy() for x in (eng.pm, eng.re, eng.ce)), cats=cats)


_REQUESTS = {}


def _requests(kind, user_base):
    """reader -> its request as device tensors (and as numpy arrays under "_host"), resident for the whole module"""
    import torch
    key = (kind, user_base)
    if key not in _REQUESTS:
        out = {}
        for r in wc.readers_of(kind):
            d = wc.shifted(wc.request(r.name), user_base)
            out[r.name] = dict(_dev(d), _host=d)
        torch.cuda.synchronize()
        _REQUESTS[key] = out
    return _REQUESTS[key]


def _ordered(kind, names=None):
    rows = [r for r in wc.readers_of(kind) if names is None or r.name in names]
    return [r for r in rows if r.name not in WAITS] + [r for r in rows if r.name in WAITS]


def _call(r, eng, t, options=None):
    """the reader's call under its options (reset behind it) -> device outputs"""
    import torch
    options = dict(r.options, **(options or {}))
    for name, value in options.items():
        eng.set_option(name, value)
    try:
        out = r.call(eng, t)
    finally:
        for name in options:
            eng.set_option(name, OPTION_DEFAULTS[name])
    return tuple(torch.from_numpy(x) if isinstance(x, np.ndarray) else x for x in (out if isinstance(out, (tuple, list)) else (out,)))


def _snapshot(eng, kind, s, names=None, options=None):
    """reader -> its outputs on the host, or the ValueError it refused with; a check() after every call"""
    t = _requests(kind, s.user_base)
    out = {}
    for r in _ordered(kind, names):
        try:
            res = _call(r, eng, t[r.name], options)
            eng.check()
        except ValueError as e:
            out[r.name] = e
            continue
        out[r.name] = _host(res)
    return out


def _refused(x):
    return isinstance(x, ValueError)


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        if _refused(a[name]) or _refused(b[name]):
            assert _refused(a[name]) and _refused(b[name]) and str(a[name]) == str(b[name]), (what, name, a[name], b[name])
        else:
            so._assert_same(a[name], b[name], "%s: %s" % (what, name))


def _take(out, idx, n):
    return out if idx is None else tuple(x[idx] if x.ndim and x.shape[0] == n else x for x in out)


def _assert_oracle(eng, snap, kind, s, what):
    """The snapshot of engine `eng` (state s: its own tables) against the float64 restatement, a sample of rows per reader; the menu
    rows against their restatement over the engine's own score words."""
    import torch
    m = wc.model_of(s)
    every_dish = torch.arange(wc.I, dtype=torch.int32, device="cuda")
    for r in wc.readers_of(kind):
        if _refused(snap[r.name]):
            continue
        d = wc.request(r.name)
        idx = wc.sample_rows(r, d, oracle=True)
        sub = wc.asked(r, d if idx is None else wc.subrequest(d, idx), s.cats)
        out = _take(snap[r.name], idx, wc.n_rows(d))
        if r.name in wc.MENU_CALLS:
            users = np.arange(wc.U, dtype=np.int32) if "members" in sub else sub["users"]
            W = eng.score_slate(torch.as_tensor(users + s.user_base, device="cuda"), every_dish)
            eng.check()
            words, ids = r.restate(W.cpu().numpy(), s.cats, sub)
            assert np.array_equal(out[1].astype(np.int64), ids), "%s: %s: ids of %d rows differ" % (
                what, r.name, int((out[1] != ids).reshape(len(ids), -1).any(1).sum()))
            assert np.array_equal(dc.words(out[0]), words), "%s: %s: score words differ" % (what, r.name)
            assert (ids.reshape(len(ids), -1)[:, 0] >= 0).all(), (what, r.name)       # no list is empty: the caps bind, they do not close
        else:
            so._assert_right(r, sub, out, what, m=m, ans=r.answer(m, sub))


def _main(r, out, what):
    """the output that `what` is said of: the ids of a list, the ranks, the scores"""
    if r.name == "cookable_dishes":
        return out[0][None, :]
    return out[1] if what == "lists" else out[0]


def _assert_expected(kind, writer, n, before, after, fresh, what):
    for r in wc.readers_of(kind):
        want, share = wc.expected(kind, writer, n, r.name)
        b, a = before[r.name], after[r.name]
        where = "%s: %s (%s)" % (what, r.name, want)
        if want == "refuses":
            assert _refused(a) and _refused(fresh[r.name]) and "m2d_" + r.covers[0] in str(a), (where, a)
            continue
        assert not _refused(a), (where, a)
        if _refused(b):                                      # it refused before the step: any answer is a change
            continue
        ans_what = wc.restated(kind, writer, n + 1, r.name).what
        if want == "same":
            for x, y in zip(b, a):
                assert wc.judge(ans_what, x, y, "same") is None, where
        else:
            kind_of = wc.measure(r, ans_what)
            why = wc.judge(kind_of, _main(r, b, ans_what), _main(r, a, ans_what), "changed")
            assert why is None, "%s %s" % (where, why)


# ---- 1. the matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,writer", wc.PAIRS)
def test_every_reader_after(kind, writer):
    import torch
    w = wc.WRITER_BY_NAME[writer]
    chain = wc.states(kind, writer)
    eng = _engine(chain[0])
    before = _snapshot(eng, kind, chain[0])
    for n, step in enumerate(w.steps):
        what = "%s, %s" % (kind, step.name)
        step.apply(eng, chain[n])
        eng.check()
        s = _state_of(eng, chain[n + 1])
        after = _snapshot(eng, kind, s)
        fresh_eng = _engine(s)
        fresh = _snapshot(fresh_eng, kind, s)
        _assert_same(after, fresh, what + ": written engine vs fresh engine")
        _assert_oracle(fresh_eng, fresh, kind, s, what + ": fresh engine")
        fresh_eng.close()
        _assert_expected(kind, writer, n, before, after, fresh, what)
        before = after
    if writer == "set_user_base":                            # an id of the range before is refused, with its value and position
        eng.topk_users(torch.arange(3, dtype=torch.int32, device="cuda"), wc.K)
        with pytest.raises(IndexError, match="user id [012] at position [012] "):
            eng.check()
    if getattr(eng, "_training", False):
        eng.train_end()
    eng.close()


def test_the_oracles_batches_are_the_engines():
    """writer_cases.write_batch / train_batch are test_gpu_readers_after_writers._write_batch / _train_batch array for array"""
    from test_gpu_readers_after_writers import _train_batch, _write_batch
    s = wc._with(wc.initial("plain"), user_base=wc.USER_BASE)
    for seed in (5, 6):
        got = _write_batch(wc._cfg(s), seed=seed)
        want = wc.write_batch(s.E, s.cats, seed=seed)
        assert np.array_equal(got[0].cpu().numpy(), want[0] + wc.USER_BASE) and tuple(got[6:]) == (1.0, 1.0, 0.5)
        assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(got[1:6], want[1:]))
    for B, seed in ((256, 11), (256, 12), (1100, 11), (1100, 13)):
        got, want = _train_batch(wc._cfg(s), B, seed=seed), wc.train_batch(s.cats, B, seed=seed)
        assert np.array_equal(got[0].cpu().numpy(), want[0] + wc.USER_BASE)
        assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(got[1:], want[1:]))


# ---- 2. set_ingredients on a warmed engine, and clear_ingredients ---------------------------------------------------------------------
def test_ingredients_set_on_a_warmed_engine_and_cleared():
    """With the table set, every reader that m2d_deep_conditions, m2d_rank_prepare or its own entry guards refuses by name -- the
    slate, deep, group, ranking and menu calls at the least -- and every other reader answers as a fresh engine with that table does.
    clear_ingredients then brings back the snapshot from before bit for bit: the menu index, the slate scratch and the head-free
    images were all built before it and the sorted rows [H[d] | RE[d]] in between, and none of it may leak."""
    kind = "plain"
    s = wc.initial(kind)
    ing = wc._ingredients(s.E, 2)
    eng = _engine(s)
    before = _snapshot(eng, kind, s)
    assert not any(_refused(x) for x in before.values())
    eng.set_ingredients(*ing)
    during = _snapshot(eng, kind, s)
    fresh_eng = _engine(wc._with(s, ing=ing))
    fresh = _snapshot(fresh_eng, kind, s)
    fresh_eng.close()
    _assert_same(during, fresh, "set_ingredients on a warmed engine vs a fresh engine with the table")
    for r in wc.readers_of(kind):
        x = during[r.name]
        if r.covers[0] in wc.REFUSE_INGREDIENTS:
            assert _refused(x) and "m2d_" + r.covers[0].lstrip("_") in str(x), (r.name, x)
        if _refused(x):
            assert str(x).startswith("m2d_") and "ingredient" in str(x), (r.name, x)
        print("%s with the ingredient table: %s" % (r.name, x if _refused(x) else "answers"))
    assert not _refused(during["topk_users-E64"])
    assert wc.judge("lists", before["topk_users-E64"][1], during["topk_users-E64"][1], "changed") is None
    eng.clear_ingredients()
    after = _snapshot(eng, kind, s)
    _assert_same(after, before, "clear_ingredients: the snapshot from before the table was set")
    _assert_oracle(eng, after, kind, s, "clear_ingredients")
    eng.close()


# ---- 3. a reader's own launch decisions ----------------------------------------------------------------------------------------------
def test_menu_family_after_writers_with_launches_cut_into_ranges_and_user_blocks():
    """The menu calls once more, with "deep_chunk_pairs" = 256 and masks that put half the dishes into ONE signature: that segment
    of 1 500 dishes is cut into six ranges of 256 -- the running-list merge (first = 0) -- and the users into blocks of one.  The
    index, the segment sizes on the host and the scratch are those of a warmed engine after Write_Memory and set_dish_categories;
    the lists are a fresh engine's at the default cut, bit for bit, and the restatement's over its words."""
    kind = "plain"
    s0 = wc.initial(kind)
    cats = wc._masks(7).copy()
    cats[::2] = (1, 0, 1, 0)
    assert (np.bincount(wc.mc.signatures(cats), minlength=64) > 256).sum() == 1
    cut = {"deep_chunk_pairs": 256}
    eng = _engine(s0)
    before = _snapshot(eng, kind, s0, wc.MENU_CALLS)
    assert wc.judge("lists", before["_topk_menu"][1], _snapshot(eng, kind, s0, ("_topk_menu",), cut)["_topk_menu"][1], "same") is None
    step = wc.step_write(True, False)
    step.apply(eng, s0)
    eng.set_dish_categories(cats)
    eng.check()
    s = _state_of(eng, wc._with(step.after(s0), cats=cats))
    after = _snapshot(eng, kind, s, wc.MENU_CALLS, cut)
    fresh_eng = _engine(s)
    fresh = _snapshot(fresh_eng, kind, s, wc.MENU_CALLS)
    _assert_same(after, fresh, "cut launches on the written engine vs a fresh engine at the default cut")
    snap = dict({r.name: ValueError("not read") for r in wc.readers_of(kind)}, **fresh)
    _assert_oracle(fresh_eng, snap, kind, s, "fresh engine, skewed masks")
    fresh_eng.close()
    for name in wc.MENU_CALLS:
        why = wc.judge("lists", before[name][1], after[name][1], "changed")
        assert why is None, (name, why)
    eng.close()


# ---- 4. on a side stream ------------------------------------------------------------------------------------------------------------
def _chain_of_readers(eng, kind, t, out):
    """every reader of the kind, the waiting ones last, with no synchronisation and no check() between them"""
    for r in _ordered(kind):
        out[r.name] = _call(r, eng, t[r.name])


def _hosts(outs):
    return {name: _host(x) for name, x in outs.items()}


@pytest.mark.parametrize("kind", ["plain", "mlp", "market", "plain200", "mlp200", "ing"])
def test_late_tables_then_every_reader(kind, blocker):  # noqa: F811
    """ONE blocker episode per kind: every reader is warmed on table set 0 -- every derived table built --; on S behind the blocker
    table set 1 is copied in, tables_updated() is called and every reader of the kind runs, nothing between them.  Each answer is a
    fresh default-stream engine's on set 1, bit for bit (and that engine's answers are right, and not those on set 0)."""
    import torch
    s0 = wc.initial(kind)
    s1 = wc._with(s0, tabs=st.tables(s0.E, 1))
    t = _requests(kind, 0)
    fresh_eng = _engine(s1)
    want = _snapshot(fresh_eng, kind, s1)
    _assert_oracle(fresh_eng, want, kind, s1, "fresh engine on table set 1")
    fresh_eng.close()
    eng = _engine(s0)
    warm = _snapshot(eng, kind, s0)
    for r in wc.readers_of(kind):
        if r.name != "cookable_dishes":                      # (it reads the recipes, no table)
            assert not all(np.array_equal(x, y) for x, y in zip(warm[r.name], want[r.name])), r.name
    dev = [torch.as_tensor(x, device="cuda") for x in s1.tabs]
    live = {"pm": eng.pm, "re": eng.re, "ce": eng.ce}
    outs = {}

    def late_call():
        eng.tables_updated()
        _chain_of_readers(eng, kind, t, outs)
        return outs
    got, _ = _late(blocker, live, dict(zip(("pm", "re", "ce"), dev)), late_call, eng.check, host=_hosts)
    for name in want:
        so._assert_same(got[name], want[name], "%s after late tables" % name)
    eng.close()


@pytest.mark.parametrize("writer", ["write_memory", "train_step-B128", "train_step-B1100"])
@pytest.mark.parametrize("kind", ["plain", "mlp", "market"])
def test_writer_then_every_reader_without_synchronising(writer, kind, blocker):  # noqa: F811
    """test_gpu_stream_order.test_writer_then_readers_without_synchronising with every reader of the kind behind the writer: the
    written tables are right against the restatement, and every reader equals a fresh engine on the tables the writer left."""
    r = st.BY_NAME[writer]
    real, decoy = st.request(writer)
    s0 = wc.initial(kind)
    t = _requests(kind, 0)
    eng = _engine(s0, prepare=r.prepare)
    _snapshot(eng, kind, s0)                                 # warm: every derived table is built from the tables before the write
    bufs, src = _dev(decoy), _dev(real)
    outs = {}

    def chain():
        written = r.call(eng, bufs)
        _chain_of_readers(eng, kind, t, outs)
        return written
    written, _ = _late(blocker, bufs, src, chain, eng.check)
    m = st.model(r.E, s0.skind)
    if writer == "write_memory":
        assert_scores_close(written[0].reshape(-1), st.written_tables(m, real).reshape(-1), what="write_memory on S")
    else:
        assert_train_tables(written[1:], st.trained_tables(m, real), (m.PM, m.RE, m.CE), st.TRAIN[0], visible=(), what=writer + " on S")
    got = _hosts(outs)
    s = _state_of(eng, s0)
    if getattr(eng, "_training", False):
        eng.train_end()
    eng.close()
    fresh_eng = _engine(s)
    want = _snapshot(fresh_eng, kind, s)
    _assert_oracle(fresh_eng, want, kind, s, "fresh engine on the tables %s left" % writer)
    fresh_eng.close()
    for name in want:
        so._assert_same(got[name], want[name], "%s after %s on S" % (name, writer))
