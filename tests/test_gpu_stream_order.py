"""The stream contract (include/m2d.h, first convention): kernels are enqueued on the caller's stream, and what a call reads on the
host it reads after waiting for that stream.

Every case makes a non-default torch.cuda.Stream S current, enqueues a BLOCKER on it (torch.cuda._sleep, calibrated once to about
0.1 s) and behind the blocker device-to-device copies that overwrite the call's inputs with the REAL request; until the copies land
the inputs hold a DECOY, another valid request of the same shapes (stream_cases.py; tests/test_stream_cases_cpu.py asserts that the
decoy's answer differs in at least 0.9 of the lists or scores).  The call is made under torch.cuda.stream(S) while the blocker runs
-- asserted: the call is entered within half the blocker's duration --, then S.synchronize() and eng.check().  The result must equal,
bit for bit, a TWIN engine's for the real request on the default stream with everything synchronised; the twin's answer is held to
the float64 restatement once, so "equal to the twin" means "equal to the reference".  A stage that ran off S, or a host read that
did not wait for S, sees the decoy and changes the answer or raises the wrong error.

The writers add with float atomics -- "order-dependent in the last bits" (csrc/m2d_train.hip) --, so two runs of one train_step
need not agree bit for bit: its tables are held to the float64 restatement by the family's own comparison on BOTH engines instead.
(The write_memory row writes one pair per user -- one add per row, which no order can change -- and is compared bit for bit.)  The
readers that follow a writer are compared with a fresh engine built from the written tables.

No host-controlled spin flags, nothing that can hang: the blocker ends by itself.
"""
import time
import types

import numpy as np
import pytest

import stream_cases as st
from helpers import assert_scores_close, assert_scores_match_nonfinite, assert_train_tables

pytestmark = pytest.mark.gpu

TARGET_S = 0.1


# ---- the blocker -----------------------------------------------------------------------------------------------------------------
def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


@pytest.fixture(scope="module")
def blocker():
    """enqueue(): about TARGET_S of work on the current stream that reads and writes nothing of the tests'.  Calibrated in two fixed
    steps with a pair of events around the blocker alone; under 20 ms the module fails -- it does not pass, and it does not loop."""
    import torch
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        if hasattr(torch.cuda, "_sleep"):
            unit = lambda n: torch.cuda._sleep(int(n))
            n = 1_000_000
        else:
            x = torch.randn(4096, 4096, device="cuda")
            unit = lambda n: [torch.mm(x, x) for _ in range(int(n))]
            n = 4
        unit(n)                                              # (first launch: module load)
        for _ in range(2):
            n = max(1, int(n * TARGET_S / max(_timed(lambda: unit(n)), 1e-6)))
        seconds = _timed(lambda: unit(n))
    if seconds < 0.02:
        pytest.fail("the blocker calibrated to %.1f ms: too short to prove that a call was made before its inputs arrived" % (seconds * 1e3))
    return types.SimpleNamespace(enqueue=lambda: unit(n), seconds=seconds, stream=S)


# ---- engines and tensors ----------------------------------------------------------------------------------------------------------
def _dev(d):
    import torch
    return {k: torch.as_tensor(np.array(a), device="cuda") for k, a in d.items()}      # (np.array: the cases are read-only)


def _engine(E, kind, tabs=None, options=None, prepare=None):
    from foodrec_amd import ScoringEngine
    m = st.model(E, kind)
    eng = ScoringEngine(*(st.tables(E) if tabs is None else tabs), coef=m.coef)
    eng.set_dish_categories(m.cats)
    if m.head is not None:
        eng.set_mlp_head(*m.head)
    if m.ing is not None:
        eng.set_ingredients(*m.ing)
    if kind == "market":
        eng.set_recipes(*st.recipes(), st.R_INGREDIENTS)
    for name, value in (options or {}).items():
        eng.set_option(name, value)
    if prepare is not None:
        prepare(eng)
    eng.check()
    return eng


def _row_engine(r):
    return _engine(r.E, r.kind, options=r.options, prepare=r.prepare)


def _host(out):
    return tuple(x.detach().cpu().numpy().copy() for x in (out if isinstance(out, (tuple, list)) else (out,)))


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for n, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, n, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), "%s: output %d differs at %d of %d" % (what, n, int((_bits(x) != _bits(y)).sum()), x.size)


def _late(blocker, bufs, real, fn, check=None, host=None):
    """On S: the blocker, the late copies real -> bufs, then fn() -- entered while the blocker runs.  Returns fn()'s outputs on the
    host after S.synchronize() and check() (default: none), and whether the stream was still busy when fn() returned."""
    import torch
    S = blocker.stream
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        t0 = time.perf_counter()
        blocker.enqueue()
        for k in bufs:
            bufs[k].copy_(real[k], non_blocking=True)
        arrived = torch.cuda.Event()
        arrived.record(S)
        blocker.arrived = arrived
        waited = time.perf_counter() - t0
        assert waited < blocker.seconds / 2, "the call would be entered %.1f ms after the blocker (%.1f ms) was enqueued" % (
            waited * 1e3, blocker.seconds * 1e3)
        out = fn()
        busy = not arrived.query()
        S.synchronize()
        if check is not None:
            check()
    return (host or _host)(out), busy


def _twin_answer(r, real):
    """The twin's outputs for the real request on the default stream, everything synchronised -- held to the float64 restatement."""
    import torch
    twin = _row_engine(r)
    want = _host(r.call(twin, _dev(real)))
    twin.check()
    torch.cuda.synchronize()
    _assert_right(r, real, want, "twin")
    twin.close()
    return want


def _assert_list(s64, among, ids, scores, what):
    """One list against the float64 row over the dishes it was ranked among: topk_mlp_cases.compare_lists, the comparison of the
    retrieval tests under the head -- position by position the scores within TOL of the reference's sorted scores, every listed id
    a candidate no further than 2 TOL below the k-th, no increase, equal scores in ascending id, and the reference's very ids where
    its first k + 1 scores are more than 2 TOL apart.  A list with fewer candidates than columns ends in -1 / NaN."""
    import topk_mlp_cases as tm
    among = np.asarray(among, np.int64)
    n = min(len(ids), len(among))
    assert (ids[n:] == -1).all() and np.isnan(scores[n:]).all(), what
    if n:
        tm.compare_lists(scores[None, :n], ids[None, :n], s64[among][None, :], n, ids=[among], what=what)


def _assert_right(r, real, out, what, m=None, ans=None):
    """The outputs of row r's call against the float64 restatement of the real request (stream_cases.answers); m, ans: another
    restatement (a stream_cases.Model of other tables) and its answer to `real` (test_gpu_readers_after_writers_all.py)."""
    import seen_dish_cases as sd
    what = "%s (%s)" % (r.name, what)
    ans = st.answers(r.name)[0] if ans is None else ans
    m = st.model(r.E, r.kind) if m is None else m
    if r.name.startswith("train_step"):
        assert_train_tables(out[1:], st.trained_tables(m, real), (m.PM, m.RE, m.CE), st.TRAIN[0], visible=(), what=what)
        assert np.isfinite(out[0]).all()
    elif r.options.get("pm_bf16"):                           # the graph on the rounded table (include/m2d.h, "Serving mirror")
        import torch
        rounded = torch.from_numpy(np.ascontiguousarray(m.PM)).to(torch.bfloat16).to(torch.float32).numpy()
        assert_scores_close(out[0], m.pairs(real["users"], real["items"], real["cats"], PM=rounded), what=what)
    elif ans.what in ("scores", "rows"):
        assert_scores_close(out[0].reshape(-1), ans.value.reshape(-1), what=what)
    elif ans.what == "ranks":
        excl = st.rank_exclusions(real, st.FIXED_EXCL)
        for q in range(len(ans.value)):
            p = int(real["held"][q])
            s64 = ans.S[q].copy()
            s64[np.setdiff1d(excl[q], [p])] = -np.inf        # an excluded dish precedes nothing
            if r.kind != "mlp":
                sd.assert_rank_band(s64, p, int(out[0][q]), out[1][q])
                continue
            # under the head the scores are held to TOL (topk_mlp_cases.bound), not to assert_rank_band's 1e-5: the same band at TOL
            t = st.TOL * max(1.0, abs(s64[p]))
            others = np.arange(st.I) != p
            lo, hi = int(((s64 > s64[p] + t) & others).sum()), int(((s64 >= s64[p] - t) & others).sum())
            assert lo <= out[0][q] <= hi and abs(float(out[1][q]) - s64[p]) <= t, (what, q, lo, int(out[0][q]), hi)
    elif ans.S is None:                                      # cookable_dishes: the list itself
        assert np.array_equal(out[0], ans.value[0]), what
    else:
        scores, ids = out[0], out[1]
        for j in range(len(ids)):
            _assert_list(ans.S[j], ans.among[j], ids[j], scores[j], "%s row %d" % (what, j))
        if r.name.startswith("topk_markets") and len(out) == 3:
            assert np.array_equal(out[2], [len(a) for a in ans.among]), what


# ---- 1. late device inputs, first use ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in st.ROWS])
def test_late_inputs_first_use(name, blocker):
    """The side-stream call is the engine's first of its kind: every lazy build it needs is queued on S behind the blocker.  A first
    build may wait for S, and what the call launches after that wait finds its inputs arrived whatever stream it is on -- so the
    readers run a second episode on the same engine, now warmed: the inputs hold the decoy again, the real request arrives late
    again, and no build stands between the call and its launches.  (Not the writers: a second write starts from other tables.)"""
    r = st.BY_NAME[name]
    real, decoy = st.request(name)
    want = _twin_answer(r, real)
    eng = _row_engine(r)
    bufs, src = _dev(decoy), _dev(real)
    got, _ = _late(blocker, bufs, src, lambda: r.call(eng, bufs), eng.check)
    if r.exact:
        _assert_same(got, want, name)
    else:
        _assert_right(r, real, got, "side stream")
    if not set(r.covers) & {"write_memory", "train_step"}:
        for k, v in _dev(decoy).items():
            bufs[k].copy_(v)
        got, _ = _late(blocker, bufs, src, lambda: r.call(eng, bufs), eng.check)
        _assert_same(got, want, name + ", warmed")
    eng.close()


# ---- 6. "never synchronises" -----------------------------------------------------------------------------------------------------------
NEVER_SYNCHRONISES = ["score_pairs-E64", "score_pairs-E200", "score_pairs_bydish-E64", "score_pairs_ingredients", "score_pairs_mlp-form0-E64",
                      "score_pairs_mlp-form1-E64", "topk_markets"]


@pytest.mark.parametrize("name", NEVER_SYNCHRONISES)
def test_warmed_call_returns_before_its_inputs_arrive(name, blocker):
    """m2d.h promises in words that these calls do not synchronise (the pair-scoring calls by the general rule, m2d_topk_markets
    after the first call of a size): on a warmed engine the event recorded behind the late copies has not completed when the call
    returns -- which is also the proof that the inputs had not arrived when the call was made."""
    r = st.BY_NAME[name]
    real, decoy = st.request(name)
    want = _twin_answer(r, real)
    eng = _row_engine(r)
    bufs, src = _dev(decoy), _dev(real)
    r.call(eng, bufs)                                        # warm: the decoy, default stream
    eng.check()
    got, busy = _late(blocker, bufs, src, lambda: r.call(eng, bufs), eng.check)
    assert busy, "%s returned after the late copies had completed: the call synchronised" % name
    _assert_same(got, want, name)
    eng.close()


# ---- 4. late errors --------------------------------------------------------------------------------------------------------------------
def _position(d, key):
    """Where a bad id may stand in input `key` without breaking another rule: the end of an exclusion segment or of the slate (the
    lists stay ascending), a group's first slot (never padding), anywhere else position 77 or the middle."""
    if key == "excl_ids":
        off = d["excl_off"]
        j = int(np.flatnonzero(np.diff(off) > 1)[3])
        return int(off[j + 1] - 1)
    if key == "slate":
        return d[key].size - 1
    if key == "members":
        return 6 * d[key].shape[1]
    return min(77, d[key].size // 2)


@pytest.mark.parametrize("name", list(st.ERRORS))
def test_late_errors(name, blocker):
    """The decoy carries a bad user id and the real request is clean: check() raises nothing and the answer is the twin's.  Then the
    real request carries a bad id at another position and the decoy is clean: check() names that position and its value."""
    r = st.BY_NAME[name]
    real, decoy = st.request(name)
    user_key, item_key = st.ERRORS[name]
    p = _position(decoy, user_key) + (1 if user_key != "members" else decoy[user_key].shape[1])
    want = _twin_answer(r, real)
    eng = _row_engine(r)
    bufs, src = _dev(st.with_bad_id(decoy, user_key, p, st.BAD_USER)), _dev(real)
    got, _ = _late(blocker, bufs, src, lambda: r.call(eng, bufs), eng.check)
    if r.exact:
        _assert_same(got, want, name + ", bad id in the decoy")
    else:
        _assert_right(r, real, got, "bad id in the decoy")
    eng.close()

    key, value, word = (item_key, st.BAD_ITEM, "item") if item_key is not None else (user_key, st.BAD_USER, "user")
    q = _position(real, key)
    assert q != p or key != user_key
    eng = _row_engine(r)
    bufs, src = _dev(decoy), _dev(st.with_bad_id(real, key, q, value))
    with pytest.raises(IndexError, match=r"%s id %d at position %d " % (word, value, q)):
        _late(blocker, bufs, src, lambda: r.call(eng, bufs), eng.check)
    blocker.stream.synchronize()
    eng.close()


def test_late_list_that_is_not_ascending(blocker):
    """topk_users_excluding: the real request's exclusion list has an id below its predecessor; the decoy's lists are in order."""
    name = "topk_users_excluding-E64"
    r = st.BY_NAME[name]
    real, decoy = st.request(name)
    off = real["excl_off"]
    j = int(np.flatnonzero(np.diff(off) > 2)[5])
    q = int(off[j] + 1)
    ids = real["excl_ids"].copy()
    ids[q - 1], ids[q] = ids[q], ids[q - 1]
    bad = dict(real, excl_ids=ids)
    eng = _row_engine(r)
    bufs, src = _dev(decoy), _dev(bad)
    with pytest.raises(ValueError, match=r"not ascending: value %d at position %d " % (ids[q], q)):
        _late(blocker, bufs, src, lambda: r.call(eng, bufs), eng.check)
    blocker.stream.synchronize()
    eng.close()


# ---- the readers of test_gpu_readers_after_writers._snapshot, on resident inputs and without a check() between them -------------------
DEFAULTS = {"topk_bf16x3": 1, "variant": 0, "topk_excl_tier": 0, "user_high_table": 0, "mlp_form": 0, "topk_grouped": 1, "mlp_bf16x3": 1}


def _reader_inputs():
    import torch
    from test_gpu_readers_after_writers import _inputs
    inp = _inputs()
    t = lambda a: torch.as_tensor(np.array(a), device="cuda")
    cats = t(st.model(64, "plain").cats)
    d = dict(users=t(inp.users), items=t(inp.items), big_users=t(inp.big_users), big_items=t(inp.big_items), held=t(inp.held),
             all_users=torch.arange(st.U, dtype=torch.int32, device="cuda"))
    d["cats"], d["big_cats"] = cats[d["items"].long()].contiguous(), cats[d["big_items"].long()].contiguous()
    for name in ("excl_some", "excl_most", "excl_none"):
        d[name] = tuple(t(x) for x in getattr(inp, name))
    d["excl_some_host"] = inp.excl_some
    torch.cuda.synchronize()
    return d


def _readers(kind):
    """(name, options, call) in _snapshot's order; catalogue_rank last: it sorts its lists on the host, which waits for the stream."""
    topk = lambda eng, t: eng.topk_users(t["all_users"], st.K)
    pairs = lambda eng, t: eng.score_pairs(t["users"], t["items"], t["cats"])
    if kind == "ing":
        return [("ingredient_pairs", {}, lambda eng, t: eng.score_pairs_ingredients(t["users"], t["items"])),
                ("topk", {}, topk), ("topk_dense", {"topk_grouped": 0}, topk)]
    if kind == "mlp":
        mlp = lambda eng, t: eng.score_pairs_mlp(t["users"], t["items"])
        return [("topk", {}, topk), ("pairs", {}, pairs), ("mlp_form0", {"mlp_form": 0}, mlp), ("mlp_form1", {"mlp_form": 1}, mlp),
                ("mlp_big", {}, lambda eng, t: eng.score_pairs_mlp(t["big_users"], t["big_items"]))]
    excl = lambda which: (lambda eng, t: eng.topk_users_excluding(t["all_users"], st.K, t[which]))
    return [("topk", {}, topk), ("pairs", {}, pairs), ("topk_f32", {"topk_bf16x3": 0}, topk), ("topk_dense", {"variant": 7}, topk),
            ("excl_most", {}, excl("excl_most")), ("excl_none", {}, excl("excl_none")), ("excl_tier2", {"topk_excl_tier": 2}, excl("excl_some")),
            ("bydish", {}, lambda eng, t: eng.score_pairs_bydish(t["users"], t["items"])),
            ("pairs_uh", {"user_high_table": 1}, lambda eng, t: eng.score_pairs(t["big_users"], t["big_items"], t["big_cats"])),
            ("rank", {}, lambda eng, t: eng.catalogue_rank(t["all_users"], t["held"], t["excl_some_host"]))]


def _options(eng, options, reset=False):
    for name, value in options.items():
        eng.set_option(name, DEFAULTS[name] if reset else value)


def _read_all(eng, kind, t, check=True):
    """Every reader by name -> device outputs; check=True: with a check() after each (the twin's way, and the warm-up)."""
    out = {}
    for name, options, call in _readers(kind):
        _options(eng, options)
        out[name] = call(eng, t)
        if check:
            eng.check()
        _options(eng, options, reset=True)
    return out


def _fresh_answers(E, kind, tabs, t):
    """Every reader on a fresh default-stream engine built from `tabs`, on the host; pairs and lists held to the float64 restatement."""
    import torch
    eng = _engine(E, kind, tabs=tabs)
    out = {name: _host(x) for name, x in _read_all(eng, kind, t).items()}
    torch.cuda.synchronize()
    eng.close()
    return out


def _assert_readers_right(E, kind, tabs, answers, t):
    m = st.Model(E, kind, tabs=tuple(np.asarray(x) for x in tabs))
    users, items = t["users"].cpu().numpy(), t["items"].cpu().numpy()
    if "pairs" in answers:
        assert_scores_close(answers["pairs"][0], m.pairs(users, items, head=False), what="twin, pairs")
    if "mlp_form0" in answers:
        for form in ("mlp_form0", "mlp_form1"):
            assert_scores_close(answers[form][0], m.pairs(users, items), what="twin, " + form)
    if "ingredient_pairs" in answers:
        assert_scores_close(answers["ingredient_pairs"][0], m.pairs(users, items), what="twin, ingredient pairs")
    else:
        sample = np.arange(0, st.U, 37)
        S = m.rows(sample, head=False)
        for j, u in enumerate(sample):
            _assert_list(S[j], np.arange(st.I), answers["topk"][1][u], answers["topk"][0][u], "twin, topk of user %d" % u)


# ---- 2. late tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,E", [("plain", 64), ("mlp", 64), ("ing", 64), ("plain", 200)])
def test_late_tables(kind, E, blocker):
    """The engine borrows eng.pm / eng.re / eng.ce.  On an engine WARMED on one set of tables -- every derived table built -- the other
    set is copied in on S behind the blocker, tables_updated() is called and one reader runs on S: every derived table it needs is
    rebuilt on S, behind the copies.  The answer is a fresh default-stream engine's on the new tables.  One episode per reader, the
    tables going back and forth."""
    import torch
    t = _reader_inputs()
    sets = [st.tables(E, 0), st.tables(E, 1)]
    want = [_fresh_answers(E, kind, tabs, t) for tabs in sets]
    for tabs, answers in zip(sets, want):
        _assert_readers_right(E, kind, tabs, answers, t)
    dev = [[torch.as_tensor(x, device="cuda") for x in tabs] for tabs in sets]
    eng = _engine(E, kind, tabs=sets[0])
    cur = 0
    for name, options, call in _readers(kind):
        _read_all(eng, kind, t)                              # warm on the tables as they stand
        nxt = 1 - cur
        _options(eng, options)
        live = {"pm": eng.pm, "re": eng.re, "ce": eng.ce}

        def late_call():
            eng.tables_updated()
            return call(eng, t)
        got, _ = _late(blocker, live, dict(zip(("pm", "re", "ce"), dev[nxt])), late_call, eng.check)
        _options(eng, options, reset=True)
        _assert_same(got, want[nxt][name], "%s after late tables (set %d)" % (name, nxt))
        cur = nxt
    eng.close()


def test_late_tables_with_an_inf(blocker):
    """The second Personal_Memory carries one inf: the finite scan runs on S behind the copies and the retrieval launcher's host copy
    of the "not finite" word must follow it -- the lists are the literal kernel's, the graph's order."""
    import torch
    E, kind = 64, "plain"
    t = _reader_inputs()
    second = [x.copy() for x in st.tables(E, 1)]
    second[0][5, 2, 3] = np.inf
    fresh = _engine(E, kind, tabs=second)
    want = _host(fresh.topk_users(t["all_users"], st.K))
    fresh.check()
    assert fresh.last_kernel() == "m2d_topk_literal"
    want_pairs = _host(fresh.score_pairs(t["users"], t["items"], t["cats"]))
    fresh.check()
    fresh.close()
    assert np.isfinite(want[0]).mean() > 0.9 and not np.isfinite(want[0][5]).all()      # user 5's list shows the inf; the others are plain
    # the fresh engine's answer is the graph's: test_gpu_nonfinite's comparison against oracle.topk_catalogue on the poisoned tables
    # for user 5 and a sample of the others, the pairs against inference_f64 with the same NaN and the same infinities
    from oracle import m2d_oracle as oracle
    from test_gpu_nonfinite import _assert_list_is_the_graphs
    cats = st.model(E, kind).cats
    sample = np.unique(np.concatenate([[5], np.arange(0, st.U, 23)]))
    ref_s, ref_i = oracle.topk_catalogue(*second, cats, sample, st.K)
    assert np.isposinf(ref_s[list(sample).index(5)]).any()
    for j, u in enumerate(sample):
        with np.errstate(invalid="ignore"):
            ref = oracle.inference_f64(*second, np.full(st.I, u), np.arange(st.I), cats)
        _assert_list_is_the_graphs(want[0][u], want[1][u], ref, ref_s[j], ref_i[j], "fresh engine, inf in Personal_Memory, user %d" % u)
    with np.errstate(invalid="ignore"):
        ref = oracle.inference_f64(*second, t["users"].cpu().numpy(), t["items"].cpu().numpy(), t["cats"].cpu().numpy())
    assert not np.isfinite(ref).all()
    assert_scores_match_nonfinite(want_pairs[0], ref, what="fresh engine, inf in Personal_Memory, pairs")
    dev =[torch.as_tensor(x, device="cuda") for x in second]
    for reader in ("topk", "pairs"):
        eng = _engine(E, kind)
        _read_all(eng, kind, t)
        live = {"pm": eng.pm, "re": eng.re, "ce": eng.ce}

        def late_call():
            eng.tables_updated()
            if reader == "topk":
                return eng.topk_users(t["all_users"], st.K)
            return eng.score_pairs(t["users"], t["items"], t["cats"])
        got, _ = _late(blocker, live, dict(zip(("pm", "re", "ce"), dev)), late_call, eng.check)
        if reader == "topk":
            assert eng.last_kernel() == "m2d_topk_literal"
        _assert_same(got, want if reader == "topk" else want_pairs, reader + " after late tables with an inf")
        eng.close()


# ---- 3. writers then readers on S, nothing between ---------------------------------------------------------------------------------
@pytest.mark.parametrize("writer", ["write_memory", "train_step-B128", "train_step-B1100"])
@pytest.mark.parametrize("kind", ["plain", "mlp"])
def test_writer_then_readers_without_synchronising(writer, kind, blocker):
    """On S behind the blocker: the writer on its late request, then every reader, with no synchronisation and no check() between
    them; one S.synchronize() at the end.  The written tables are held to the float64 restatement (the writers' sums are float
    atomics: a twin's tables need not have the same last bits), and every reader's answer is a fresh default-stream engine's on the
    tables the writer left -- a reader that ran before the writer, or off S, read other tables."""
    r = st.BY_NAME[writer]
    real, decoy = st.request(writer)
    t = _reader_inputs()
    eng = _engine(r.E, kind, prepare=r.prepare)
    _read_all(eng, kind, t)                                  # warm: every derived table is built from the tables before the write
    bufs, src = _dev(decoy), _dev(real)
    out = {}

    def chain():
        written = r.call(eng, bufs)
        out.update(_read_all(eng, kind, t, check=False))
        return written
    written, _ = _late(blocker, bufs, src, chain, eng.check)
    m = st.model(r.E, kind)
    if writer == "write_memory":
        assert_scores_close(written[0].reshape(-1), st.written_tables(m, real).reshape(-1), what="write_memory on S")
    else:
        assert_train_tables(written[1:], st.trained_tables(m, real), (m.PM, m.RE, m.CE), st.TRAIN[0], visible=(), what=writer + " on S")
    tabs = tuple(x.cpu().numpy().copy() for x in (eng.pm, eng.re, eng.ce))
    want = _fresh_answers(r.E, kind, tabs, t)
    _assert_readers_right(r.E, kind, tabs, want, t)
    for name in want:
        _assert_same(_host(out[name]), want[name], "%s after %s on S" % (name, writer))
    eng.close()


# ---- 5. a chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "mlp"])
def test_chain_of_calls_behind_one_blocker(kind, blocker):
    """topk_users, rank_candidates at L = 1024, score_pairs on the big batch, topk_users_excluding, topk_slate, topk_users with three
    times the users (scratch grows in the middle of the chain) and score_pairs_mlp, on S behind ONE blocker with no synchronisation
    and no check() between them: each output equals its solo default-stream answer from the twin.  topk_users_excluding and
    topk_slate refuse an engine with a head and score_pairs_mlp needs one, so the chain runs twice: without a head less its last
    step, with a head less those two.  The engine is warmed on the decoys (tables built, scratch at the size of every step but the
    tripled one), so no call before the growth waits for the stream -- asserted by an event query, as in the "never synchronises"
    cases -- and a launch moved off S reads the decoy or races the scratch of the call before it."""
    E = 64
    steps = st.CHAINS[kind]                                  # rows like any other: the CPU test holds each step's decoy to the 0.9 condition
    requests = [st.request(r.name) for r in steps]
    twin = _engine(E, kind)
    want = []
    for r, (real, _) in zip(steps, requests):
        want.append(_host(r.call(twin, _dev(real))))
        twin.check()
        _assert_right(r, real, want[-1], "twin")             # each step's solo answer against the float64 restatement
    twin.close()
    eng = _engine(E, kind)
    bufs = [_dev(decoy) for _, decoy in requests]
    srcs = [_dev(real) for real, _ in requests]
    flat = lambda ds: {(n, k): v for n, d in enumerate(ds) for k, v in d.items()}
    # warmed on the decoys, the tripled topk_users apart: the derived tables are built and the scratch has the size of every other
    # step (a first build and a first call of a size may wait for the stream -- hipFree does), so the chain's first wait is the
    # growth in its middle and every call before it is made while the blocker still runs
    grows = [r.name.endswith("topk_users_tripled") for r in steps].index(True)
    for n, r in enumerate(steps):
        if n != grows:
            r.call(eng, bufs[n])
            eng.check()
    late = {}

    def chain():
        outs = []
        for n, (r, b) in enumerate(zip(steps, bufs)):
            if n == grows:
                late["before the growth"] = not blocker.arrived.query()
            outs.append(r.call(eng, b))
        return outs
    got, _ = _late(blocker, flat(bufs), flat(srcs), chain, eng.check, host=lambda outs: [_host(o) for o in outs])
    assert late["before the growth"], "a call before the growth waited for the stream: the calls after it were not made before their inputs arrived"
    for r, g, w in zip(steps, got, want):
        _assert_same(g, w, r.name)
    eng.close()
