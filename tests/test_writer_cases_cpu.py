"""The conditions that keep tests/test_gpu_readers_after_writers_all.py from passing on stale state, checked without a GPU
(writer_cases.py): every (reader, writer) pair is "same", "refuses", or "changed" clear of its threshold on the float64 restatement
alone; every public method of ScoringEngine is a reader or a writer of the matrix or excused with a reason; and the comparison the GPU
file makes fails a reader that answers from the tables before the writer, and one that follows a writer that must change nothing."""
import inspect

import numpy as np
import pytest

import stream_cases as st
import writer_cases as wc


@pytest.mark.parametrize("kind,writer", wc.PAIRS)
def test_every_pair_is_same_refuses_or_changed_clear_of_its_threshold(kind, writer):
    """... over a sample of at least 40 result rows per reader (all of them where the reader has fewer).  A "changed" pair within 0.05
    of its threshold is a weak writer: strengthen the writer, the thresholds stay."""
    steps = wc.WRITER_BY_NAME[writer].steps
    readers = wc.readers_of(kind)
    assert readers and steps
    seen = set()
    for n, step in enumerate(steps):
        for r in readers:
            d = wc.request(r.name)
            idx = wc.sample_rows(r, d)
            assert wc.n_rows(d) <= wc.N_SAMPLE or idx is None or len(idx) >= wc.N_SAMPLE, r.name
            want, share = wc.expected(kind, writer, n, r.name)
            print("%s / %s step %d (%s) / %s: %s%s" % (kind, writer, n, step.name, r.name, want, "" if share is None else " %.3f" % share))
            assert want in ("same", "refuses", "changed"), (r.name, step.name, want, share)
            if want == "changed":
                what = wc.measure(r, wc.restated(kind, writer, n + 1, r.name).what)
                assert share >= wc.threshold(what) + wc.MARGIN, (r.name, step.name, share)
            seen.add(want)
    assert seen


def test_the_writers_that_change_nothing_and_the_refusals_are_where_they_belong():
    for kind in wc.ENGINE_KINDS:
        assert {wc.expected(kind, "write_memory-general", 0, r.name)[0] for r in wc.readers_of(kind)} == {"same"}
        assert {wc.expected(kind, "set_user_base", 0, r.name)[0] for r in wc.readers_of(kind)} == {"same"}
    assert {wc.expected("plain", "train_step-unapplied", 1, r.name)[0] for r in wc.readers_of("plain")} == {"same"}
    assert {wc.expected("plain", "ingredients-set-and-cleared", 0, r.name)[0] for r in wc.readers_of("plain")} == {"same"}
    refused = {r.name for r in wc.readers_of("plain") if wc.expected("plain", "set_dish_categories", 1, r.name)[0] == "refuses"}
    assert refused == {"catalogue_rank", "topk_users_excluding-E64", "topk_users_excluding-tier2", "topk_profiles-excluding"}
    assert all(wc.expected("plain", "set_dish_categories", 2, name) == ("changed", 1.0) for name in refused)
    assert not any(wc.expected("plain", "set_dish_categories", 0, r.name)[0] == "refuses" for r in wc.readers_of("plain"))
    # a table at a time: compose_profiles reads Personal_Memory alone, cookable_dishes no table at all
    assert wc.expected("plain", "tables_updated-re", 0, "compose_profiles")[0] == "same"
    assert wc.expected("plain", "tables_updated-ce", 0, "compose_profiles")[0] == "same"
    assert wc.expected("plain", "tables_updated-pm", 0, "compose_profiles")[0] == "changed"
    assert wc.expected("market", "tables_updated-all", 0, "cookable_dishes")[0] == "same"
    assert wc.expected("market", "set_recipes", 0, "cookable_dishes")[0] == "changed"


def test_every_public_method_is_a_reader_a_writer_or_excused():
    """The next reader someone adds fails here until it joins the matrix (through stream_cases.ROWS, or a row of writer_cases)."""
    from foodrec_amd import ScoringEngine
    public = {n for n, f in inspect.getmembers(ScoringEngine, inspect.isfunction) if not n.startswith("_")}
    readers = {m for r in wc.READERS for m in r.covers if not m.startswith("_")}
    writers = set(wc.WRITER_COVERS)
    excused = set(wc.NOT_IN_MATRIX)
    assert readers <= public and writers <= public and excused <= public, (readers - public, writers - public, excused - public)
    assert not readers & writers and not readers & excused and not writers & excused
    assert public == readers | writers | excused, sorted(public - readers - writers - excused)
    assert all(len(reason) > 10 for reason in wc.NOT_IN_MATRIX.values())
    for name in ("_topk_menu", "_topk_menu_filtered", "_plan_menus", "_plan_groups"):       # private: asserted present by name
        assert name in wc.BY_NAME and wc.BY_NAME[name].covers == (name,) and inspect.isfunction(getattr(ScoringEngine, name))
    # every reader row stands in a kind of the GPU matrix, every writer's method is a step of some writer
    assert {r.name for kind in wc.ENGINE_KINDS for r in wc.readers_of(kind)} == set(wc.BY_NAME)
    names = " ".join(s.name for w in wc.WRITERS for s in w.steps)
    assert all(m in names for m in wc.WRITER_COVERS), [m for m in wc.WRITER_COVERS if m not in names]
    # stream_cases' rows are all here: the readers as they are, the writers as writers
    assert {r.name for r in st.ROWS} - set(wc.BY_NAME) == {"write_memory", "train_step-B128", "train_step-B1100"}


def _host_value(a):
    """what the GPU file compares of an answer: ids and ranks as int32, scores as float32"""
    v = np.asarray(a.value)
    return v.astype(np.float32) if a.what in ("scores", "rows") else v.astype(np.int32)


@pytest.mark.parametrize("kind,writer", [("plain", "write_memory-personal"), ("plain", "write_memory-general"), ("plain", "set_dish_categories"),
                                         ("plain", "set_user_base"), ("mlp", "set_mlp_head"), ("market", "set_recipes"),
                                         ("plain200", "tables_updated-re"), ("ing", "tables_updated-pm")])
def test_stale_and_wrongly_fresh_stand_ins_fail_the_comparison(kind, writer):
    """A stand-in reader that returns the BEFORE answer after the writer fails every "changed" pair; one that returns the AFTER
    answer of a writer that changes this reader fails the comparison a "same" pair makes; the true reader passes both."""
    for n in range(len(wc.WRITER_BY_NAME[writer].steps)):
        for r in wc.readers_of(kind):
            want = wc.expected(kind, writer, n, r.name)[0]
            if want == "refuses" or wc.refuses_weighted(r) and not wc.binary(wc.states(kind, writer)[n].cats):
                continue
            a, b = wc.restated(kind, writer, n, r.name), wc.restated(kind, writer, n + 1, r.name)
            before, after, what = _host_value(a), _host_value(b), wc.measure(r, a.what)
            assert wc.judge(what, before, after, want) is None, (r.name, want)
            if want == "changed":
                assert wc.judge(what, before, before.copy(), "changed") is not None, r.name          # the stale stand-in
            else:                                            # "same": an answer that moved (another writer's) must not pass for it
                moved = (kind, "tables_updated-all") if r.name != "cookable_dishes" else ("market", "set_recipes")
                other = wc.restated(*moved, 1, r.name)
                assert wc.judge(what, before, _host_value(other), "same") is not None, r.name


def test_the_numpy_batches_are_drawn_as_the_gpu_files_are():
    """(the GPU file compares the arrays themselves; here: shapes, and that every user is written to and most are trained)"""
    users, items, cats, sign, y, gm = wc.write_batch(64, st.model(64, "plain").cats)
    assert set(users) == set(range(wc.U)) and cats.shape == (600, wc.C) and gm.shape == (7, wc.C + 1, 64) and (y[:, 0] == 1).all()
    users, items, cats, labels = wc.train_batch(st.model(64, "plain").cats, 1100)
    assert len(set(users)) == wc.U and set(labels) == {0.0, 1.0}
