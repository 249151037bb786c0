"""The conditions that keep tests/test_gpu_stream_order.py from passing vacuously, checked without a GPU (stream_cases.py)."""
import inspect

import numpy as np
import pytest

import market_cases as mc
import stream_cases as st


@pytest.mark.parametrize("name", list(st.BY_NAME))            # the rows of the table and the steps of the two chains
def test_decoy_answer_differs_from_the_real_one(name):
    """A stage that ran off the stream, or a host read that did not wait for it, sees the decoy: that must change the answer."""
    real, decoy = st.request(name)
    assert all(not np.array_equal(real[k], decoy[k]) for k in real), [k for k in real if np.array_equal(real[k], decoy[k])]
    share = st.decoy_share(name)
    print("%s: the decoy differs in %.3f of the answer" % (name, share))
    assert share >= st.MIN_DIFFERENT, (name, share)


def test_second_tables_change_every_answer():
    """The late-table cases: a reader that still saw table set 0 must not pass for one that read table set 1."""
    for E, kind in ((64, "plain"), (64, "mlp"), (64, "ing"), (200, "plain")):
        a, b = st.model(E, kind, 0), st.model(E, kind, 1)
        rng = np.random.default_rng(5)
        users, items = rng.integers(0, st.U, st.NPAIRS), rng.integers(0, st.I, st.NPAIRS)
        assert st.different("scores", a.pairs(users, items), b.pairs(users, items)) >= st.MIN_DIFFERENT          # under the kind's own formula
        if kind == "ing":                                    # (its lists need H per user: the pairs stand for the kind)
            continue
        assert st.different("scores", a.pairs(users, items, head=False), b.pairs(users, items, head=False)) >= st.MIN_DIFFERENT
        held = rng.integers(0, st.I, 40)
        ranks = lambda m: np.array([st.sd.host_rank(row, int(p)) for row, p in zip(m.rows(np.arange(40), head=False), held)])
        assert st.different("ranks", ranks(a), ranks(b)) >= st.MIN_DIFFERENT
        sample = np.arange(0, st.U, 7)
        la = st.lists_among(a.rows(sample, head=False), st.K).value
        lb = st.lists_among(b.rows(sample, head=False), st.K).value
        assert st.different("lists", la, lb) >= st.MIN_DIFFERENT


def test_every_public_method_is_covered_or_excused():
    from foodrec_amd import ScoringEngine
    public = {n for n, f in inspect.getmembers(ScoringEngine, inspect.isfunction) if not n.startswith("_")}
    covered = {m for r in st.ROWS for m in r.covers}
    assert covered <= public, covered - public
    assert set(st.NOT_COVERED) <= public, set(st.NOT_COVERED) - public
    assert not covered & set(st.NOT_COVERED), covered & set(st.NOT_COVERED)
    assert public == covered | set(st.NOT_COVERED), sorted(public - covered - set(st.NOT_COVERED))
    assert all(len(reason) > 10 for reason in st.NOT_COVERED.values())


def test_error_rows_exist_and_name_late_inputs():
    for name, (user_key, item_key) in st.ERRORS.items():
        real = st.request(name)[0]
        assert user_key in real and (item_key is None or item_key in real), name


def test_cookable_is_market_cases_restatement():
    off, ids = st.recipes()
    assert (np.diff(off) > 0).all()
    rng = np.random.default_rng(3)
    for mm in (0, 1):
        market = rng.choice(st.R_INGREDIENTS, 30, replace=False)
        assert np.array_equal(st.cookable(market, mm), mc.restate(off, ids, st.R_INGREDIENTS, market, mm)[0])
    assert 10 * st.K < len(st.cookable(market, 1)) < st.I      # a real filter: more than k dishes remain, not all of them
