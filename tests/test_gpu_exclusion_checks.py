"""GPU tests of what the calls with exclusion lists share (foodrec_amd/csrc/m2d_exclusions.h): the one whole-list check launch behind
m2d_topk_users_excluding, m2d_topk_users_mlp_excluding and m2d_catalogue_rank_mlp -- one malformed device list per case, the same
report from all three --, and m2d_markets_topk's walk through the shared strike cursor at the edges of its 64-dish groups.

The malformed lists are reports through the id-error latch, not faults: every kernel clamps a segment into [0, offsets[n]] before it
reads (csr_segment), an id is only ever compared, and the check itself reads ids[i] for i < offsets[n] and ids[i - 1] for i > 0 --
offsets[n], the array's length, is left right in every case."""
import re

import numpy as np
import pytest

import market_cases as mc
import market_excluding_cases as mx
import market_request_cases as mq
import seen_dish_cases as sd
from helpers import mlp_head

pytestmark = pytest.mark.gpu

U, I, E, K = 8, 300, 32, 5                                   # I: past one 256-id step of the cursor and one 256-dish block
HELD = np.asarray([10, 290, 64, 255, 256, 1, 128, 200], np.int32)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _lists():
    """user u leaves out five ids of [37 u, 37 u + 37) -- ascending over the WHOLE array, so that an offset out of place leaves no
    second violation where two segments meet -- and the last user the last dish; none of HELD"""
    rng = np.random.default_rng(7)
    lists = []
    for u in range(U):
        pool = np.setdiff1d(np.arange(37 * u, 37 * u + 37), HELD)
        lists.append(np.sort(rng.permutation(pool)[:5]))
    lists[-1][-1] = I - 1
    off = np.zeros(U + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, np.concatenate(lists).astype(np.int32)


OFF, IDS = _lists()
SEG = slice(int(OFF[3]), int(OFF[4]))                        # user 3's segment
# case -> (edit of (offsets, ids), exception, (value, position) of the report)
CASES = {
    "first offset 1": (lambda o, x: o.__setitem__(0, 1), ValueError, (1, 0)),
    "first offset -1": (lambda o, x: o.__setitem__(0, -1), ValueError, (-1, 0)),
    "offset below its predecessor": (lambda o, x: o.__setitem__(4, o[3] - 1), ValueError, (int(OFF[3]) - 1, 4)),
    "id equal to I": (lambda o, x: x.__setitem__(SEG.stop - 1, I), IndexError, (I, SEG.stop - 1)),
    "id -1": (lambda o, x: x.__setitem__(SEG.start, -1), IndexError, (-1, SEG.start)),
    "id below its predecessor": (lambda o, x: x.__setitem__(SEG.start + 2, x[SEG.start + 1] - 1), ValueError,
                                 (int(IDS[SEG.start + 1]) - 1, SEG.start + 2)),
}
HOST_REJECTS = ("first offset 1", "first offset -1", "offset below its predecessor")     # exclusion_csr raises on these itself


def _report(eng):
    """check()'s exception: (type, (value, position))"""
    with pytest.raises((IndexError, ValueError)) as e:
        eng.check()
    m = re.search(r"(?:value|item id) (-?\d+) at position (\d+) ", str(e.value))
    assert m, str(e.value)
    return e.type, (int(m.group(1)), int(m.group(2)))


@pytest.fixture(scope="module")
def engines():
    """(engine without a head, engine under a small head) and each one's well-formed answers, computed once"""
    from foodrec_amd import ScoringEngine
    rng = np.random.default_rng(11)
    PM, RE, CE, cats = sd.exact_tables(rng, U, I, E)
    made = []
    for head in (False, True):
        eng = ScoringEngine(PM, RE, CE, coef=sd.COEF)
        eng.set_dish_categories(cats)
        if head:
            eng.set_mlp_head(*mlp_head(5 * E, 16, 16, rng))
        made.append(eng)
    plain, headed = made
    users = _dev(np.arange(U, dtype=np.int32))
    calls = {
        "topk_users_excluding": (plain, lambda x: plain.topk_users_excluding(users, K, x)),
        "topk_users_mlp_excluding": (headed, lambda x: headed.topk_users_mlp_excluding(users, K, x, 0)),
        "catalogue_rank(head=True)": (headed, lambda x: headed.catalogue_rank(users, _dev(HELD), x, head=True)),
        "catalogue_rank(head=False)": (plain, lambda x: plain.catalogue_rank(users, _dev(HELD), x)),
    }
    good = (_dev(OFF), _dev(IDS))
    before = {}
    for name, (eng, call) in calls.items():
        out = call(good)
        eng.check()
        before[name] = tuple(t.cpu().numpy().view(np.int32) for t in out)
    for name in ("topk_users_excluding", "topk_users_mlp_excluding"):        # (no listed dish is an excluded one)
        assert all(not set(before[name][1][u]) & set(IDS[OFF[u]:OFF[u + 1]]) for u in range(U)), name
    yield calls, before
    for eng in made:
        eng.close()


@pytest.mark.parametrize("case", list(CASES))
def test_one_malformed_list_one_report_from_every_call(engines, case):
    calls, before = engines
    edit, exc, where = CASES[case]
    off, ids = OFF.copy(), IDS.copy()
    edit(off, ids)
    assert off[-1] == len(ids) == OFF[-1]                       # the array's length stays right: nothing indexes outside `ids`
    bad = (_dev(off), _dev(ids))
    good = (_dev(OFF), _dev(IDS))
    for name in ("topk_users_excluding", "topk_users_mlp_excluding", "catalogue_rank(head=True)"):
        eng, call = calls[name]
        call(bad)
        assert _report(eng) == (exc, where), "%s: %s" % (name, case)
        eng.check()                                              # the latch is clear again
        again = call(good)
        eng.check()
        assert all(np.array_equal(a.cpu().numpy().view(np.int32), b) for a, b in zip(again, before[name])), "%s after %s" % (name, case)
    # catalogue_rank(head=False) sorts what it is given on the host: the host pair, where exclusion_csr lets the case through
    eng, call = calls["catalogue_rank(head=False)"]
    if case in HOST_REJECTS:
        with pytest.raises(ValueError, match="offsets must be non-decreasing from 0"):
            call((off, ids))
    else:
        call((off, ids))
        if case == "id below its predecessor":                   # ... sorted there: no error, one id of user 3 is another dish
            eng.check()
        else:                                                    # -1 sorts to the front of its segment, I to its end: where they stood
            assert _report(eng) == (exc, where), "catalogue_rank(head=False): %s" % case
    again = call((OFF, IDS))
    eng.check()
    assert all(np.array_equal(a.cpu().numpy().view(np.int32), b) for a, b in zip(again, before["catalogue_rank(head=False)"]))


# ---- m2d_markets_topk<LDS, true> through the shared cursor ---------------------------------------------------------------------------------
# segments that are empty, end at a 64-dish group's last id and at the next group's first, end on either side of the 256-dish block
# (and share) boundary, cover a whole group, hold the last dish
EDGE_LISTS = ((), (62, 63), (10, 64), (254, 255), (3, 256), tuple(range(64, 128)) + (I - 1,))


def _market_case(form):
    if form == "lds":                                            # 300 dishes, none with an empty list; the full market: every dish cookable
        c = mx.edge_case(I)
        users = np.arange(len(EDGE_LISTS), dtype=np.int32)
        return c, users, [np.arange(c.R, dtype=np.int32)] * len(users), list(EDGE_LISTS)
    c = mq.bitmap_case(mc.LB + 1)                                # R = 65 537: the bitmap through L2; the markets "all", "all twice
    order = (0, 1, 2, 5, 3, 4)                                   # reversed" and "every second" take the longer lists
    return c, c.users, c.markets, [EDGE_LISTS[j] for j in order]


@pytest.mark.parametrize("form", ["lds", "l2"])
def test_market_lists_at_the_cursors_group_and_block_edges(form):
    from foodrec_amd import ScoringEngine
    c, users, markets, excl = _market_case(form)
    assert c.I == I
    eng = ScoringEngine(c.PM, c.RE, c.CE, coef=c.coef)
    eng.set_dish_categories(c.cats)
    eng.set_recipes(c.off, c.ids, c.R)
    xoff, xids = mx.csr(excl)
    k, mm = 10, 1
    want = mx.restate(c.S, users, c.off, c.ids, c.R, markets, excl, mm, k)
    assert not mq.same_answer(want, mx.restate(c.S, users, c.off, c.ids, c.R, markets, None, mm, k))    # the lists matter
    try:
        for shares in (1, 3):
            eng.set_option("market_shares", shares)
            s, i, n = eng.topk_markets_excluding(_dev(users), list(markets), (_dev(xoff), _dev(xids)), k, mm, return_counts=True)
            eng.check()
            assert eng.last_kernel() == "m2d_markets_topk_excl_" + form
            assert eng.get_option("market_shares_used") == len(mq.share_bounds(I, shares))
            got = (s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy())
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), "%s, %d shares: ids / counts" % (form, shares)
            assert mq.same_answer(got, want), "%s, %d shares: score words" % (form, shares)
    finally:
        eng.close()
