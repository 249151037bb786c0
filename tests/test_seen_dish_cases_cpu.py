"""The inputs of tests/test_gpu_seen_dish_edges.py, checked without a GPU (tests/seen_dish_cases.py).

Two things.  Every recipe meets the conditions its GPU comparison rests on: float32 arithmetic is exact on it (so a rank is an
integer to compare, not a band), the intended dishes are there, the boundary cases sit exactly on their boundary, and each
share-count case reaches its share count from the launcher's formula.  And the comparison can see a subtly wrong kernel: the expected
values are recomputed under a stand-in of each fault and the share that changes is asserted -- at least 0.9 of the values a wrong
column count or row stride touches, at least one value in every case for the others."""
import numpy as np
import pytest

import seen_dish_cases as sd

LAUNCH_ES = (8, 32, 48, 64, 132)
VISIBLE = 0.9


def _assert_exact(r):
    S32 = sd.score_matrix(r.PM, r.RE, r.CE, r.cats, dtype=np.float32)
    assert S32.dtype == np.float32
    assert np.array_equal(S32.astype(np.float64), r.S, equal_nan=True), "float32 differs from float64 on the exact recipe"
    assert np.nanmax(np.abs(r.S)) <= 14.0
    ties = [r.I - np.unique(r.S[u][~np.isnan(r.S[u])]).size - int(np.isnan(r.S[u]).sum()) for u in range(r.U)]
    assert min(ties) >= 10, ties                              # id order decides many positions for every user
    return ties


@pytest.mark.parametrize("E", sd.WIDTHS)
def test_width_recipe_conditions(E):
    r = sd.width_recipe(E)
    ties = _assert_exact(r)
    print("E = %d: ties per user %d .. %d, max |s| %.3f" % (E, min(ties), max(ties), np.nanmax(np.abs(r.S))))
    assert all((r.cats[d] == 0).all() and np.isnan(r.S[:, d]).all() for d in sd.EMPTY_DISHES)
    assert np.array_equal(r.RE[sd.COPY_TO:], r.RE[:sd.COPIES]) and np.array_equal(r.cats[sd.COPY_TO:], r.cats[:sd.COPIES])
    assert np.array_equal(r.S[:, sd.COPY_TO:], r.S[:, :sd.COPIES], equal_nan=True)
    held = r.q_items.reshape(r.U, sd.WIDTH_HELD)
    assert all(set(sd.EMPTY_DISHES) | {7, sd.COPY_TO + 7} <= set(row.tolist()) for row in held)
    empt = set(np.flatnonzero(r.cats.sum(1) == 0).tolist())
    for q in range(0, r.q_users.size, 7):                     # the vectorised table is host_rank
        u, p, x = int(r.q_users[q]), int(r.q_items[q]), r.q_excl[q]
        assert r.rank0[q] == sd.host_rank(r.S[u], p) and r.rank1[q] == sd.host_rank(r.S[u], p, x), q
        assert p in x and len(x) >= 31
        assert (not any(e < p for e in empt)) or any(e < p for e in empt & set(x))
        assert (not any(e > p for e in empt)) or any(e > p for e in empt & set(x))
    E4, W = E // 4, sd.one_lane_width(E)
    if E in (12, 20, 48, 100):
        assert E4 < W and E4 % 16 != 0 and sd.row_width(E) != E     # a width without a kernel of its own, a padded row
    if E == 128:                                              # k = 10 is tier 1 here (K1 = 10): users it serves and users it hands on
        left = sd.survivors(r, range(r.U), r.lists, K1=10)
        assert (left == 10).any() and (left < 10).any(), left
    if E in (132, 256):
        assert W is None and (E4 % 16 == 1 or E4 == 64)


@pytest.mark.parametrize("E", LAUNCH_ES)
def test_launch_recipe_conditions(E):
    r = sd.launch_recipe(E)
    _assert_exact(r)
    assert all(np.isnan(r.S[:, d]).all() for d in sd.LAUNCH_EMPTY) and int(np.isnan(r.S[0]).sum()) == 4
    assert sum(d >= 256 for d in sd.LAUNCH_EMPTY) >= 2        # a NaN held-out dish past the first 256-dish block meets blk_hist
    off, ids = sd.user_sets(r, 3)
    assert np.array_equal(np.diff(off), np.full(r.U, 3))
    u, p = sd.random_queries(r, 500, 1)
    qoff, qids = sd.gather_csr(off, ids, u)
    got = sd.ranks_excluding(r.pos, u, p, qoff, qids)
    for q in range(0, 500, 11):
        assert got[q] == sd.host_rank(r.S[u[q]], int(p[q]), ids[off[u[q]]:off[u[q] + 1]]), q
    # per_query_csr is gather_csr for user-major queries
    a, b = sd.per_query_csr(off, ids, 3)
    c, d = sd.gather_csr(off, ids, np.repeat(np.arange(r.U), 3))
    assert np.array_equal(a, c) and np.array_equal(b, d) and a[-1] == 9 * r.U


@pytest.mark.parametrize("num_cu", [256, 104])
def test_share_count_cases_reach_their_share_count(num_cu):
    for E in (8, 132):
        for ns, n in sd.share_counts(E, num_cu).items():
            assert sd.rank_nsplit(E, n, num_cu) == ns, (E, ns, n)
            assert sd.excl_nsplit(E, n, num_cu) == ns, (E, ns, n)
    assert sd.share_counts(132, 256)[512] == 50               # clamped: ceil(128 * 256 / 50) = 656
    assert sd.share_counts(8, num_cu)[1] > 2048 * num_cu - 1  # m2d_rank_exclude's offsets: n + 1 of them, 2048 num_cu threads
    assert 4 * sd.share_counts(8, num_cu)[1] > 1024 * num_cu  # m2d_check_exclusions' ids at |X_u| = 4
    r = sd.launch_recipe(8)
    _, tiles = sd.pattern_tiles(r.cats)
    assert int(tiles[1:].sum()) % 3 != 0, tiles               # nsplit 3: the last share is shorter than the others
    r = sd.launch_recipe(132)
    pt, _ = sd.pattern_tiles(r.cats)
    assert (pt > 0).sum() < 2 * 512                           # n = 50 at 512 shares: fewer rows than 2 per share, some shares empty


def test_tier_boundary_cases_sit_on_the_boundary():
    r = sd.launch_recipe(64)
    users, lists = sd.boundary_sets(r)
    left = sd.survivors(r, users, lists)
    assert (left[0::2] == 10).all() and (left[1::2] == 9).all(), left
    for odd_short in (True, False):
        for at in (0, 64):
            users, lists = sd.odd_one_sets(r, odd_short, at)
            short = sd.survivors(r, users, lists) < 10
            assert short.sum() == (1 if odd_short else 64) and bool(short[at]) == odd_short and users.size == 65


@pytest.mark.parametrize("E", [32, 132])
def test_too_few_dishes_case(E):
    r = sd.launch_recipe(E)
    users, lists = sd.too_few_sets(r)
    _, tiles = sd.pattern_tiles(r.cats)
    pt_rows = np.bincount((r.cats != 0).astype(np.int64) @ (1 << np.arange(4)), minlength=16)[1:]
    want = sd.topk_lists(r.S, users, 16, lists)
    for j, x in enumerate(lists):
        assert 16 + len(set(x)) > pt_rows.max()
        assert sum(1 for e in sd.LAUNCH_EMPTY if e in x) == 2
        rest_empty = [e for e in sd.LAUNCH_EMPTY if e not in x]
        assert (want[j, :7] >= 0).all() and not np.isnan(r.S[users[j], want[j, :7]]).any()
        assert want[j, 7:9].tolist() == rest_empty and (want[j, 9:] == -1).all()


def test_xs_segments_straddle_the_lds_limit():
    for E in (8, 64):
        r = sd.launch_recipe(E)
        users, lens, lists = sd.xs_segments(r)
        assert set(lens.tolist()) == {0, 1, 59, 60, 61, 200} and [len(set(x)) for x in lists] == lens.tolist()
        for u, n, x in zip(users, lens, lists):
            assert set(sd.host_topk(r.S[u], 20, [])[:n].tolist()) <= set(x)
        want = sd.topk_lists(r.S, users, 16, lists)
        # (d) the lookup misses ids past position 60 of the ascending segment
        alt = sd.topk_lists(r.S, users, 16, [sorted(x)[:sd.EXCL_XS] for x in lists])
        ch = (want != alt).any(axis=1)
        assert not ch[lens <= 60].any() and ch[lens == 61].all() and ch[lens == 200].all(), (E, ch)


# ---- visibility -----------------------------------------------------------------------------------------------------------------------
def _width_expected(r, S, higher_id=False):
    pos = sd.positions(S, higher_id)
    ranks = np.concatenate([sd.ranks_excluding(pos, r.q_users, r.q_items), sd.ranks_excluding(pos, r.q_users, r.q_items, r.q_off, r.q_ids)])
    return ranks, sd.topk_lists(S, range(r.U), 16, r.lists, higher_id), sd.topk_lists(S, range(r.U), 1, r.lists, higher_id)


@pytest.mark.parametrize("E", sd.WIDTHS)
def test_wrong_column_count_stride_and_tie_rule_are_visible(E):
    r = sd.width_recipe(E)
    ranks, l16, l1 = _width_expected(r, r.S)
    masked = np.tile(r.cats[r.q_items].sum(1) > 0, 2)         # a NaN held-out dish is ranked by ids alone: no score touches it
    stand = {"a": sd.standin_no_last_column(r)}
    if sd.row_width(E) != E and E <= 128:                     # the one-lane kernels read the padded table; the 16-lane forms read RE
        stand["b"] = sd.standin_stride_E(r)
    for name, S in stand.items():
        ra, la16, la1 = _width_expected(r, S)
        share_r, share_l = float((ra != ranks)[masked].mean()), sd.changed_share(la16, l16)
        print("E = %d (%s): ranks changed %.3f, k = 16 lists %.3f, k = 1 lists %.3f" % (E, name, share_r, share_l, sd.changed_share(la1, l1)))
        assert share_r >= VISIBLE and share_l >= VISIBLE, (E, name, share_r, share_l)
    # (e) ties to the higher id
    re_, le16, _ = _width_expected(r, r.S, higher_id=True)
    print("E = %d (e): ranks changed %d, k = 16 lists %d" % (E, (re_ != ranks).sum(), (le16 != l16).any(axis=1).sum()))
    assert (re_ != ranks).any() and (le16 != l16).any()


@pytest.mark.parametrize("E", [8, 132])
def test_a_lost_tile_and_the_tie_rule_are_visible_in_the_share_cases(E):
    r = sd.launch_recipe(E)
    off, ids = sd.user_sets(r, 3)
    u, p = sd.random_queries(r, 4096, 2)                      # (a sample: the calls hold these and up to half a million more)
    qoff, qids = sd.gather_csr(off, ids, u)
    want = sd.ranks_excluding(r.pos, u, p, qoff, qids)
    alt_pos = sd.positions(r.S, higher_id=True)
    assert (sd.ranks_excluding(alt_pos, u, p, qoff, qids) != want).any()
    voff, vids, vwant = sd.variant_lists(E, 4, 3)
    rows = np.repeat(np.arange(r.U), sd.VARIANTS)
    vlists = [vids[voff[j]:voff[j + 1]] for j in range(rows.size)]
    for ns in (2, 3, 512):
        lost = sd.last_tile_of_first_share(r.cats, ns)
        assert 0 < lost.size <= 32
        loff, lids = sd.lists_csr([np.concatenate([ids[off[v]:off[v + 1]], lost]) for v in range(r.U)])
        a, b = sd.gather_csr(loff, lids, u)
        assert (sd.ranks_excluding(r.pos, u, p, a, b) != want).any(), ns
        alt = sd.topk_lists(r.S, rows, 3, [np.concatenate([x, lost]) for x in vlists])
        if ns != 512:
            assert (alt != vwant).any(), ns
    assert (sd.topk_lists(r.S, rows, 3, vlists, higher_id=True) != vwant).any()


@pytest.mark.parametrize("E", LAUNCH_ES)
def test_the_tie_rule_is_visible_in_the_launch_recipes(E):
    r = sd.launch_recipe(E)
    alt = sd.positions(r.S, higher_id=True)
    assert (alt != r.pos).mean() > 0.01
    users, lists = sd.boundary_sets(r)
    assert (sd.topk_lists(r.S, users, 10, lists, higher_id=True) != sd.topk_lists(r.S, users, 10, lists)).any()
