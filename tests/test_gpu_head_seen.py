"""GPU tests of seen-dish filtering under the MLP head (m2d_topk_users_mlp_excluding, m2d_catalogue_rank_mlp; DESIGN.md section
8.6).  The exact reference is the engine's own pair words: all nU x I pairs through score_pairs_mlp, each row ordered on the host
by the key rule over the dishes not excluded (tests/head_seen_cases.py) -- ids, score words and ranks compared as integers, no
tolerance.  One tie to the float64 oracle per head kernel family."""
import functools
import types

import numpy as np
import pytest

import head_seen_cases as hs
import topk_mlp_cases as tc
from helpers import mlp_head

pytestmark = pytest.mark.gpu

DEFAULT_P = 1 << 22
POISON_I, POISON_F = -777, -12345.0


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(r, head=True, tables=None, user_base=0):
    from foodrec_amd import ScoringEngine
    PM, RE, CE = tables if tables is not None else (r.PM, r.RE, r.CE)
    eng = ScoringEngine(PM, RE, CE, coef=r.coef, user_base=user_base)
    eng.set_dish_categories(r.cats)
    if r.ing is not None:
        eng.set_ingredients(*r.ing)
    if head:
        eng.set_mlp_head(*(r.head if head is True else head))
    return eng


def _all_words(eng, r, users, base=0):
    """[len(users), I] float32: every pair's score_pairs_mlp word"""
    u = np.repeat(np.asarray(users, np.int32) + base, r.I)
    d = np.tile(np.arange(r.I, dtype=np.int32), len(users))
    w = eng.score_pairs_mlp(_dev(u), _dev(d))
    eng.check()
    return w.cpu().numpy().reshape(len(users), r.I)


@functools.lru_cache(maxsize=None)
def _words(name):
    """The recipe's words, computed once and shared (read-only), and the kernel that scored them."""
    r = hs.recipe(name)
    eng = _engine(r)
    w = _all_words(eng, r, r.users)
    kernel = eng.last_kernel()
    eng.close()
    w.setflags(write=False)
    return w, kernel


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_rows(got, want, what=""):
    gs, gi = got
    ws, wi = want
    assert np.array_equal(gi, wi), "%s: ids\n%s\nvs\n%s" % (what, gi[np.any(gi != wi, 1)][:3], wi[np.any(gi != wi, 1)][:3])
    ok = wi >= 0
    assert np.array_equal(_bits(gs)[ok], _bits(ws)[ok]), "%s: score words" % what
    assert np.isnan(gs[~ok]).all(), "%s: padding scores" % what


def _lists(eng, users, k, excl, candidates=0, chunk=None):
    if chunk is not None:
        eng.set_option("topk_mlp_chunk_pairs", chunk)
    s, i = eng.topk_users_mlp_excluding(_dev(np.asarray(users, np.int32)), k, None if excl is None else list(excl), candidates)
    eng.check()
    return s.cpu().numpy(), i.cpu().numpy()


def _ranks(eng, users, held, excl):
    rk, sc = eng.catalogue_rank(_dev(np.asarray(users, np.int32)), _dev(np.asarray(held, np.int32)), None if excl is None else list(excl),
                                head=True)
    eng.check()
    return rk.cpu().numpy().astype(np.int64), sc.cpu().numpy()


def _rank_consistency(eng, users, lists, excl, what=""):
    """catalogue_rank(head=True) of every listed dish is its column"""
    ids = lists[1]
    n, k = ids.shape
    rows, cols = np.nonzero(ids >= 0)
    if len(rows) == 0:
        return
    got, sc = _ranks(eng, np.asarray(users)[rows], ids[rows, cols], [excl[j] for j in rows])
    assert np.array_equal(got, cols), "%s: rank of a listed dish is not its column: %s" % (what, np.flatnonzero(got != cols)[:5])
    assert np.array_equal(_bits(sc), _bits(lists[0][rows, cols])), "%s: held-out word differs from the listed word" % what


# ---- 1. every block size and head kernel family: lists, ranks, the oracle ------------------------------------------------------
@pytest.mark.parametrize("name", ["pc", "gather", "generic", "ing", "w255", "w256", "w257", "w16385"])
def test_lists_and_ranks_are_the_key_rule_on_the_engines_words(name):
    r, ref = hs.recipe(name), hs.reference(name)
    words, kernel = _words(name)
    excl = hs.exclusions(name)
    if name in hs.FAMILIES:
        assert kernel == hs.FAMILIES[name]
    eng = _engine(r)
    k = hs.LIST_K
    got = _lists(eng, r.users, k, excl)
    assert eng.last_kernel() == kernel and eng.get_option("topk_mlp_launches") == 1
    _assert_rows(got, hs.filtered_lists(words, excl, k), name)
    assert not np.array_equal(got[1], hs.filtered_lists(words, excl, k, "ignore")[1])
    _rank_consistency(eng, r.users, got, excl, name)
    # held-out dishes: rank 0, the last-ranked one, an excluded one (ignored in its own X), some behind excluded dishes
    rng = np.random.default_rng(5)
    rows, held = [], []
    for j in range(len(r.users)):
        h = hs.held_out(ref[j], excl[j], rng)
        rows += [j] * len(h)
        held += h
    rows, held = np.asarray(rows), np.asarray(held)
    qx = [excl[j] for j in rows]
    rk, sc = _ranks(eng, r.users[rows], held, qx)
    assert eng.get_option("topk_mlp_launches") == 2                # the held-out launch and one dish range
    want = hs.ranks(words, rows, held, qx)
    assert np.array_equal(rk, want), (name, np.flatnonzero(rk != want)[:5])
    assert np.array_equal(_bits(sc), _bits(words[rows, held]))
    assert (rk == 0).any() and rk.max() >= r.I - 40
    # the oracle: brackets for the ranks, compare_lists user by user over the remaining dishes
    lo, hi = hs.rank_brackets(ref, rows, held, qx)
    assert np.all((lo <= rk) & (rk <= hi)), name
    if name in hs.FAMILIES:
        sharp = []
        for j in range(len(r.users)):
            left = np.setdiff1d(np.arange(r.I), np.asarray(excl[j]))
            sharp.append(tc.compare_lists(got[0][j:j + 1], got[1][j:j + 1], ref[j:j + 1, left], k, ids=left[None, :], what="%s user %d" % (name, j))[0])
        print("%s: sharp users %.2f, exact ranks %.2f" % (name, np.mean(sharp), np.mean(lo == hi)))
    eng.close()


# ---- 2. k = 1 / 10 / 64, the filtered prefix, segment lengths, repeated users, null exclusions --------------------------------------
def test_k_edges_prefix_of_the_unfiltered_list_and_segment_lengths():
    import torch
    from foodrec_amd import _native
    r = hs.recipe("pc")
    words, _ = _words("pc")
    eng = _engine(r)
    excl = hs.exclusions("pc")
    full = _lists(eng, r.users, 64, None)
    _assert_rows(full, hs.filtered_lists(words, None, 64), "k = 64, no exclusions")
    plain = eng.topk_users_mlp(_dev(r.users), 64)
    _assert_rows(full, (plain[0].cpu().numpy(), plain[1].cpu().numpy()), "null exclusions are topk_users_mlp")
    for k in (1, 10, 64):
        got = _lists(eng, r.users, k, excl)
        _assert_rows(got, hs.filtered_lists(words, excl, k), "k = %d" % k)
        checked = 0
        for j in range(len(r.users)):                               # the unfiltered k = 64 list with the excluded ids struck out
            keep = ~np.isin(full[1][j], np.asarray(excl[j]))
            if (~keep).sum() <= 64 - k:
                assert np.array_equal(got[1][j], full[1][j][keep][:k]) and np.array_equal(_bits(got[0][j]), _bits(full[0][j][keep][:k]))
                checked += 1
        assert checked >= (len(r.users) if k < 64 else 0)
    # segment lengths 0 / 1 / 63 / 64 / 65 / 300 with repeats, through the host path; the same user twice with different X
    rng = np.random.default_rng(3)
    users = np.array([0, 1, 2, 3, 4, 5, 5, 5], np.int32)
    best = hs.filtered_lists(words, None, 3)[1]
    lens = (0, 1, 63, 64, 65, 300, 2, 40)
    lists = []
    for u, n in zip(users, lens):
        x = list(best[u][:min(n, 3)]) + list(rng.choice(r.I, max(n - 3, 0), replace=False))
        lists.append([int(d) for d in x[:n]] + [int(d) for d in x[:min(n, 2)]])         # (repeats)
    got = _lists(eng, users, 10, lists)
    _assert_rows(got, hs.filtered_lists(words[users], lists, 10), "segment lengths")
    assert not np.array_equal(got[1][5], got[1][6]) and not np.array_equal(got[1][6], got[1][7])
    _rank_consistency(eng, users, got, lists, "segment lengths")
    # the C ABI with excl_off = NULL passes every `candidates` value m2d_topk_users_mlp takes through to it
    out_s = torch.empty((len(r.users), 10), dtype=torch.float32, device="cuda")
    out_i = torch.empty((len(r.users), 10), dtype=torch.int32, device="cuda")
    ut = _dev(r.users)
    rc = _native.lib().m2d_topk_users_mlp_excluding(eng._h, ut.data_ptr(), len(r.users), 10, 64, None, None, out_s.data_ptr(), out_i.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream)
    assert rc == _native.M2D_OK
    eng.check()
    two = eng.topk_users_mlp(ut, 10, 64)
    assert np.array_equal(out_i.cpu().numpy(), two[1].cpu().numpy()) and np.array_equal(_bits(out_s.cpu().numpy()), _bits(two[0].cpu().numpy()))
    eng.close()


# ---- 3. dish-range boundaries ---------------------------------------------------------------------------------------------------
def test_range_boundaries_give_the_same_words_and_ranks_at_every_chunk_size():
    r, ref = hs.recipe("pc5000"), hs.reference("pc5000")
    words, _ = _words("pc5000")
    excl = hs.exclusions("pc5000")
    assert all(set(hs.RANGE_IDS) <= set(excl[j]) for j in range(0, len(r.users), 2))
    want = hs.filtered_lists(words, excl, r.k)
    # every user excludes a range's first id or another multiple of 64, and everything in front of it: a selection that loses that
    # id lists it first (the stand-ins of tests/test_head_seen_cases_cpu.py)
    front = hs.front_exclusions(words)
    front_want = hs.filtered_lists(words, front, r.k)
    lost = np.array([hs.WINDOW_DISHES[j % len(hs.WINDOW_DISHES)] for j in range(len(r.users))])
    assert np.all(hs.filtered_lists(words, front, r.k, "mult64")[1][:, 0] != front_want[1][:, 0]) and not np.any(front_want[1] == lost[:, None])
    rng = np.random.default_rng(9)
    rows = np.repeat(np.arange(len(r.users)), 4)                    # per user: the last dish, an excluded one, one behind, 4 096
    held = np.concatenate([hs.held_out(ref[j], excl[j], rng, 1)[1:] + [4096] for j in range(len(r.users))])
    qx = [excl[j] for j in rows]
    want_rk = hs.ranks(words, rows, held, qx)
    eng = _engine(r)
    for P in (256, 2048, DEFAULT_P):
        got = _lists(eng, r.users, r.k, excl, chunk=P)
        assert eng.get_option("topk_mlp_launches") == tc.chunk_geometry(len(r.users), r.I, P)[2], P
        _assert_rows(got, want, "chunk %d" % P)
        rk, _ = _ranks(eng, r.users[rows], held, qx)
        assert eng.get_option("topk_mlp_launches") == 1 + tc.chunk_geometry(len(rows), r.I, P)[2], P
        assert np.array_equal(rk, want_rk), "ranks at chunk %d" % P
        _rank_consistency(eng, r.users, got, excl, "chunk %d" % P)
        front_got = _lists(eng, r.users, r.k, front)
        _assert_rows(front_got, front_want, "everything in front of a window edge excluded, chunk %d" % P)
        _rank_consistency(eng, r.users, front_got, front, "window edges, chunk %d" % P)
    eng.close()


def test_copies_on_both_sides_of_a_range_boundary_with_one_of_the_pair_excluded():
    r = hs.recipe("ties")
    words, _ = _words("ties")
    assert np.array_equal(_bits(words[:, :tc.TIE_COPIES]), _bits(words[:, tc.TIE_SHIFT:tc.TIE_SHIFT + tc.TIE_COPIES]))
    order = hs.filtered_lists(words, None, r.I)[1]
    excl, lead = [], []
    for j in range(len(r.users)):      # everything in front of the user's best original goes, and one of the pair: even users lose the original
        at = int(np.flatnonzero(order[j] < tc.TIE_COPIES)[0])
        d = int(order[j][at])
        assert order[j][at + 1] == d + tc.TIE_SHIFT
        excl.append(tuple(int(x) for x in order[j][:at]) + ((d,) if j % 2 == 0 else (d + tc.TIE_SHIFT,)))
        lead.append(d + tc.TIE_SHIFT if j % 2 == 0 else d)
    want = hs.filtered_lists(words, excl, r.k)
    assert want[1][:, 0].tolist() == lead
    assert not np.array_equal(want[1], hs.filtered_lists(words, excl, r.k, "ties_high")[1])
    eng = _engine(r)
    for P in (2048, DEFAULT_P):                                    # ranges [0, 2048) and [2048, 2200); one range
        got = _lists(eng, r.users, r.k, excl, chunk=P)
        _assert_rows(got, want, "ties, chunk %d" % P)
        _rank_consistency(eng, r.users, got, excl, "ties, chunk %d" % P)
    eng.close()


# ---- 4. tails: 40 dishes, 30 of them with an empty mask -----------------------------------------------------------------------------
def test_tails_few_dishes_left_none_left_and_nan_dishes():
    r = hs.recipe("nan40")
    words, _ = _words("nan40")
    empty = np.flatnonzero(r.cats.sum(1) == 0)
    assert len(empty) == 30 and np.isnan(words[:, empty]).all()
    eng = _engine(r)
    everything = tuple(range(r.I))
    for what, x in (("all but 3", everything[:11] + everything[14:]), ("every dish", everything), ("the NaN dishes", tuple(int(d) for d in empty)),
                    ("nothing", ())):
        excl = [x] * len(r.users)
        got = _lists(eng, r.users, 16, excl)
        _assert_rows(got, hs.filtered_lists(words, excl, 16), what)
        left = r.I - len(x)
        assert (got[1] >= 0).sum(1).tolist() == [min(16, left)] * len(r.users), what
        _rank_consistency(eng, r.users, got, excl, what)
    # held-out NaN dishes, with and without NaN dishes of lower id excluded
    rows = np.arange(len(r.users))
    held = np.resize(empty[[0, 7, 29]], len(rows))
    qx = [tuple(int(d) for d in empty[1:5]) + (3,)] * len(rows)
    rk, _ = _ranks(eng, r.users[rows], held, qx)
    assert np.array_equal(rk, hs.ranks(words, rows, held, qx))
    assert not np.array_equal(rk, hs.ranks(words, rows, held, qx, "count_excluded"))
    eng.close()


# ---- 5. two-stage with exclusions ---------------------------------------------------------------------------------------------------
def test_two_stage_takes_its_candidates_from_the_exclusion_retrieval():
    r = hs.recipe("base600")
    excl = list(hs.exclusions("base600"))
    excl[0] = tuple(range(5, r.I))                                  # 5 dishes left: fewer than K1
    excl[1] = tuple(range(r.I))                                     # none
    base = _engine(r, head=False)
    eng = _engine(r)
    for K1, k in ((16, 10), (10, 10)):
        _, cand = base.topk_users_excluding(_dev(r.users), K1, excl)
        base.check()
        cand = cand.cpu().numpy()
        assert (cand[0] >= 0).sum() == 5 and (cand[1] >= 0).sum() == 0
        hw = eng.score_pairs_mlp(_dev(np.repeat(r.users, K1)), _dev(np.maximum(cand, 0).reshape(-1).astype(np.int32)))
        hw = hw.cpu().numpy().reshape(cand.shape)
        want = hs.two_stage(cand, hw, k)
        assert not np.array_equal(want[1][0], hs.two_stage(cand, hw, k, "keep_minus1")[1][0])
        got = _lists(eng, r.users, k, excl, candidates=K1)
        assert eng.get_option("topk_mlp_launches") == 1
        _assert_rows(got, want, "K1 = %d" % K1)
        assert not np.isin(got[1], -1)[2:].any()
        for j in range(len(r.users)):
            assert not set(got[1][j].tolist()) & set(excl[j])
    with pytest.raises(ValueError, match="candidates"):
        _lists(eng, r.users, 10, excl, candidates=17)
    eng.close()
    base.close()
    ri = hs.recipe("ing")
    eng = _engine(ri)
    with pytest.raises(Exception, match="m2d_topk_users_mlp_excluding: the ingredient table is set"):
        _lists(eng, ri.users, 10, hs.exclusions("ing"), candidates=16)
    got = _lists(eng, ri.users, 10, hs.exclusions("ing"))           # the engine stays usable: the exact mode
    _assert_rows(got, hs.filtered_lists(_words("ing")[0], hs.exclusions("ing"), 10), "ing after the refusal")
    eng.close()


# ---- 6. user_base, latched errors (C ABI, poisoned buffers, guard rows) ------------------------------------------------------------
def test_user_base_and_latched_errors():
    import torch
    from foodrec_amd import _native
    lib = _native.lib()
    r = hs.recipe("pc")
    words, _ = _words("pc")
    excl = hs.exclusions("pc")
    nU, k = len(r.users), 10
    want = hs.filtered_lists(words, excl, k)
    eng = _engine(r, user_base=7000)
    st = torch.cuda.current_stream().cuda_stream

    def call(users, off, ids):
        """rows 1 .. nU of poisoned buffers with a guard row on either side"""
        out_s = torch.full((nU + 2, k), POISON_F, dtype=torch.float32, device="cuda")
        out_i = torch.full((nU + 2, k), POISON_I, dtype=torch.int32, device="cuda")
        ut, ot, it = _dev(users), _dev(off), _dev(ids)
        rc = lib.m2d_topk_users_mlp_excluding(eng._h, ut.data_ptr(), nU, k, 0, ot.data_ptr(), it.data_ptr(), out_s[1].data_ptr(), out_i[1].data_ptr(), st)
        assert rc == _native.M2D_OK
        torch.cuda.synchronize()
        s, i = out_s.cpu().numpy(), out_i.cpu().numpy()
        assert (i[[0, -1]] == POISON_I).all() and (s[[0, -1]] == POISON_F).all(), "a guard row was written"
        return s[1:-1], i[1:-1]

    def call_rank(users, held, off, ids):
        out = torch.full((nU + 2,), POISON_I, dtype=torch.int32, device="cuda")
        ut, ht, ot, it = _dev(users), _dev(held), _dev(off), _dev(ids)
        rc = lib.m2d_catalogue_rank_mlp(eng._h, ut.data_ptr(), ht.data_ptr(), nU, ot.data_ptr(), it.data_ptr(), out[1:].data_ptr(), None, st)
        assert rc == _native.M2D_OK
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert o[0] == POISON_I and o[-1] == POISON_I
        return o[1:-1]

    off, ids = hs.csr(excl)
    users = r.users + 7000
    _assert_rows(call(users, off, ids), want, "user_base 7000")
    eng.check()
    held = want[1][:, 4].copy()
    assert np.array_equal(call_rank(users, held, off, ids), np.full(nU, 4))
    eng.check()
    bad = users.copy()
    bad[5] = 6999
    call(bad, off, ids)
    with pytest.raises(IndexError, match="user id 6999"):
        eng.check()
    others = np.arange(nU) != 7
    seg = slice(int(off[7]), int(off[8]))
    flat_off, flat_ids = np.arange(nU + 1, dtype=np.int64), np.full(nU, 5, np.int32)       # every user leaves out dish 5
    flat_want = hs.filtered_lists(words, [(5,)] * nU, k)
    _assert_rows(call(users, flat_off, flat_ids), flat_want, "one id per user")
    # (one violation per case, and none that a second kernel thread could report in its place: the first report wins)
    for what, o2, x2, edit, exc, text in (
            ("an excluded id past the catalogue", off, ids, lambda o, x: x.__setitem__(seg.stop - 1, r.I), IndexError,
             "item id %d at position %d " % (r.I, seg.stop - 1)),
            ("a negative excluded id", off, ids, lambda o, x: x.__setitem__(seg.start, -5), IndexError, "item id -5 at position %d " % seg.start),
            ("an unsorted segment", off, ids, lambda o, x: x.__setitem__(seg.start + 2, x[seg.start]), ValueError,
             "not ascending: value %d at position %d " % (ids[seg.start], seg.start + 2)),
            ("an offset below its predecessor", flat_off, flat_ids, lambda o, x: o.__setitem__(8, o[7] - 1), ValueError,
             "not ascending: value 6 at position 8 "),
            ("a first offset that is not 0", flat_off, flat_ids, lambda o, x: o.__setitem__(0, 1), ValueError, "not ascending: value 1 at position 0 "),
            ("a negative first offset", flat_off, flat_ids, lambda o, x: o.__setitem__(0, -1), ValueError, "not ascending: value -1 at position 0 ")):
        o2, x2 = o2.copy(), x2.copy()
        edit(o2, x2)
        got = call(users, o2, x2)
        with pytest.raises(exc, match=text):
            eng.check()
        if "offset" not in what:
            _assert_rows((got[0][others], got[1][others]), (want[0][others], want[1][others]), what)
        else:                                                       # the segment in front of the bad offset is the one spoiled row
            rest = np.arange(nU) != (7 if "predecessor" in what else 0)
            _assert_rows((got[0][rest], got[1][rest]), (flat_want[0][rest], flat_want[1][rest]), what)
        call_rank(users, held, o2, x2)
        with pytest.raises(exc, match=text):
            eng.check()
    bad_held = held.copy()
    bad_held[3] = r.I
    call_rank(users, bad_held, off, ids)
    with pytest.raises(IndexError, match="item id %d" % r.I):
        eng.check()
    _assert_rows(call(users, off, ids), want, "the engine stays usable")
    eng.check()
    # argument errors
    no_head = _engine(r, head=False)
    ut, ot, it = _dev(users), _dev(off), _dev(ids)
    buf = torch.empty((nU, k), dtype=torch.int32, device="cuda")
    assert lib.m2d_topk_users_mlp_excluding(no_head._h, ut.data_ptr(), nU, k, 0, ot.data_ptr(), it.data_ptr(), buf.data_ptr(), buf.data_ptr(), st) == \
        _native.M2D_ERR_NOT_CONFIGURED == lib.m2d_catalogue_rank_mlp(no_head._h, ut.data_ptr(), ut.data_ptr(), nU, None, None, buf.data_ptr(), None, st)
    no_head.close()
    assert lib.m2d_topk_users_mlp_excluding(eng._h, ut.data_ptr(), nU, k, 0, ot.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), st) == _native.M2D_ERR_INVALID_ARG
    assert lib.m2d_catalogue_rank_mlp(eng._h, ut.data_ptr(), ut.data_ptr(), nU, ot.data_ptr(), None, buf.data_ptr(), None, st) == _native.M2D_ERR_INVALID_ARG
    assert lib.m2d_catalogue_rank_mlp(eng._h, ut.data_ptr(), None, nU, None, None, buf.data_ptr(), None, st) == _native.M2D_ERR_INVALID_ARG
    eng.close()


# ---- 7. readers after writers -------------------------------------------------------------------------------------------------------
def test_results_follow_write_memory_table_edits_and_a_new_head():
    import torch
    r = hs.recipe("pc")
    excl = hs.exclusions("pc")
    rng = np.random.default_rng(78)
    eng = _engine(r)

    def both(e):
        lists = _lists(e, r.users, r.k, excl)
        rk, sc = _ranks(e, r.users, lists[1][:, 0] * 0 + 17, excl)
        return lists, rk, sc

    before = both(eng)
    # write_memory: results equal a fresh engine's on the written tables
    t = lambda a: torch.as_tensor(a, device="cuda")
    B, L = 600, 7
    wu = (np.arange(B) % r.U).astype(np.int32)
    wi = rng.choice(r.I, B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32)
    y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, r.C + 1, r.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(r.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5)
    eng.check()
    written = both(eng)
    fresh = _engine(r, tables=(eng.pm.cpu().numpy(), eng.re.cpu().numpy(), eng.ce.cpu().numpy()))
    want = both(fresh)
    fresh.close()
    _assert_rows(written[0], want[0], "after write_memory")
    assert np.array_equal(written[1], want[1]) and np.array_equal(_bits(written[2]), _bits(want[2]))
    assert not np.array_equal(written[0][1], before[0][1]) and not np.array_equal(written[1], before[1]), "write_memory changed nothing"
    RE2 = (rng.standard_normal(r.RE.shape) * 0.5).astype(np.float32)
    PM2 = (rng.standard_normal(r.PM.shape) * 0.5).astype(np.float32)
    eng.re.copy_(torch.as_tensor(RE2))                               # in place: the engine borrows these tensors
    eng.pm.copy_(torch.as_tensor(PM2))
    eng.tables_updated()
    after = both(eng)
    fresh = _engine(r, tables=(PM2, RE2, r.CE))
    want = both(fresh)
    _assert_rows(after[0], want[0], "after the table edit")
    assert np.array_equal(after[1], want[1]) and np.array_equal(_bits(after[2]), _bits(want[2]))
    assert not np.array_equal(after[0][1], before[0][1]) and not np.array_equal(after[1], before[1])
    fresh.close()
    head2 = mlp_head((r.C + 1) * r.E, r.H1, r.H2, rng, scale=4.0)
    eng.set_mlp_head(*head2)
    fresh = _engine(r, head=head2, tables=(PM2, RE2, r.CE))
    new, want = both(eng), both(fresh)
    _assert_rows(new[0], want[0], "after the new head")
    assert np.array_equal(new[1], want[1]) and not np.array_equal(new[0][1], after[0][1])
    eng.close()
    fresh.close()


# ---- 8. the Python surface ----------------------------------------------------------------------------------------------------------
def test_torch_ops_model_and_evaluators():
    import torch
    import foodrec_amd
    r = hs.recipe("gather")
    words, _ = _words("gather")
    excl = hs.exclusions("gather")
    args = types.SimpleNamespace(num_categories=r.C, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    model.set_mlp_head(*r.head)
    eng = model.engine
    want = hs.filtered_lists(words, excl, 10)
    off, ids = hs.csr(excl)
    s, i = torch.ops.m2d.topk_users_mlp_excluding(eng.id, _dev(r.users), 10, 0, _dev(off), _dev(ids))
    _assert_rows((s.cpu().numpy(), i.cpu().numpy()), want, "torch op")
    rk, sc = torch.ops.m2d.catalogue_rank_mlp(eng.id, _dev(r.users), _dev(want[1][:, 7].copy()), _dev(off), _dev(ids))
    assert rk.cpu().numpy().tolist() == [7] * len(r.users)
    users = r.users.tolist()
    _assert_rows(model.topk_head(users, 10, exclude={u: excl[u] for u in users}), want, "Model.topk_head, dict")
    _assert_rows(model.topk_head(users, 10, exclude=[list(x) for x in excl]), want, "Model.topk_head, list")
    _assert_rows(model.topk_head(users, 10), hs.filtered_lists(words, None, 10), "Model.topk_head, no exclusions")
    with pytest.raises(ValueError, match="head=True together with exclude"):
        model.topk(users, 5, exclude=[[1]] * len(users), head=True)
    # evaluate_model_full(head=True): a host loop of getHitRatio / getNDCG over the filtered ranking of the same words
    d2c = {str(d): r.cats[d].tolist() for d in range(r.I)}
    rng = np.random.default_rng(4)
    K = 10
    test = {str(u): [int(want[1][u][rng.integers(0, 10)]) if u % 2 else int(rng.integers(0, r.I))] for u in users}
    train = {str(u): [d for d in excl[u] if d != test[str(u)][0]] for u in users}
    hits, ndcgs = foodrec_amd.evaluate_model_full(None, model, test, train, K, d2c, head=True)
    plain = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))        # (the base rank refuses a head)
    base_h, base_n = foodrec_amd.evaluate_model_full(None, plain, test, train, K, d2c)
    assert (base_h, base_n) == tuple(foodrec_amd.evaluate_model_full(None, plain, test, train, K, d2c, head=False))
    with pytest.raises(ValueError, match="the MLP head is set"):
        foodrec_amd.evaluate_model_full(None, model, test, train, K, d2c)
    for u in users:
        lst = hs.filtered_lists(words[u:u + 1], [train[str(u)]], K)[1][0].tolist()
        assert hits[u] == foodrec_amd.getHitRatio(lst, test[str(u)][0]) and ndcgs[u] == foodrec_amd.getNDCG(lst, test[str(u)][0]), u
    assert sum(hits) >= len(users) // 2 and (hits, ndcgs) != (base_h, base_n)
    # evaluate_model(head=True): rank_candidates under the head; head=False is the call as it was
    negs = {str(u): [int(d) for d in rng.choice(r.I, 100, replace=False)] for u in users}
    h1, n1 = foodrec_amd.evaluate_model(None, model, test, negs, K, d2c, head=True)
    h0, n0 = foodrec_amd.evaluate_model(None, model, test, negs, K, d2c)
    assert (h0, n0) == tuple(foodrec_amd.evaluate_model(None, model, test, negs, K, d2c, head=False))
    compared = 0
    for u in users:
        items = [test[str(u)][0]] + negs[str(u)][50:100]
        table = {}
        for it in items:
            table[it] = words[u][it]
        lst = sorted(table, key=lambda d: (-table[d], items.index(d)))[:K]
        if len(set(np.float32(table[d]) for d in lst)) == K:        # (distinct words: the order does not hang on the tie rule)
            assert h1[u] == foodrec_amd.getHitRatio(lst, items[0]) and n1[u] == foodrec_amd.getNDCG(lst, items[0]), u
            compared += 1
    assert compared >= 0.9 * len(users), compared
    assert (h1, n1) != (h0, n0)
    # NaN among a user's candidate scores: the row takes the host sequence (evaluate.py:35-66) with predict_extended(head=True)'s
    # scores -- "nan40": 30 of 40 dishes have an empty mask, so every user's 51 candidates hold some
    n = hs.recipe("nan40")
    nwords, _ = _words("nan40")
    nargs = types.SimpleNamespace(num_categories=n.C, num_users=n.U, embed_size=n.E, high_level_score_coefficient=n.coef)
    nmodel = foodrec_amd.Model(nargs, n.PM, n.RE, n.CE, None, device=torch.device("cuda", 0))
    nmodel.set_mlp_head(*n.head)
    nd2c = {str(d): n.cats[d].tolist() for d in range(n.I)}
    nusers = n.users.tolist()
    ntest = {str(u): [int(rng.integers(0, n.I))] for u in nusers}
    nnegs = {str(u): [int(d) for d in rng.integers(0, n.I, 100)] for u in nusers}
    calls = []
    inner = nmodel.predict_extended
    nmodel.predict_extended = lambda *a, **kw: (calls.append(kw.get("head")), inner(*a, **kw))[1]
    hn, nn = foodrec_amd.evaluate_model(None, nmodel, ntest, nnegs, K, nd2c, head=True)
    assert calls == [True] * len(nusers), calls
    import heapq
    for u in nusers:
        items = [ntest[str(u)][0]] + nnegs[str(u)][50:100]
        assert np.isnan(nwords[u][items]).any()
        table = {}
        for it in items:
            table[it] = nwords[u][it]
        lst = heapq.nlargest(K, table, key=table.get)
        assert hn[u] == foodrec_amd.getHitRatio(lst, items[0]) and nn[u] == foodrec_amd.getNDCG(lst, items[0]), u
