"""GPU tests of menu retrieval (m2d_topk_menu; build-defined, no reference counterpart): the lists against the
restatement (tests/menu_cases.py) applied to the engine's OWN m2d_score_slate words over arange(I), uncapped calls against
m2d_topk_users_deep, independence from the launcher's cut, state changes, errors and refusals, the neighbouring calls, the Python
surface.  No comparison has a tolerance: ids as integers, scores as 32-bit words.  The calls go through the C ABI into poisoned buffers
with a guard row on either side.  The conditions the cases rely on are asserted in tests/test_menu_cases_cpu.py on host scores and
again here, where a case depends on them, on the engine's words."""
import ctypes

import numpy as np
import pytest

import deep_cases as dc
import menu_cases as mc

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN no kernel computes; as an id: no dish


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _engine(r, user_base=0, masks=True, tables=None):
    from foodrec_amd import ScoringEngine
    PM, RE, CE = tables if tables is not None else (r.PM, r.RE, r.CE)
    eng = ScoringEngine(PM, RE, CE, coef=r.coef, user_base=user_base)
    if masks:
        eng.set_dish_categories(r.cats)
    return eng


def eng_error(eng):
    from foodrec_amd import _native
    return (_native.lib().m2d_last_error(eng._h) or b"").decode()


def _latched(eng):
    """(code, value, index) of m2d_check"""
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    bv, bi = ctypes.c_int64(), ctypes.c_int64()
    rc = _native.lib().m2d_check(eng._h, _stream_ptr(), ctypes.byref(bv), ctypes.byref(bi))
    return rc, bv.value, bi.value


def _abi(eng, users, caps, k, null=()):
    """One m2d_topk_menu call through the C ABI -> (status, score words uint32 [nU, k], ids int64 [nU, k]); the guard rows are checked."""
    import torch
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    users = np.asarray(users, np.int32)
    nU = len(users)
    caps = np.ascontiguousarray(np.broadcast_to(np.asarray(caps, np.int32), (nU, eng.C)))
    ut = _dev(users if nU else np.zeros(1, np.int32))
    ct = _dev(caps.reshape(-1) if nU else np.zeros(1, np.int32))
    kk = max(int(k), 1)
    bs = torch.full(((nU + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    bi = torch.full(((nU + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    ptr = lambda t, name, shift=0: None if name in null else t.data_ptr() + shift      # noqa: E731
    rc = _native.lib().m2d_topk_menu(eng._h, ptr(ut, "users"), nU, int(k), ptr(ct, "caps"), ptr(bs, "scores", 4 * kk),
                                     ptr(bi, "out_ids", 4 * kk), _stream_ptr())
    torch.cuda.synchronize()
    s, i = bs.cpu().numpy().view(np.uint32).reshape(nU + 2, kk), bi.cpu().numpy().reshape(nU + 2, kk)
    assert (s[[0, -1]] == POISON).all() and (i[[0, -1]] == POISON).all(), "a guard row was written"
    return rc, s[1:-1], i[1:-1].astype(np.int64)


def _menu(eng, users, caps, k):
    """the lists of a call that must succeed: every element written, the id latch clear"""
    rc, s, i = _abi(eng, users, caps, k)
    assert rc == 0, eng_error(eng)
    eng.check()
    assert (i != POISON).all() and (s != POISON).all(), "%d elements not written" % int((i == POISON).sum())
    return s, i


def _matrix(eng, U, user_base=0):
    """the engine's own m2d_score_slate words of every user for every dish: float32 [U, I]"""
    out = eng.score_slate(_dev(np.arange(U, dtype=np.int32) + user_base), _dev(np.arange(eng.I, dtype=np.int32)))
    eng.check()
    return out.cpu().numpy()


def _same(got, want, what=""):
    assert np.array_equal(np.asarray(got[1], np.int64), np.asarray(want[1], np.int64)), "%s: ids of %d rows differ" % (
        what, int((np.asarray(got[1]) != np.asarray(want[1])).any(1).sum()))
    assert np.array_equal(np.asarray(got[0], np.uint32), np.asarray(want[0], np.uint32)), "%s: score words differ" % what


def _t(x):
    s, i = x
    return dc.words(s.cpu().numpy()), i.cpu().numpy().astype(np.int64)


def _all_cap_sets(eng, r, S, users, k, what, must_change=True):
    """every cap set of menu_cases.CAP_SETS at k against the restatement over the engine's words; -> a row ended short somewhere"""
    W32 = S[np.asarray(users)]
    n, C = len(users), r.cats.shape[1]
    free = dc.key_lists(W32, k)
    busy = mc.busiest(W32, r.cats, k)
    short = False
    for name in mc.CAP_SETS:
        caps = mc.cap_set(name, n, C, k, busy)
        want = mc.menu_lists(W32, r.cats, caps, k)
        _same(_menu(eng, users, caps, k), want, "%s, caps %s, k = %d" % (what, name, k))
        if must_change:
            assert mc.changed_rows(want, free).mean() >= 0.5, (what, name)
        short |= bool(mc.short_rows(want).any())
    return short


# ---- 1. uncapped calls are the deep lists ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", ("exact4", "normal6"))
def test_caps_of_k_and_more_give_topk_users_deeps_lists(recipe):
    r = mc.exact_recipe(4, 64, 1300) if recipe == "exact4" else mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    users = r.users
    for k in (1, 10, 64):
        deep = _t(eng.topk_users_deep(_dev(users), k))
        eng.check()
        _same(deep, dc.key_lists(S[users], k), "topk_users_deep against the key rule")
        for caps in (mc.caps_uncapped(len(users), r.C, k), mc.caps_uncapped(len(users), r.C, k, 1), np.full(r.C, 2 ** 31 - 1, np.int32)):
            _same(_menu(eng, users, caps, k), deep, "caps >= k, k = %d" % k)
    eng.close()


# ---- 2. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,E,I", ((4, 64, 255), (4, 64, 256), (4, 64, 257), (4, 64, 1300), (6, 64, 16385), (3, 64, 257), (5, 64, 1300),
                                   (6, 64, 1300), (4, 4, 257), (4, 200, 257), (6, 200, 1300), (3, 4, 1300)))
def test_capped_lists_at_every_shape(C, E, I):
    """exact tables where every signature's division is exact (C = 3, 4, 5), normal tables with all 2^C signatures at C = 6; every cap
    set at k = 10, the per-user caps at k = 64 and k = 1; rows that end short; empty-mask dishes in the tail"""
    r = mc.normal_recipe(C, E, I) if C == 6 else mc.exact_recipe(C, E, I)
    if C == 6:
        assert len(set(r.sig.tolist())) == 64
    eng = _engine(r)
    S = _matrix(eng, r.U)
    assert np.isnan(S[:, r.sig == 0]).all() and not np.isnan(S[:, r.sig != 0]).any()
    assert _all_cap_sets(eng, r, S, r.users, 10, "C %d E %d I %d" % (C, E, I)), "no row ended short"
    n = len(r.users)
    for k in (1, 64):
        caps = mc.caps_mixed(n, C, seed=k, hi=5)
        _same(_menu(eng, r.users, caps, k), mc.menu_lists(S[r.users], r.cats, caps, k), "per-user caps, k = %d" % k)
    # caps exhausted: the empty-mask dishes fill the tail in id order, then the row ends
    s, i = _menu(eng, r.users, mc.caps_all(n, C, 1), 64)
    empty = np.flatnonzero(r.sig == 0)
    for row in i:
        real = row[row >= 0]
        assert real[-len(empty):].tolist() == empty.tolist() and len(real) <= C + len(empty) < 64
    eng.close()


def test_segments_of_0_1_63_64_65_dishes_and_one_signature_for_all():
    r = mc.segment_recipe()
    sizes = np.bincount(r.sig, minlength=16)
    assert all(sizes[s] == n for s, n in mc.SEGMENT_SIZES.items())
    eng = _engine(r)
    S = _matrix(eng, r.U)
    for k in (10, 64):
        _all_cap_sets(eng, r, S, r.users, k, "segment sizes", must_change=k == 10)
    caps = np.asarray([1, 64, 64, 0], np.int32)              # signature 1 = {0}: its one dish; 2 = {1}: 63 dishes and no more
    _same(_menu(eng, r.users, caps, 64), mc.menu_lists(S[r.users], r.cats, caps, 64), "the small segments alone")
    eng.close()
    r = mc.one_signature_recipe()
    eng = _engine(r)
    S = _matrix(eng, r.U)
    for P in (256, dc.DEFAULT_P):
        eng.set_option("deep_chunk_pairs", P)
        for caps in ((64, 64, 64, 64), (7, 0, 64, 0), (64, 64, 3, 64), (0, 1, 1, 1)):
            want = mc.menu_lists(S[r.users], r.cats, np.asarray(caps), 64)
            assert (want[1] >= 0).sum(1).tolist() == [min(caps[0], caps[2], 64)] * r.U       # every dish is {0, 2}
            _same(_menu(eng, r.users, np.asarray(caps, np.int32), 64), want, "one signature, caps %s" % (caps,))
    eng.close()


# ---- 3. mask forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("weighted", "negative", "minus_zero"))
def test_weighted_negative_and_minus_zero_masks(form):
    r = mc.normal_recipe(6, 64, 1300, form=form)
    if form == "minus_zero":
        assert (np.signbit(r.cats) & (r.cats == 0)).sum() > r.I
    if form == "negative":
        assert (r.cats < 0).sum() > r.I // 4
    eng = _engine(r)
    S = _matrix(eng, r.U)
    _all_cap_sets(eng, r, S, r.users, 10, form)
    if form == "minus_zero":                                  # -0.0 counted as a member would give other lists
        caps = mc.caps_all(len(r.users), 6, 1)
        assert not dc.same(mc.menu_lists(S[r.users], r.cats, caps, 10), mc.menu_lists(S[r.users], r.cats, caps, 10, "minus_zero_member"))
    eng.close()


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", mc.TIE_GROUPS)
def test_tie_groups_across_segments_and_across_position_k(group):
    r = mc.tie_recipe(group)
    eng = _engine(r)
    S = _matrix(eng, r.U)
    w = dc.words(S)
    assert (w[:, r.copies] == w[:, r.copies[:1]]).all() and sorted(set(r.sig[r.copies])) == [1, 2]       # bit-equal words, two segments
    assert (w[r.U - 1][r.sig != 0] << 1 == 0).all()                                                      # the all-zero user
    for j, u in enumerate(r.users):
        k = r.k[j]
        for caps in (mc.caps_uncapped(1, 4, k), mc.caps_all(1, 4, max(k // 2, 1)), np.asarray([[k, 1, k, k]], np.int32)):
            want = mc.menu_lists(S[u:u + 1], r.cats, caps, k)
            _same(_menu(eng, [u], caps, k), want, "group %d, user %d" % (group, u))
        free = mc.menu_lists(S[u:u + 1], r.cats, mc.caps_uncapped(1, 4, k), k)
        assert not dc.same(free, mc.menu_lists(S[u:u + 1], r.cats, mc.caps_uncapped(1, 4, k), k, "higher_id")), (group, u)
    ks = [10] * len(r.users)                                  # one call for all of them, the zero user in the middle of the block
    users = np.concatenate([r.users[-1:], r.users, r.users[-1:]])
    for caps in (mc.caps_all(len(users), 4, 2), mc.caps_mixed(len(users), 4)):
        _same(_menu(eng, users, caps, ks[0]), mc.menu_lists(S[users], r.cats, caps, ks[0]), "group %d, one call" % group)
    eng.close()


# ---- 5. the launcher's cut ----------------------------------------------------------------------------------------------------------------
def test_lists_do_not_depend_on_the_launchers_cut():
    """deep_chunk_pairs 256 (ranges of 256 dishes, blocks of one user), 2 048 (blocks of 8 users: 11 rows end in a partial block) and the
    default, both selections, nU = 1: the same words, with best dishes planted on both sides of every range and segment edge"""
    r = mc.edge_recipe()
    eng = _engine(r)
    S = _matrix(eng, r.U)
    n = len(r.users)
    cases = [(mc.caps_uncapped(n, 4, 64), 64), (mc.caps_all(n, 4, 2), 10), (mc.caps_mixed(n, 4), 10), (mc.caps_mixed(n, 4, hi=9), 64)]
    want = [mc.menu_lists(S[r.users], r.cats, caps, k) for caps, k in cases]
    assert mc.edge_condition(want[0][1], r)
    for P in (256, 2048, dc.DEFAULT_P):
        eng.set_option("deep_chunk_pairs", P)
        for select in (0, 1):
            eng.set_option("menu_select", select)
            for (caps, k), w in zip(cases, want):
                _same(_menu(eng, r.users, caps, k), w, "P = %d, menu_select = %d, k = %d" % (P, select, k))
        eng.set_option("menu_select", 0)
        for j in (0, n - 1):                                  # nU = 1
            caps, k = cases[2]
            _same(_menu(eng, r.users[j:j + 1], caps[j:j + 1], k), (want[2][0][j:j + 1], want[2][1][j:j + 1]), "nU = 1, P = %d" % P)
    users = np.tile(r.users, 28)[:300]                        # 300 rows: three user tiles of the score kernel, the last one partial
    caps = mc.caps_mixed(300, 4, seed=3)
    want300 = mc.menu_lists(S[users], r.cats, caps, 10)
    for P in (1 << 15, dc.DEFAULT_P):                         # blocks of 56 users (the last: 20), and one block of 300
        eng.set_option("deep_chunk_pairs", P)
        _same(_menu(eng, users, caps, 10), want300, "300 users, P = %d" % P)
    eng.close()


# ---- 6. state changes -----------------------------------------------------------------------------------------------------------------------
def test_a_user_base_shard_and_repeated_users_with_different_caps():
    r = mc.normal_recipe(6, 64, 1300)
    base = 1000
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, user_base=base)
    users = np.asarray([3, 3, 3, 0, 7, 3, 0], np.int32)
    caps = mc.caps_mixed(len(users), 6, seed=4)
    assert len({tuple(c) for c in caps[users == 3]}) > 1
    want = mc.menu_lists(S[users], r.cats, caps, 10)
    assert len({tuple(row) for row in want[1][users == 3]}) > 1
    _same(_menu(eng, users + base, caps, 10), want, "a shard")
    eng.close()


def test_lists_follow_write_memory_tables_updated_and_new_masks():
    import torch
    b = dc.normal_recipe(64, I=500, U=16, seed=2, head=False)
    rng = np.random.default_rng(8)
    eng = _engine(b, tables=(b.PM.copy(), b.RE.copy(), b.CE.copy()))
    users = np.arange(b.U, dtype=np.int32)
    caps = mc.caps_all(b.U, 4, 2)
    t = lambda a: torch.as_tensor(a, device="cuda")         # noqa: E731
    cats = [b.cats]

    def check(before, what):
        now = _menu(eng, users, caps, 10)
        assert before is None or not dc.same(before, now), what + " changed nothing"
        _same(now, mc.menu_lists(_matrix(eng, b.U), cats[0], caps, 10), what)
        return now

    state = check(None, "at the start")
    B, L = 400, 7
    wu = (np.arange(B) % b.U).astype(np.int32)
    wi = rng.choice(np.flatnonzero(b.cats.sum(1) > 0), B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, b.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(b.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    state = check(state, "write_memory")
    eng.re[:50] *= 1.5
    eng.tables_updated()
    state = check(state, "tables_updated")
    cats[0] = np.roll(b.cats, 1, axis=1)                     # other signatures for the same dishes: the index is rebuilt
    assert (mc.signatures(cats[0]) != mc.signatures(b.cats)).mean() > 0.5
    eng.set_dish_categories(cats[0])
    state = check(state, "a second set_dish_categories")
    cats[0] = b.cats
    eng.set_dish_categories(cats[0])
    check(state, "the first masks again")
    eng.close()


def test_inputs_that_arrive_late_on_a_side_stream():
    """Stream order: on a side stream a blocker (matrix products), then the copies that put the real users and caps where a decoy
    request stood, then the call -- entered while the blocker runs.  The lists are the real request's, on an engine whose first menu
    call this is (the index build may wait for that stream) and again on the warmed engine (no build in front of the launches)."""
    import torch
    r = mc.normal_recipe(6, 64, 1300)
    eng = _engine(r)
    n = len(r.users)
    real = (r.users, mc.caps_mixed(n, 6, seed=5))
    decoy = (np.roll(r.users, 3), mc.caps_mixed(n, 6, seed=6))
    twin = _engine(r)
    want, other = _menu(twin, *real, 10), _menu(twin, *decoy, 10)
    twin.close()
    assert mc.changed_rows(want, other).mean() >= 0.9       # the decoy's answer is another one
    a = torch.randn((8192, 8192), device="cuda")
    S = torch.cuda.Stream()
    src = [_dev(x) for x in real]
    for episode in ("first use", "warmed"):
        bufs = [_dev(x) for x in decoy]
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            for _ in range(6):
                a @ a
            for b, s in zip(bufs, src):
                b.copy_(s, non_blocking=True)
            arrived = torch.cuda.Event()
            arrived.record(S)
            late = not arrived.query()                        # the copies had not landed when the call was made
            got = torch.ops.m2d.topk_menu(eng.id, bufs[0], bufs[1], 10)
            S.synchronize()
            eng.check()
        assert late, "the blocker was too short to show anything"
        _same(_t(got), want, "side stream, " + episode)
    eng.close()


# ---- 7. errors and refusals ------------------------------------------------------------------------------------------------------------------
def test_bad_users_and_negative_caps_are_latched_with_value_and_position():
    from foodrec_amd import _native
    r = mc.normal_recipe(6, 64, 1300)
    base = 100
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, user_base=base)
    users = r.users + base
    n = len(users)
    caps = mc.caps_mixed(n, 6, seed=2)
    want = mc.menu_lists(S[r.users], r.cats, caps, 10)
    _same(_menu(eng, users, caps, 10), want)
    for P in (dc.DEFAULT_P, 256):                            # 256: blocks of one user -- the position is the caller's
        eng.set_option("deep_chunk_pairs", P)
        for row in (0, n // 2, n - 1):
            for value in (base + r.U, base - 1, -1):
                u = users.copy(); u[row] = value
                rc, s, i = _abi(eng, u, caps, 10)
                assert rc == 0 and _latched(eng) == (_native.M2D_ERR_BAD_USER_ID, value, row), (P, row, eng_error(eng))
                assert _latched(eng)[0] == 0                 # cleared; the engine is usable
                ok = np.setdiff1d(np.arange(n), [row])
                _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), "the other users' rows")
            for c, value in ((0, -1), (5, -7), (2, -(2 ** 31))):
                bad = caps.copy(); bad[row, c] = value
                rc, s, i = _abi(eng, users, bad, 10)
                assert rc == 0 and _latched(eng) == (_native.M2D_ERR_INVALID_ARG, value, row * 6 + c), (P, row, c, eng_error(eng))
                assert "m2d_topk_menu: a cap below 0" in eng_error(eng)
                ok = np.setdiff1d(np.arange(n), [row])
                _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), "the other users' rows")
            _same(_menu(eng, users, caps, 10), want, "after a latched error")
    eng.close()


def test_argument_errors():
    from foodrec_amd import _native
    r = mc.exact_recipe(4, 64, 257)
    eng = _engine(r)
    caps = mc.caps_all(len(r.users), 4, 2)
    bad = _native.M2D_ERR_INVALID_ARG
    for k in (0, 65, -3, 1024):
        assert _abi(eng, r.users, caps, k)[0] == bad and "m2d_topk_menu: need nU >= 0 and 1 <= k <= min(64, I)" in eng_error(eng)
    for null in ("users", "caps", "scores", "out_ids"):
        assert _abi(eng, r.users, caps, 5, null=(null,))[0] == bad and eng_error(eng) == "m2d_topk_menu: null buffer"
    assert _abi(eng, np.zeros(0, np.int32), caps[:0], 5)[0] == 0 and _latched(eng)[0] == 0      # nU == 0: nothing is launched
    eng.close()
    bare = _engine(r, masks=False)
    assert _abi(bare, r.users, caps, 5)[0] == _native.M2D_ERR_NOT_CONFIGURED
    bare.close()
    small = mc.exact_recipe(4, 64, 40)                       # k above I
    eng = _engine(small)
    assert _abi(eng, small.users, mc.caps_all(len(small.users), 4, 2), 41)[0] == bad
    S = _matrix(eng, small.U)
    c40 = mc.caps_uncapped(len(small.users), 4, 40)
    _same(_menu(eng, small.users, c40, 40), mc.menu_lists(S[small.users], small.cats, c40, 40), "k = I")
    eng.close()


def test_refusals_name_the_call():
    from foodrec_amd import _native
    from helpers import mlp_head
    rng = np.random.default_rng(2)
    r7 = mc.normal_recipe(7, 64, 300)
    eng = _engine(r7)
    assert _abi(eng, r7.users, mc.caps_all(len(r7.users), 7, 2), 5)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng).startswith("m2d_topk_menu: more than 6 categories")
    eng.close()
    r = dc.normal_recipe(64, I=300, U=8, seed=1, head=False)
    eng = _engine(r)
    users = np.arange(r.U, dtype=np.int32)
    caps = mc.caps_all(r.U, 4, 2)
    want = _menu(eng, users, caps, 10)
    nnz = 3 * r.I
    eng.set_ingredients((rng.standard_normal((50, r.E)) / 8).astype(np.float32), np.arange(0, nnz + 1, 3, dtype=np.int32),
                        rng.integers(0, 50, nnz).astype(np.int32))
    assert _abi(eng, users, caps, 10)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng) == "m2d_topk_menu: the ingredient table is set (not supported)"
    eng.clear_ingredients()
    _same(_menu(eng, users, caps, 10), want, "after clear_ingredients")
    keep = eng.re[7, 3].item()
    eng.re[7, 3] = float("inf")
    eng.tables_updated()
    assert _abi(eng, users, caps, 10)[0] == _native.M2D_ERR_UNSUPPORTED
    assert eng_error(eng) == "m2d_topk_menu: needs finite tables (a table value is not finite)"
    eng.re[7, 3] = keep
    eng.tables_updated()
    _same(_menu(eng, users, caps, 10), want, "after the value was put back")
    eng.set_mlp_head(*mlp_head(5 * r.E, 256, 64, rng, scale=4.0))                    # an MLP head is ignored
    _same(_menu(eng, users, caps, 10), want, "under an MLP head")
    eng.close()


# ---- 8. the neighbouring calls ----------------------------------------------------------------------------------------------------------------
def test_existing_calls_are_what_they_were_around_menu_calls():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, head=False)
    users = _dev(r.users)
    pu, pi = _dev(np.repeat(r.users, 20)), _dev(np.tile(np.arange(20, dtype=np.int32) * 7, len(r.users)))
    eng = _engine(r)

    def existing():
        out = [_t(eng.topk_users(users, 10)), _t(eng.topk_users_deep(users, 300)),
               (dc.words(eng.score_pairs_bydish(pu, pi).cpu().numpy()), np.zeros(1))]
        eng.check()
        return out

    before = existing()
    n = len(r.users)
    for caps, k in ((mc.caps_all(n, 4, 1), 10), (mc.caps_mixed(n, 4), 64)):
        _menu(eng, r.users, caps, k)
    assert _abi(eng, r.users, mc.caps_all(n, 4, 1), 65)[0] == _native.M2D_ERR_INVALID_ARG          # a refused call
    bad = r.users.copy(); bad[3] = r.U                                                             # two failed ones
    assert _abi(eng, bad, mc.caps_all(n, 4, 1), 10)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_USER_ID
    assert _abi(eng, r.users, mc.caps_all(n, 4, -1), 10)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_INVALID_ARG
    for a, b in zip(before, existing()):
        _same(a, b, "an existing call moved")
    eng.close()


# ---- 9. the Python surface ----------------------------------------------------------------------------------------------------------------------
def test_torch_op_and_the_model():
    import types
    import torch
    import foodrec_amd
    r = dc.normal_recipe(64, head=False)
    eng = _engine(r)
    n = len(r.users)
    caps = mc.caps_mixed(n, 4)
    want = _menu(eng, r.users, caps, 10)
    _same(_t(torch.ops.m2d.topk_menu(eng.id, _dev(r.users), _dev(caps), 10)), want, "torch.ops.m2d.topk_menu")
    one = np.asarray([2, 0, 1, 3], np.int32)                  # a single row is broadcast
    _same(_t(torch.ops.m2d.topk_menu(eng.id, _dev(r.users), _dev(one), 12)), _menu(eng, r.users, np.tile(one, (n, 1)), 12), "caps [C]")
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        eng._topk_menu(_dev(r.users), 65, _dev(one))
    with pytest.raises(ValueError, match="caps must be"):
        eng._topk_menu(_dev(r.users), 5, _dev(caps[:3]))
    with pytest.raises(TypeError):
        eng._topk_menu(_dev(r.users), 5, _dev(caps.astype(np.int64)))
    eng.close()

    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    ids = [str(u) for u in r.users]                          # ids as the reference feeds them: str
    s, i = model.topk_menu(ids)
    assert s.shape == i.shape == (n, 10) and s.dtype == np.float32 and i.dtype == np.int32
    _same((dc.words(s), i), _t(model.engine.topk_users_deep(_dev(r.users), 10)), "Model.topk_menu, uncapped")
    s, i = model.topk_menu(ids, 12, {1: 2, 3: 0})
    _same((dc.words(s), i), _menu(model.engine, r.users, np.tile(np.asarray([12, 2, 12, 0], np.int32), (n, 1)), 12), "Model.topk_menu, a dict")
    s, i = model.topk_menu(ids, 7, [1, 2, 3, 0])
    _same((dc.words(s), i), _menu(model.engine, r.users, np.tile(np.asarray([1, 2, 3, 0], np.int32), (n, 1)), 7), "Model.topk_menu, a list")
    per_user = [{0: j % 3} if j % 2 else [int(c) for c in caps[j]] for j in range(n)]
    table = np.asarray([[j % 3, 9, 9, 9] if j % 2 else caps[j] for j in range(n)], np.int32)
    s, i = model.topk_menu(ids, 9, per_user)
    _same((dc.words(s), i), _menu(model.engine, r.users, table, 9), "Model.topk_menu, per-user caps")
    for kw in (dict(k=65), dict(caps=[1, 2, 3]), dict(caps={4: 1}), dict(caps=[-1, 1, 1, 1]), dict(caps=per_user[:3])):
        with pytest.raises(ValueError):
            model.topk_menu(ids, **kw)
