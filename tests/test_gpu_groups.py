"""GPU tests of household retrieval (m2d_topk_groups, m2d_score_groups_slate, m2d_topk_groups_slate; DESIGN.md section 4.12;
build-defined, no reference counterpart): the group words against the restatement applied to the engine's OWN m2d_score_slate words,
the lists against the key rule over the restated words, groups of one against the calls that exist, independence from the launcher's
cut, exclusions, a shard, writers, the Python surface, errors and refusals.  No comparison has a tolerance: ids as integers, scores
as 32-bit words -- except that a MEAN word that is a NaN is compared as a NaN (its payload is the adder's own).  The calls go through
the C ABI into poisoned buffers with a guard row on either side.  Inputs, restatement and stand-ins: tests/group_cases.py (the
conditions the cases rely on are asserted in tests/test_group_cases_cpu.py)."""
import ctypes

import numpy as np
import pytest

import deep_cases as dc
import group_cases as gc

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN no kernel computes; as an id: no dish
ALL_MODES = (gc.LEAST, gc.MEAN, gc.MOST)


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


def _abi(eng, members, mode, k=None, slate=None, off=None, ids=None, null=(), M=None):
    """One call through the C ABI.  k None: m2d_score_groups_slate -> (status, words uint32 [nG, nD]); otherwise m2d_topk_groups
    (slate None) or m2d_topk_groups_slate -> (status, score words uint32 [nG, k], ids int64 [nG, k]).  The guard rows are checked."""
    import torch
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    members = np.asarray(members, np.int32)
    nG, M = members.shape[0], members.shape[1] if M is None else M
    mt = _dev(members.reshape(-1) if members.size else np.zeros(1, np.int32))
    st = _dev(np.asarray(slate, np.int32)) if slate is not None else None
    nD = 0 if slate is None else len(slate)
    xo = _dev(np.asarray(off, np.int64)) if off is not None else None
    xi = _dev(np.asarray(ids, np.int32)) if ids is not None else None
    ptr = lambda t, name, shift=0: None if t is None or name in null else t.data_ptr() + shift      # noqa: E731
    lib = _native.lib()
    if k is None:
        width = max(nD, 1)
        buf = torch.full(((nG + 2) * width,), POISON, dtype=torch.int32, device="cuda")
        rc = lib.m2d_score_groups_slate(eng._h, ptr(mt, "members"), nG, M, mode, ptr(st, "slate"), nD, ptr(buf, "out", 4 * width), _stream_ptr())
        torch.cuda.synchronize()
        w = buf.cpu().numpy().view(np.uint32).reshape(nG + 2, width)
        assert (w[[0, -1]] == POISON).all(), "a guard row was written"
        return rc, w[1:-1]
    kk = max(int(k), 1)
    bs = torch.full(((nG + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    bi = torch.full(((nG + 2) * kk,), POISON, dtype=torch.int32, device="cuda")
    if slate is None:
        rc = lib.m2d_topk_groups(eng._h, ptr(mt, "members"), nG, M, mode, int(k), ptr(xo, "off"), ptr(xi, "ids"), ptr(bs, "scores", 4 * kk),
                                 ptr(bi, "out_ids", 4 * kk), _stream_ptr())
    else:
        rc = lib.m2d_topk_groups_slate(eng._h, ptr(mt, "members"), nG, M, mode, ptr(st, "slate"), nD, int(k), ptr(bs, "scores", 4 * kk),
                                       ptr(bi, "out_ids", 4 * kk), _stream_ptr())
    torch.cuda.synchronize()
    s, i = bs.cpu().numpy().view(np.uint32).reshape(nG + 2, kk), bi.cpu().numpy().reshape(nG + 2, kk)
    assert (s[[0, -1]] == POISON).all() and (i[[0, -1]] == POISON).all(), "a guard row was written"
    return rc, s[1:-1], i[1:-1].astype(np.int64)


def _words(eng, members, mode, slate):
    rc, w = _abi(eng, members, mode, None, slate)
    assert rc == 0, eng_error(eng)
    eng.check()
    assert (w != POISON).all(), "%d words not written" % int((w == POISON).sum())
    return w


def _lists(eng, members, mode, k, lists=None, slate=None):
    """the lists of a call that must succeed: every element written, the id latch clear"""
    off, ids = dc.csr(lists) if lists is not None else (None, None)
    rc, s, i = _abi(eng, members, mode, k, slate, off, ids)
    assert rc == 0, eng_error(eng)
    eng.check()
    assert (i != POISON).all() and (s != POISON).all(), "%d elements not written" % int((i == POISON).sum())
    return s, i


def _matrix(eng, U, slate, user_base=0):
    """the engine's own m2d_score_slate words of every user for the slate: float32 [U, nD]"""
    out = eng.score_slate(_dev(np.arange(U, dtype=np.int32) + user_base), _dev(np.asarray(slate, np.int32)))
    eng.check()
    return out.cpu().numpy()


def _same(got, want, mode, what=""):
    gs, gi = got
    ws, wi = want
    assert np.array_equal(np.asarray(gi, np.int64), np.asarray(wi, np.int64)), "%s: ids of %d rows differ" % (
        what, int((np.asarray(gi) != np.asarray(wi)).any(1).sum()))
    assert gc.same_words(gs, ws, mode), "%s: score words differ" % what


def _t(x):
    s, i = x
    return dc.words(s.cpu().numpy()), i.cpu().numpy().astype(np.int64)


# ---- 1. the reduction words ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables,E", (("exact", 4), ("exact", 64), ("exact", 200), ("normal", 64)))
def test_group_words_equal_the_restatement_over_the_engines_words(tables, E):
    """m2d_score_groups_slate at M = 1 / 2 / 3 / 8 / 64 with every count from 1 to M in a call, slates of 1 ... 1 300 dishes (the 16-byte
    and the scalar path of m2d_group_reduce, its tail, the slate kernel's TN switch), blocks that end in a partial one
    (deep_chunk_pairs = 2 048) and a call of one group; repeated members, an all-zero member (equal words), a NaN column."""
    r = gc.words_recipe(tables, E)
    eng = _engine(r)
    eng.set_option("deep_chunk_pairs", 2048)
    full = _matrix(eng, r.U, np.arange(r.I))
    assert np.isnan(full[:, 5]).all() and (dc.words(full[1])[~np.isnan(full[1])] == 0).all()
    for nD in gc.SLATE_SIZES:
        slate = gc.slate_of(r.I, nD)
        S = _matrix(eng, r.U, slate)
        assert np.array_equal(dc.words(S), dc.words(full[:, slate]))          # a member word does not depend on the slate around it
        for M in gc.MEMBER_COUNTS:
            members = gc.member_matrix(r.U, gc.words_groups(M), M)
            for mode in ALL_MODES:
                got = _words(eng, members, mode, slate)
                assert gc.same_words(got, gc.group_words(S, members, mode), mode), (tables, E, M, nD, mode)
            one = members[M - 1:M]                                             # nG = 1: the group with M members
            assert gc.same_words(_words(eng, one, gc.LEAST, slate), gc.group_words(S, one, gc.LEAST), gc.LEAST), (M, nD)
    eng.close()


@pytest.mark.parametrize("variant", (0, 9))
def test_zeros_of_both_signs_and_infinities_in_the_engines_own_words(variant):
    """Finite tables whose m2d_score_slate words hold -0, +0, -inf and +inf (group_cases.sign_recipe), on the MFMA kernel and on the
    generic one ("variant" = 9): -0 against +0 in both member orders -- equal under the key, the FIRST member's word is returned, which
    is where a reduce that resolves ties to the last member shows --, infinities against finite words, all three modes, words and lists."""
    r = gc.sign_recipe()
    eng = _engine(r)
    eng.set_option("variant", variant)
    slate = np.arange(r.I)
    S = _matrix(eng, r.U, slate)
    assert eng.last_kernel() == ("m2d_score_slate_generic" if variant == 9 else "m2d_score_slate_mfma")
    w, u = dc.words(S), gc.SIGN_USERS
    NZ, PINF, NINF = 0x80000000, 0x7F800000, 0xFF800000
    assert (w[u["neg"], :4] == NZ).all() and (w[u["pos"], :4] == 0).all() and (w[u["zero"]] == 0).all()      # what the case relies on
    assert (w[u["huge"], 4:6] == NINF).all() and (w[u["huge"], 6:] == PINF).all() and not np.isnan(S).any()
    if variant == 9:
        assert np.array_equal(w, dc.words(r.S))              # fmaf in increasing k: the host chain, word for word
    members = gc.sign_members()
    assert members[0].tolist()[:2] == [u["neg"], u["pos"]] and members[1].tolist()[:2] == [u["pos"], u["neg"]]
    for mode in ALL_MODES:
        got = _words(eng, members, mode, slate)
        assert gc.same_words(got, gc.group_words(S, members, mode), mode), (variant, mode)
        if mode != gc.MEAN:
            assert (got[0, :4] == NZ).all() and (got[1, :4] == 0).all()                  # equal under the key: the first member's word
            assert not gc.same_words(got, gc.group_words(S, members, mode, standin="last_tie"), mode)
        for k in (1, 8):
            _same(_lists(eng, members, mode, k), gc.group_lists(S, members, mode, k), mode, "variant %d, mode %d, k = %d" % (variant, mode, k))
    least, most = _words(eng, members, gc.LEAST, slate), _words(eng, members, gc.MOST, slate)
    assert (least[4, 4:6] == NINF).all() and (most[4, 6:] == PINF).all() and (least[4, 6:] == w[u["plain"], 6:]).all()
    eng.close()


@pytest.mark.parametrize("variant", (0, 9))
def test_a_nan_in_one_member_alone_is_worst_and_never_best(variant):
    """Finite tables the calls accept whose DISH VECTORS overflow (group_cases.nan_recipe): on the engine's own m2d_score_slate words
    one member is a NaN where others are +inf, -inf or finite.  LEAST returns the NaN (the first one in member order), MOST returns a
    NaN only where every member has one; a reduce that compares floats -- from +inf or from row 0 -- gives other words.  All three
    modes, words and lists, on the MFMA kernel and on the generic one."""
    r = gc.nan_recipe()
    eng = _engine(r)
    eng.set_option("variant", variant)
    slate = np.arange(r.I)
    S = _matrix(eng, r.U, slate)
    assert eng.last_kernel() == ("m2d_score_slate_generic" if variant == 9 else "m2d_score_slate_mfma")
    w, u, multi = dc.words(S), gc.NAN_USERS, list(gc.NAN_MULTI)
    PINF, NINF = 0x7F800000, 0xFF800000
    assert np.isnan(S[u["zero"], multi]).all() and np.isnan(S[u["opp"], multi]).all()            # what the case relies on:
    assert (w[u["plain"], multi] == PINF).all() and (w[u["plain2"], multi] == PINF).all() and (w[u["neg"], multi] == NINF).all()
    assert np.isfinite(S[:, 4:6]).all()                                                            # one member NaN, the others not
    assert np.array_equal(np.isnan(S), np.isnan(r.S))
    if variant == 9:
        assert np.array_equal(w[~np.isnan(S)], dc.words(r.S)[~np.isnan(r.S)])          # fmaf in increasing k: the host chain
    members = gc.nan_members()
    for mode in ALL_MODES:
        got = _words(eng, members, mode, slate)
        assert gc.same_words(got, gc.group_words(S, members, mode), mode), (variant, mode)
        for k in (1, 5, 8):
            _same(_lists(eng, members, mode, k), gc.group_lists(S, members, mode, k), mode, "variant %d, mode %d, k = %d" % (variant, mode, k))
    least, most = _words(eng, members, gc.LEAST, slate), _words(eng, members, gc.MOST, slate)
    for g in (0, 1, 2):                                      # plain | zero, zero | plain, neg | opp | plain
        assert np.isnan(least[g, multi].view(np.float32)).all() and (most[g, multi] == PINF).all(), g
    assert np.isnan(most[3, multi].view(np.float32)).all()  # zero | opp: every member a NaN
    assert (least[4, multi] == NINF).all() and (most[4, multi] == PINF).all()
    assert np.array_equal(least[0, multi], w[u["zero"], multi]) and np.array_equal(least[6, multi], w[u["opp"], multi])      # the first NaN member's word
    for mode, standins in ((gc.LEAST, ("float_least", "float_row0")), (gc.MOST, ("float_row0",))):
        got = least if mode == gc.LEAST else most
        for s in standins:
            assert not gc.same_words(got, gc.group_words(S, members, mode, standin=s), mode), (mode, s)
    eng.close()


# ---- 2. the lists ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", gc.LIST_SIZES)
def test_lists_on_exact_tables_follow_the_key_rule_over_the_group_words(I):
    r = dc.exact_recipe(64, I, U=3 if I > 2000 else 6)
    eng = _engine(r)
    S = _matrix(eng, r.U, np.arange(I))
    members = gc.list_members(r.U)
    slate = gc.slate_of(I, min(I, 1100))
    for mode in ALL_MODES:
        for k in gc.list_ks(I):
            _same(_lists(eng, members, mode, k), gc.group_lists(S, members, mode, k), mode, "I = %d, mode %d, k = %d" % (I, mode, k))
        for k in sorted({min(k, len(slate)) for k in (10, 65, 1024)}):
            w = gc.group_words(S[:, slate], members, mode).view(np.float32)
            _same(_lists(eng, members, mode, k, slate=slate), dc.key_lists(w, k, ids=slate), mode, "slate form, I = %d, k = %d" % (I, k))
    eng.close()


@pytest.mark.parametrize("E", (64, 200))
def test_lists_on_normal_tables(E):
    r = dc.normal_recipe(E, head=False)
    eng = _engine(r)
    S = _matrix(eng, r.U, np.arange(r.I))
    members = gc.list_members(r.U)
    for mode in ALL_MODES:
        for k in (10, 65, 1024):
            _same(_lists(eng, members, mode, k), gc.group_lists(S, members, mode, k), mode, "E = %d, mode %d, k = %d" % (E, mode, k))
    eng.close()


def test_a_group_of_one_is_the_single_user_call():
    r = dc.normal_recipe(64, head=False)
    eng = _engine(r)
    users = r.users
    slate = gc.slate_of(r.I, 300)
    for M in (1, 5):                                         # M = 5: one member and four fillers
        members = np.full((len(users), M), -1, np.int32)
        members[:, 0] = users
        for mode in ALL_MODES:
            for k in (10, 300, 1024):
                _same(_lists(eng, members, mode, k), _t(eng.topk_users_deep(_dev(users), k)), gc.LEAST, "topk_users_deep, k = %d" % k)
            for k in (1, 64):
                _same(_lists(eng, members, mode, k, slate=slate), _t(eng.topk_slate(_dev(users), _dev(slate), k)), gc.LEAST, "topk_slate, k = %d" % k)
    eng.check()
    eng.close()


# ---- 3. independence from the cut --------------------------------------------------------------------------------------------------------
def test_lists_do_not_depend_on_ranges_blocks_order_or_padding():
    r = dc.range_recipe("exact1300")                         # best dishes on both sides of every range edge
    eng = _engine(r)
    S = _matrix(eng, r.U, np.arange(r.I))
    members = gc.list_members(r.U)
    lists = dc.boundary_lists(r.I, dc.RANGE_W, len(members))[0]          # excluded ids on both sides of every edge too
    k = 1024
    rng = np.random.default_rng(4)
    perm = rng.permutation(len(members))
    m3 = gc.member_matrix(r.U, 9, 3, seed=5)
    m64 = np.full((9, 64), -1, np.int32)
    m64[:, :3] = m3
    for mode in ALL_MODES:
        want = None
        for P in (dc.DEFAULT_P, 2048, 256):                  # 256: ranges of 256 dishes (narrower than k), one group per block
            eng.set_option("deep_chunk_pairs", P)
            got = _lists(eng, members, mode, k, lists)
            if want is None:
                want = got
                _same(got, gc.group_lists(S, members, mode, k, lists), mode, "default ranges, mode %d" % mode)
                assert dc.boundary_condition(got[1], lists, r.edges)
            _same(got, want, gc.LEAST, "deep_chunk_pairs = %d, mode %d" % (P, mode))
            s, i = _lists(eng, members[perm], mode, k, [lists[j] for j in perm])
            _same((s, i), (want[0][perm], want[1][perm]), gc.LEAST, "groups permuted, P = %d" % P)
            _same(_lists(eng, m64, mode, 300), _lists(eng, m3, mode, 300), gc.LEAST, "M padded from 3 to 64, P = %d" % P)
            sl = gc.slate_of(r.I, 129)
            assert np.array_equal(_words(eng, m64, mode, sl), _words(eng, m3, mode, sl)), "M padded from 3 to 64 (words), P = %d" % P
    eng.close()


# ---- 4. exclusions -------------------------------------------------------------------------------------------------------------------------
def test_exclusion_segments_across_blocks_and_range_edges():
    r = dc.normal_recipe(64, head=False)
    eng = _engine(r)
    S = _matrix(eng, r.U, np.arange(r.I))
    members = gc.list_members(r.U, nG=16)
    for P in (256, dc.DEFAULT_P):                            # 256: sixteen blocks of one group, g0 = 0 .. 15
        eng.set_option("deep_chunk_pairs", P)
        for mode in ALL_MODES:
            lists = gc.exclusion_lists(r.I, len(members), gc.group_lists(S, members, mode, 2)[1])
            for k in (10, 300, 1024):
                want = gc.group_lists(S, members, mode, k, lists)
                _same(_lists(eng, members, mode, k, lists), want, mode, "P = %d, mode %d, k = %d" % (P, mode, k))
            assert not np.isin(want[1][2], lists[2]).any() and want[1][2][0] != gc.group_lists(S, members, mode, 1)[1][2][0]
    few = [list(range(r.I - 5))] + [[] for _ in range(len(members) - 1)]             # fewer than k left: -1 / NaN from column 5 on
    s, i = _lists(eng, members, gc.LEAST, 10, few)
    assert (i[0, :5] >= r.I - 5).all() and (i[0, 5:] == -1).all() and (s[0, 5:] == dc.NAN_WORD).all()
    eng.close()


# ---- 5. a shard, writers, the calls around ---------------------------------------------------------------------------------------------------
def test_a_user_base_shard():
    r = dc.normal_recipe(64, head=False)
    base = 9000
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, np.arange(r.I), user_base=base)
    members = gc.list_members(r.U, user_base=base)
    assert members.max() >= base and (members[members >= 0] >= base).all()
    for mode in ALL_MODES:
        _same(_lists(eng, members, mode, 100), gc.group_lists(S, members, mode, 100, user_base=base), mode, "shard, mode %d" % mode)
        sl = gc.slate_of(r.I, 65)
        assert gc.same_words(_words(eng, members, mode, sl), gc.group_words(S[:, sl], members, mode, user_base=base), mode)
    eng.close()


def test_lists_follow_writers():
    import torch
    r = dc.normal_recipe(64, I=500, U=16, seed=2, head=False)
    rng = np.random.default_rng(8)
    eng = _engine(r, tables=(r.PM.copy(), r.RE.copy(), r.CE.copy()))
    members = gc.list_members(r.U)
    t = lambda a: torch.as_tensor(a, device="cuda")         # noqa: E731

    def snapshot(e):
        return [_lists(e, members, mode, 200) for mode in ALL_MODES]

    def fresh():
        f = _engine(r, tables=(eng.pm.cpu().numpy(), eng.re.cpu().numpy(), eng.ce.cpu().numpy()))
        out = snapshot(f)
        f.close()
        return out

    def check(before, what):
        now = snapshot(eng)
        assert any(not dc.same(a, b) for a, b in zip(before, now)), what + " changed nothing"
        for a, b in zip(now, fresh()):
            _same(a, b, gc.LEAST, what)
        return now

    state = snapshot(eng)
    B, L = 400, 7
    wu = (np.arange(B) % r.U).astype(np.int32)
    wi = rng.choice(np.flatnonzero(r.cats.sum(1) > 0), B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, 5, r.E)) / 4).astype(np.float32))
    eng.write_memory(t(wu), t(wi), t(r.cats[wi]), t(sign), t(y), gm, 1.0, 1.0, 0.5); eng.check()
    state = check(state, "write_memory")
    eng.re[:50] *= 1.5
    eng.tables_updated()
    check(state, "tables_updated")
    eng.close()


def test_existing_calls_are_what_they_were_around_group_calls():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, head=False)
    users = _dev(r.users)
    slate = _dev(np.arange(0, r.I, 3, dtype=np.int32))
    pu, pi = _dev(np.repeat(r.users, 20)), _dev(np.tile(np.arange(20, dtype=np.int32) * 7, len(r.users)))
    eng = _engine(r)

    def existing():
        out = [_t(eng.topk_users(users, 10)), _t(eng.topk_users_deep(users, 300)), _t(eng.topk_slate(users, slate, 10)),
               (dc.words(eng.score_pairs_bydish(pu, pi).cpu().numpy()), np.zeros(1))]
        eng.check()
        return out

    before = existing()
    members = gc.list_members(r.U)
    for mode in ALL_MODES:
        _lists(eng, members, mode, 1024)
        _lists(eng, members, mode, 64, slate=np.arange(0, r.I, 3))
        _words(eng, members, mode, np.arange(0, r.I, 3))
    assert _abi(eng, members, gc.LEAST, 1025)[0] == _native.M2D_ERR_INVALID_ARG                # a refused call
    bad = members.copy(); bad[3, 0] = r.U                                                        # a failed one
    assert _abi(eng, bad, gc.LEAST, 10)[0] == 0 and _latched(eng)[0] == _native.M2D_ERR_BAD_USER_ID
    for a, b in zip(before, existing()):
        _same(a, b, gc.LEAST, "an existing call moved")
    eng.close()


def test_torch_ops_and_the_model():
    import types
    import torch
    import foodrec_amd
    r = dc.normal_recipe(64, head=False)
    eng = _engine(r)
    members = gc.list_members(r.U)
    S = _matrix(eng, r.U, np.arange(r.I))
    lists = gc.exclusion_lists(r.I, len(members), gc.group_lists(S, members, gc.LEAST, 2)[1])
    off, ids = map(_dev, dc.csr(lists))
    want = _lists(eng, members, gc.LEAST, 300, lists)
    _same(_t(torch.ops.m2d.topk_groups(eng.id, _dev(members), 300, "least", off, ids)), want, gc.LEAST, "torch.ops.m2d.topk_groups")
    as_lists = [[int(u) for u in row if u >= 0] for row in members]
    _same(_t(eng.topk_groups(as_lists, 300, "least", lists)), want, gc.LEAST, "lists of id lists")
    slate = gc.slate_of(r.I, 129)
    _same(_t(torch.ops.m2d.topk_groups(eng.id, _dev(members), 20, "mean", None, None, _dev(slate))),
          _lists(eng, members, gc.MEAN, 20, slate=slate), gc.LEAST, "torch.ops.m2d.topk_groups(among)")
    got = torch.ops.m2d.score_groups(eng.id, _dev(members), _dev(slate), "most")
    assert np.array_equal(dc.words(got.cpu().numpy()), _words(eng, members, gc.MOST, slate))
    eng.check()
    eng.close()

    args = types.SimpleNamespace(num_categories=4, num_users=r.U, embed_size=r.E, high_level_score_coefficient=r.coef)
    model = foodrec_amd.Model(args, r.PM, r.RE, r.CE, None, device=torch.device("cuda", 0))
    model.set_dish_categories(r.cats)
    groups = [[str(u) for u in g] for g in as_lists]         # ids as the reference feeds them: str
    had = {str(u): set(lists[(3 * u) % len(lists)][:40]) for u in range(0, r.U, 2)}
    best = gc.group_lists(S, members, gc.LEAST, 1)[1]
    for g in range(0, len(groups), 2):                       # every other group's best dish: one of its first member's dishes
        had.setdefault(groups[g][0], set()).add(int(best[g, 0]))
    had = {u: sorted(x) for u, x in had.items()}
    union =[sorted({d for u in g for d in had.get(u, ())}) for g in groups]
    s, i = model.topk_group(groups, exclude=had)
    assert s.shape == i.shape == (len(groups), 10) and s.dtype == np.float32 and i.dtype == np.int32
    _same((dc.words(s), i), _lists(model.engine, members, gc.LEAST, 10, union), gc.LEAST, "Model.topk_group, dict exclusions")
    assert any(np.isin(_lists(model.engine, members, gc.LEAST, 10)[1][g], union[g]).any() for g in range(len(groups)))    # the union matters
    s, i = model.topk_group(groups, 7, "mean", exclude=union)
    _same((dc.words(s), i), _lists(model.engine, members, gc.MEAN, 7, union), gc.LEAST, "Model.topk_group, aligned exclusions")
    among = [int(d) for d in slate[::-1]] + [int(slate[0])]                          # any order, a repeat
    s, i = model.topk_group(groups, 12, "most", among=among)
    _same((dc.words(s), i), _lists(model.engine, members, gc.MOST, 12, slate=slate), gc.LEAST, "Model.topk_group(among)")
    rng = np.random.default_rng(3)
    R = 40
    roff = np.arange(0, 3 * r.I + 1, 3, dtype=np.int32)
    model.set_recipes((roff, rng.integers(0, R, 3 * r.I).astype(np.int32)), R)
    market = list(range(0, 24))
    cook = model.cookable(market, 1)
    assert 12 < cook.size < r.I
    s, i = model.topk_group(groups, 12, market=market, max_missing=1)
    _same((dc.words(s), i), _lists(model.engine, members, gc.LEAST, 12, slate=cook), gc.LEAST, "Model.topk_group(market)")
    for kw in (dict(market=market, among=among), dict(market=market, exclude=union), dict(among=among, exclude=union)):
        with pytest.raises(ValueError):
            model.topk_group(groups, 5, **kw)
    with pytest.raises(ValueError, match="1 <= k <= 1024"):
        model.topk_group(groups, 1025)


# ---- 6. errors and refusals --------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, I=300, U=8, seed=1, head=False)
    eng = _engine(r)
    members = gc.list_members(r.U, nG=4)
    slate = np.arange(0, 300, 2)
    off, ids = dc.csr([[1], [2, 3], [], [7]])
    bad = _native.M2D_ERR_INVALID_ARG
    for k in (0, 1025, r.I + 1, -3):
        assert _abi(eng, members, gc.LEAST, k)[0] == bad and "m2d_topk_groups: need 1 <= k <= min(1024, I)" in eng_error(eng)
    for k in (0, 1025, len(slate) + 1):
        assert _abi(eng, members, gc.LEAST, k, slate)[0] == bad and "1 <= k <= min(1024, nD)" in eng_error(eng)
    for M in (0, 65, -1):
        for k, sl in ((5, None), (5, slate), (None, slate)):
            assert _abi(eng, members, gc.LEAST, k, sl, M=M)[0] == bad and "1 <= M <= 64" in eng_error(eng)
    for mode in (-1, 3):
        for k, sl in ((5, None), (5, slate), (None, slate)):
            assert _abi(eng, members, mode, k, sl)[0] == bad and "mode must be" in eng_error(eng)
    for null in ("members", "scores", "out_ids"):
        assert _abi(eng, members, gc.LEAST, 5, null=(null,))[0] == bad and eng_error(eng) == "m2d_topk_groups: null buffer"
        assert _abi(eng, members, gc.LEAST, 5, slate, null=(null,))[0] == bad and eng_error(eng) == "m2d_topk_groups_slate: null buffer"
    for null in ("members", "slate", "out"):
        assert _abi(eng, members, gc.LEAST, None, slate, null=(null,))[0] == bad and eng_error(eng) == "m2d_score_groups_slate: null buffer"
    assert _abi(eng, members, gc.LEAST, 5, slate, null=("slate",))[0] == bad
    assert _abi(eng, members, gc.LEAST, 5, None, off, ids, null=("ids",))[0] == bad              # excl_off without excl_ids
    assert _abi(eng, members, gc.LEAST, None, np.arange(r.I + 1))[0] == bad                      # nD > I
    empty = np.zeros((0, 4), np.int32)                                                            # nG == 0: nothing is launched
    assert _abi(eng, empty, gc.LEAST, 5)[0] == 0 and _abi(eng, empty, gc.LEAST, 5, slate)[0] == 0 and _abi(eng, empty, gc.LEAST, None, slate)[0] == 0
    assert _latched(eng)[0] == 0
    eng.close()
    bare = _engine(r, masks=False)
    for k, sl in ((5, None), (5, slate), (None, slate)):
        assert _abi(bare, members, gc.LEAST, k, sl)[0] == _native.M2D_ERR_NOT_CONFIGURED
    bare.close()


def test_refusals_name_the_call():
    from foodrec_amd import _native
    from helpers import mlp_head
    r = dc.normal_recipe(64, I=300, U=8, seed=1, head=False)
    rng = np.random.default_rng(2)
    eng = _engine(r)
    members = gc.list_members(r.U, nG=6)
    slate = np.arange(0, 300, 2)
    forms = ((100, None, "m2d_topk_groups"), (100, slate, "m2d_topk_groups_slate"), (None, slate, "m2d_score_groups_slate"))
    want = _lists(eng, members, gc.LEAST, 100)
    nnz = 3 * r.I
    eng.set_ingredients((rng.standard_normal((50, r.E)) / 8).astype(np.float32), np.arange(0, nnz + 1, 3, dtype=np.int32),
                        rng.integers(0, 50, nnz).astype(np.int32))
    for k, sl, name in forms:
        assert _abi(eng, members, gc.LEAST, k, sl)[0] == _native.M2D_ERR_UNSUPPORTED
        assert eng_error(eng) == name + ": the ingredient table is set (not supported)"
    eng.clear_ingredients()
    _same(_lists(eng, members, gc.LEAST, 100), want, gc.LEAST, "after clear_ingredients")
    keep = eng.re[7, 3].item()
    eng.re[7, 3] = float("inf")
    eng.tables_updated()
    for k, sl, name in forms:
        assert _abi(eng, members, gc.LEAST, k, sl)[0] == _native.M2D_ERR_UNSUPPORTED
        assert eng_error(eng) == name + ": needs finite tables (a table value is not finite)"
    eng.re[7, 3] = keep
    eng.tables_updated()
    _same(_lists(eng, members, gc.LEAST, 100), want, gc.LEAST, "after the value was put back")
    eng.set_mlp_head(*mlp_head(5 * r.E, 256, 64, rng, scale=4.0))                    # an MLP head is ignored
    _same(_lists(eng, members, gc.LEAST, 100), want, gc.LEAST, "under an MLP head")
    eng.close()


def test_bad_members_and_exclusions_are_latched_with_value_and_position():
    from foodrec_amd import _native
    r = dc.normal_recipe(64, I=300, U=8, seed=1, head=False)
    base = 100
    eng = _engine(r, user_base=base)
    S = _matrix(eng, r.U, np.arange(r.I), user_base=base)
    members = gc.member_matrix(r.U, 12, 4, seed=3, user_base=base)           # counts 1, 2, 3, 4, 1, ...
    M = members.shape[1]
    good = [[1, 5], [], [0, 2, 299], [7]] * 3
    off, ids = dc.csr(good)
    slate = np.arange(0, 300, 2)
    want = gc.group_lists(S, members, gc.LEAST, 70, good, user_base=base)
    _same(_lists(eng, members, gc.LEAST, 70, good), want, gc.LEAST)
    BAD_USER, BAD_ITEM, INVALID = _native.M2D_ERR_BAD_USER_ID, _native.M2D_ERR_BAD_ITEM_ID, _native.M2D_ERR_INVALID_ARG

    def latched(members_, off_, ids_, code, value, index, spoilt):
        for P in (dc.DEFAULT_P, 256):                        # 256: blocks of one group -- the position is the caller's
            eng.set_option("deep_chunk_pairs", P)
            rc, s, i = _abi(eng, members_, gc.LEAST, 70, None, off_, ids_)
            assert rc == 0 and _latched(eng) == (code, value, index), (P, eng_error(eng))
            assert _latched(eng)[0] == 0                     # cleared; the engine is usable
            ok = np.setdiff1d(np.arange(len(members_)), [spoilt])
            if off_ is off and ids_ is ids:                  # a bad member: every other group's row is right
                _same((s[ok], i[ok]), (want[0][ok], want[1][ok]), gc.LEAST, "the other groups' rows")
            for k, sl in ((70, slate), (None, slate)):       # the slate forms latch the members alike
                if off_ is off and ids_ is ids:
                    assert _abi(eng, members_, gc.LEAST, k, sl)[0] == 0 and _latched(eng) == (code, value, index), (k, P)
            _same(_lists(eng, members, gc.LEAST, 70, good), want, gc.LEAST, "after a latched error")

    for g, j in ((0, 0), (6, 2), (11, 3)):                   # the first, a middle and the last used slot (group 11 has four members)
        assert members[g, j] >= 0
        for value in (base + r.U, base - 1, -2, -7):         # above the range, below it, below -1
            m = members.copy(); m[g, j] = value
            latched(m, off, ids, BAD_USER, value, g * M + j, g)
    m = members.copy(); m[5] = -1                            # an empty group
    latched(m, off, ids, INVALID, -1, 5 * M, 5)
    m = members.copy(); m[4, 2] = base + 3                   # group 4 has one member: [a, -1, id, -1] -- an id behind a -1
    assert m[4, 1] == -1
    latched(m, off, ids, INVALID, base + 3, 4 * M + 2, 4)
    x = ids.copy(); x[4] = r.I                               # position 4 of the id array: [0, 2, 299] -> 300
    latched(members, off, x, BAD_ITEM, r.I, 4, 2)
    x = ids.copy(); x[2], x[3] = 9, 2                        # [9, 2, 299]: the id at position 3 is below its predecessor
    latched(members, off, x, INVALID, 2, 3, 2)
    o = off.copy(); o[0] = 1
    latched(members, o, ids, INVALID, 1, 0, 0)
    bad_slate = slate.copy(); bad_slate[10] = bad_slate[9]   # the slate's own errors are m2d_topk_slate's
    assert _abi(eng, members, gc.LEAST, 20, bad_slate)[0] == 0 and _latched(eng) == (INVALID, int(bad_slate[10]), 10)
    bad_slate[10] = r.I
    assert _abi(eng, members, gc.LEAST, None, bad_slate)[0] == 0 and _latched(eng) == (BAD_ITEM, r.I, 10)
    eng.close()
