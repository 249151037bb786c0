"""GPU tests of the profile calls (m2d_compose_profiles, m2d_topk_profiles, m2d_score_profiles, m2d_topk_markets_profiles; DESIGN.md
section 8.7), through the C ABI into poisoned buffers with a guard row on either side.  The composer against the float64 restatement --
bit for bit on exact recipes, inside the op sequence's gamma-bound on normal tables --, containment and errors by code, value and
position, the witness against Write_Memory, every served call against the same call on an engine built on the composed rows, the
engine's own state around a profile call, and the Python surface.  Recipes, restatement, stand-ins: tests/profile_cases.py.

Time of the whole file: see README.md (status row "profiles")."""
import ctypes
import types

import numpy as np
import pytest

import profile_cases as pc

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN word no kernel writes; no dish id, no count
LITERAL = "m2d_topk_literal"


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _small_engine(PM, user_base=0):
    """an engine for the composer alone: the case's Personal_Memory, three dishes"""
    from foodrec_amd import ScoringEngine
    C, E = PM.shape[1] - 1, PM.shape[2]
    rng = np.random.default_rng(E)
    return ScoringEngine(PM, rng.standard_normal((3, E)).astype(np.float32), rng.standard_normal((C, E)).astype(np.float32),
                         coef=pc.COEF, user_base=user_base)


def _served_engine(c, PM=None, user_base=0):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(c.PM if PM is None else PM, c.RE, c.CE, coef=pc.COEF, user_base=user_base)
    eng.set_dish_categories(c.cats)
    eng.set_recipes(c.off, c.ids, c.R)
    return eng


def _batch(users, labels, GM, alpha):
    """(m2d_profile_batch, the device tensors it points into)"""
    from foodrec_amd import _native
    u = _dev(np.asarray(users, np.int32)) if users is not None else None
    y, g = _dev(np.asarray(labels, np.float32)), (GM if not isinstance(GM, np.ndarray) else _dev(GM))
    return _native.ProfileBatch(u.data_ptr() if u is not None else None, y.data_ptr(), g.data_ptr(), y.shape[0], y.shape[1], float(alpha)), (u, y, g)


def _guarded(n, *tail):
    import torch
    return torch.full((n + 2,) + tail, POISON, dtype=torch.int32, device="cuda")


def _inner(t, written=True):
    """the call's rows of a guarded buffer as int32 words, after checking that the guard rows were not written and every word between was"""
    a = t.cpu().numpy()
    assert (a[0] == POISON).all() and (a[-1] == POISON).all(), "a guard row was written"
    assert not written or (a[1:-1] != POISON).all(), "words of the call's rows were not written"
    return a[1:-1]


def _latched(eng):
    """m2d_check: (code, bad value, bad index); synchronises and clears the latch"""
    from foodrec_amd import _native
    bv, bi = ctypes.c_int64(), ctypes.c_int64()
    rc = _native.lib().m2d_check(eng._h, _stream(), ctypes.byref(bv), ctypes.byref(bi))
    return rc, bv.value, bi.value


def _compose(eng, users, labels, GM, alpha, rc_want=0):
    """m2d_compose_profiles -> float32 [n, (C+1) E]"""
    from foodrec_amd import _native
    n, W = len(labels), (eng.C + 1) * eng.E
    b, keep = _batch(users, labels, GM, alpha)
    out = _guarded(n, W)
    rc = _native.lib().m2d_compose_profiles(eng._h, ctypes.byref(b), out[1:].data_ptr(), _stream())
    assert rc == rc_want, _native.error_text(eng._h)
    return _inner(out).view(np.float32)


def _topk(eng, users, labels, GM, alpha, k, exclude=None):
    """m2d_topk_profiles -> (score words i32[n, k], ids i32[n, k]); exclude: (offsets, ids) arrays"""
    from foodrec_amd import _native
    n = len(labels)
    b, keep = _batch(users, labels, GM, alpha)
    s, i = _guarded(n, k), _guarded(n, k)
    xo = xi = None
    if exclude is not None:
        xo, xi = _dev(np.asarray(exclude[0], np.int64)), _dev(np.asarray(exclude[1], np.int32) if len(exclude[1]) else np.zeros(1, np.int32))
    rc = _native.lib().m2d_topk_profiles(eng._h, ctypes.byref(b), k, xo.data_ptr() if xo is not None else None,
                                         xi.data_ptr() if xi is not None else None, s[1:].data_ptr(), i[1:].data_ptr(), _stream())
    _native.raise_for(rc, eng._h)
    return _inner(s), _inner(i)


def _csr(lists, dtype=np.int32):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, (np.concatenate([np.asarray(x, dtype) for x in lists]).astype(dtype) if off[-1] else np.zeros(0, dtype))


def _words(t):
    return t.cpu().numpy().view(np.int32)


@pytest.fixture(scope="module")
def num_cu():
    eng = _small_engine(np.zeros((1, 5, 4), np.float32))
    n = eng.get_option("num_cu")
    eng.close()
    return n


@pytest.fixture(scope="module")
def served():
    """per catalogue: (case, engine, composed rows, an engine built on those rows), made on first use and shared"""
    made = {}

    def get(I):
        if I not in made:
            c = pc.served_case(I)
            eng = _served_engine(c)
            rows = _compose(eng, c.users, c.labels, c.GM, c.alpha)
            assert _latched(eng) == (0, 0, 0)
            made[I] = (c, eng, rows, _served_engine(c, PM=rows.reshape(c.n, c.C + 1, c.E).copy()))
        return made[I]

    yield get
    for _, a, _, b in made.values():
        a.close()
        b.close()


# ---- 1. exact recipes: bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.EXACT_SHAPES)
def test_composer_equals_the_restatement_on_exact_recipes(shape, num_cu):
    L, E, C, n, mode, base = shape
    c = pc.exact_case(L, E, C, pc.second_trip_requests(num_cu) if n is None else n, mode, base)
    eng = _small_engine(c.PM, base)
    try:
        got = _compose(eng, c.users, c.labels, c.GM, c.alpha)
        want = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float64, base)
        assert _latched(eng) == (0, 0, 0)
        assert not np.isnan(got).any()
        bad = np.flatnonzero((got.astype(np.float64) != want).any(1))
        assert bad.size == 0, "rows %s of %d differ from the restatement (L = %d, E = %d, C = %d)" % (bad[:8], c.n, L, E, C)
    finally:
        eng.close()


# ---- 2. normal tables: the gamma-bound -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.NORMAL_SHAPES)
def test_composer_is_inside_the_bound_on_normal_tables(shape):
    c = pc.normal_case(*shape)
    assert pc.bound_conditions(c.labels, c.alpha)
    eng = _small_engine(c.PM, c.user_base)
    try:
        got = _compose(eng, c.users, c.labels, c.GM, c.alpha)
        assert _latched(eng) == (0, 0, 0)
        want = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float64, c.user_base)
        err, b = np.abs(got.astype(np.float64) - want), pc.bound(c.PM, c.GM, c.labels, c.users, c.alpha, c.user_base)
        print("shape %s: largest error / bound = %.3f" % (shape, float((err / b).max())))
        assert (err <= b).all()
    finally:
        eng.close()


# ---- 3. containment and errors ---------------------------------------------------------------------------------------------------------------
def _right_rows(got, c, labels, users, GM, rows):
    want = pc.restate(c.PM, GM, labels, users, c.alpha, np.float64, c.user_base)
    with np.errstate(invalid="ignore"):
        b = pc.bound(c.PM, np.where(np.isfinite(GM), GM, 0), np.where(labels > 0, labels, 0) + (labels.sum(1, keepdims=True) == 0), users,
                     c.alpha, c.user_base)
    for q in rows:
        assert (np.abs(got[q].astype(np.float64) - want[q]) <= b[q]).all(), "row %d is wrong" % q


def test_containment_and_user_errors_by_code_value_and_position():
    from foodrec_amd import _native
    c = pc.normal_case(*pc.NORMAL_SHAPES[0])
    eng = _small_engine(c.PM, c.user_base)
    every = range(c.n)
    try:
        # a request without labels: a row of zeros, (INVALID_ARG, 0 labels, request 2)
        y = c.labels.copy()
        y[2] = 0
        got = _compose(eng, c.users, y, c.GM, c.alpha)
        assert _latched(eng) == (_native.M2D_ERR_INVALID_ARG, 0, 2)
        assert (got[2] == 0).all()
        _right_rows(got, c, y, c.users, c.GM, [q for q in every if q != 2])
        # an inf in a General_Memory row one request addresses: that row is zeros, (INVALID_ARG, its label count, its index)
        used = (c.labels != 0).sum(0)
        l1 = int(np.flatnonzero(used == 1)[0])
        q1 = int(np.flatnonzero(c.labels[:, l1])[0])
        GM = c.GM.copy()
        GM[l1, 2, 5] = np.inf
        got = _compose(eng, c.users, c.labels, GM, c.alpha)
        assert _latched(eng) == (_native.M2D_ERR_INVALID_ARG, int((c.labels[q1] != 0).sum()), q1)
        assert (got[q1] == 0).all()
        _right_rows(got, c, c.labels, c.users, GM, [q for q in every if q != q1])
        # an inf (and a NaN) in rows nobody addresses: it does not matter
        GM = c.GM.copy()
        l0 = np.flatnonzero(used == 0)[:2]
        GM[l0[0]], GM[l0[1], 0, 0] = np.inf, np.nan
        got = _compose(eng, c.users, c.labels, GM, c.alpha)
        assert _latched(eng) == (0, 0, 0)
        _right_rows(got, c, c.labels, c.users, GM, every)
        # overflow: finite inputs, an infinite row
        got = _compose(eng, c.users, c.labels, c.GM, 3e38)
        rc, m, q = _latched(eng)
        assert rc == _native.M2D_ERR_INVALID_ARG and m == int((c.labels[q] != 0).sum()) and (got[q] == 0).all()
        # user ids outside the table, other than -1
        for bad in (-2, c.user_base + pc.N_KNOWN):
            u = c.users.copy()
            u[3] = bad
            got = _compose(eng, u, c.labels, c.GM, c.alpha)
            assert _latched(eng) == (_native.M2D_ERR_BAD_USER_ID, bad, 3)
            assert (got[3] == 0).all()
            _right_rows(got, c, c.labels, c.users, c.GM, [q for q in every if q != 3])
        # users == NULL: every request a guest
        got = _compose(eng, None, c.labels, c.GM, c.alpha)
        assert _latched(eng) == (0, 0, 0)
        _right_rows(got, c, c.labels, None, c.GM, every)
    finally:
        eng.close()


def test_host_side_refusals(served):
    import torch
    from foodrec_amd import _native
    lib = _native.lib()
    c, eng, rows, _ = served(255)
    b, keep = _batch(c.users, c.labels, c.GM, c.alpha)
    out = torch.empty((c.n, 64), dtype=torch.int32, device="cuda")
    o, st = out.data_ptr(), _stream()
    INV = _native.M2D_ERR_INVALID_ARG

    def variant(**kw):
        v = _native.ProfileBatch(b.users, b.labels, b.general_memory, b.n, b.L, b.alpha)
        for key, val in kw.items():
            setattr(v, key, val)
        return ctypes.byref(v)

    for entry, call in (("m2d_compose_profiles", lambda p: lib.m2d_compose_profiles(eng._h, p, o, st)),
                        ("m2d_topk_profiles", lambda p: lib.m2d_topk_profiles(eng._h, p, 10, None, None, o, o, st)),
                        ("m2d_score_profiles", lambda p: lib.m2d_score_profiles(eng._h, p, o, o, 1, o, st)),
                        ("m2d_topk_markets_profiles",
                         lambda p: lib.m2d_topk_markets_profiles(eng._h, p, o, o, 0, None, None, 10, 0, o, o, None, None, st))):
        for p in (None, variant(labels=None), variant(general_memory=None), variant(L=0), variant(n=-1), variant(alpha=float("nan")),
                  variant(alpha=float("inf"))):
            assert call(p) == INV
            assert _native.error_text(eng._h).startswith(entry + ":"), _native.error_text(eng._h)
        assert call(variant(n=0)) == 0
    p = ctypes.byref(b)
    assert lib.m2d_compose_profiles(eng._h, p, None, st) == INV
    for k, xo in ((0, None), (65, None), (17, o), (c.I + 1, None)):
        assert lib.m2d_topk_profiles(eng._h, p, k, xo, o if xo else None, o, o, st) == INV
        assert "m2d_topk_profiles" in _native.error_text(eng._h)
    assert lib.m2d_topk_profiles(eng._h, p, 10, o, None, o, o, st) == INV
    assert lib.m2d_topk_profiles(eng._h, p, 10, None, None, None, o, st) == INV
    assert lib.m2d_score_profiles(eng._h, p, o, o, -1, o, st) == INV
    assert lib.m2d_score_profiles(eng._h, p, None, o, 1, o, st) == INV
    assert lib.m2d_topk_markets_profiles(eng._h, p, o, o, 0, None, None, 65, 0, o, o, None, None, st) == INV
    assert lib.m2d_topk_markets_profiles(eng._h, p, o, o, 0, None, None, 10, -1, o, o, None, None, st) == INV
    assert lib.m2d_topk_markets_profiles(eng._h, p, None, o, 0, None, None, 10, 0, o, o, None, None, st) == INV
    assert _latched(eng) == (0, 0, 0)
    # nothing configured: the refusal names the entry
    bare = _small_engine(c.PM)
    try:
        assert lib.m2d_topk_profiles(bare._h, p, 1, None, None, o, o, st) == _native.M2D_ERR_NOT_CONFIGURED
        assert _native.error_text(bare._h).startswith("m2d_topk_profiles:")
        assert lib.m2d_score_profiles(bare._h, p, o, o, 1, o, st) == _native.M2D_ERR_NOT_CONFIGURED
        assert lib.m2d_topk_markets_profiles(bare._h, p, o, o, 0, None, None, 10, 0, o, o, None, None, st) == _native.M2D_ERR_NOT_CONFIGURED
    finally:
        bare.close()


def test_bad_exclusions_are_latched_as_the_user_call_latches_them(served):
    from foodrec_amd import _native
    c, eng, rows, eng2 = served(257)
    # segments of 0, 1 and 65 ids whose concatenation ascends: each case below then holds exactly one violation, and the first error
    # latched does not depend on which thread is first
    off, ids = _csr([[], [0], list(range(1, 66)), [], [200]])
    users2 = _dev(np.arange(c.n, dtype=np.int32))
    INV, ITEM = _native.M2D_ERR_INVALID_ARG, _native.M2D_ERR_BAD_ITEM_ID
    cases = []
    bad = ids.copy()
    bad[off[3] - 1] = c.I                                     # an id outside the catalogue, the last of its segment
    cases.append((off, bad, (ITEM, c.I, int(off[3] - 1))))
    bad = ids.copy()
    bad[off[2] + 9] = 8                                       # an id below its predecessor (9)
    cases.append((off, bad, (INV, 8, int(off[2] + 9))))
    o2 = off.copy()
    o2[3] = 0                                                 # an offset below its predecessor
    cases.append((o2, ids, (INV, 0, 3)))
    for xo, xi, expected in cases:
        _topk(eng, c.users, c.labels, c.GM, c.alpha, 10, (xo, xi))
        got = _latched(eng)
        eng2.topk_users_excluding(users2, 10, (_dev(xo), _dev(xi)))
        want = _latched(eng2)
        assert got == want == expected, (got, want, expected)
    # and the call after them is clean
    s, i = _topk(eng, c.users, c.labels, c.GM, c.alpha, 10, (off, ids))
    s2, i2 = eng2.topk_users_excluding(users2, 10, (_dev(off), _dev(ids)))
    assert _latched(eng) == (0, 0, 0) and np.array_equal(i, i2.cpu().numpy()) and np.array_equal(s, _words(s2))


def test_non_finite_personal_memory_rows_as_computed_and_the_literal_lists(served):
    """an inf in Personal_Memory: the engine's word is 1, rows are written as computed (a request without labels is NaN, nothing is
    latched), retrieval takes m2d_topk_literal and returns what it returns on an engine built on those rows"""
    from foodrec_amd import _native
    c = pc.served_case(255)
    PM = c.PM.copy()
    PM[3, 1, 7] = np.inf                                      # user 3 is request 0's
    y = c.labels.copy()
    y[1] = 0
    eng = _served_engine(c, PM=PM)
    try:
        rows = _compose(eng, c.users, y, c.GM, c.alpha)
        assert _latched(eng) == (0, 0, 0)
        assert np.isnan(rows[1]).all() and np.isinf(rows[0, 1 * c.E + 7]) and np.isfinite(rows[2:]).all()
        want = pc.restate(PM, c.GM, y, c.users, c.alpha, np.float64)
        b = pc.bound(np.where(np.isfinite(PM), PM, 0), c.GM, y + (y.sum(1, keepdims=True) == 0), c.users, c.alpha)
        assert (np.abs(rows[2:].astype(np.float64) - want[2:]) <= b[2:]).all()
        eng2 = _served_engine(c, PM=rows.reshape(c.n, c.C + 1, c.E).copy())
        try:
            users_before = _dev(np.arange(pc.N_KNOWN, dtype=np.int32))
            before = [_words(t) for t in eng.topk_users(users_before, 10)]
            for k in (1, 10, 64):
                s, i = _topk(eng, c.users, y, c.GM, c.alpha, k)
                assert eng.last_kernel() == LITERAL
                s2, i2 = eng2.topk_users(_dev(np.arange(c.n, dtype=np.int32)), k)
                assert eng2.last_kernel() == LITERAL
                assert np.array_equal(i, i2.cpu().numpy()) and np.array_equal(s, _words(s2)), "k = %d" % k
            # with exclusions the user call refuses non-finite tables: so does this one, under its own name, from inside the view --
            # and the engine's own table is back in place
            off, ids = _csr(c.exclude)
            with pytest.raises(ValueError, match="m2d_topk_profiles: needs finite tables"):
                _topk(eng, c.users, y, c.GM, c.alpha, 10, (off, ids))
            after = [_words(t) for t in eng.topk_users(users_before, 10)]
            assert all(np.array_equal(a, b_) for a, b_ in zip(before, after))
            assert _latched(eng) == (0, 0, 0)
            assert _native.lib().m2d_abi_version() == 2
        finally:
            eng2.close()
    finally:
        eng.close()


# ---- 4. the witness: Write_Memory ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((130, 68, 4, 5, "known", 0), (95, 64, 4, 5, "known", 7000), (257, 6, 3, 4, "known", 0)))
def test_rows_equal_personal_memory_after_write_memory(shape):
    import torch
    c = pc.normal_case(*shape)
    assert len(set(c.users.tolist())) == c.n
    eng, clone = _small_engine(c.PM, c.user_base), _small_engine(c.PM.copy(), c.user_base)
    try:
        rows = _compose(eng, c.users, c.labels, c.GM, c.alpha)
        assert _latched(eng) == (0, 0, 0)
        gm = _dev(c.GM)
        clone.write_memory(_dev(c.users), torch.zeros(c.n, dtype=torch.int32, device="cuda"), torch.ones((c.n, c.C), device="cuda"),
                           torch.ones(c.n, device="cuda"), _dev(c.labels), gm, 0.0, 0.0, c.alpha, write_pm=True, write_gm=False)
        assert _latched(clone) == (0, 0, 0)
        written = clone.pm.cpu().numpy().reshape(pc.N_KNOWN, c.W)[c.users - c.user_base]
        assert np.array_equal(rows.view(np.uint32), written.view(np.uint32)), "%d words differ" % int((rows.view(np.uint32) != written.view(np.uint32)).sum())
        assert np.array_equal(gm.cpu().numpy(), c.GM) and np.array_equal(eng.pm.cpu().numpy(), c.PM), "a table was written"
    finally:
        eng.close()
        clone.close()


# ---- 5. every served call equals the call it stands for, on an engine built on the rows -------------------------------------------------------
@pytest.mark.parametrize("I", pc.CATALOGUES)
def test_topk_profiles_equals_topk_users_on_the_rows(served, I):
    c, eng, rows, eng2 = served(I)
    users2 = _dev(np.arange(c.n, dtype=np.int32))
    for k in pc.SERVED_KS:
        s, i = _topk(eng, c.users, c.labels, c.GM, c.alpha, k)
        kernel = eng.last_kernel()
        s2, i2 = eng2.topk_users(users2, k)
        assert kernel == eng2.last_kernel()
        assert np.array_equal(i, i2.cpu().numpy()), "I = %d, k = %d: ids differ" % (I, k)
        assert np.array_equal(s, _words(s2)), "I = %d, k = %d: score words differ" % (I, k)
    assert eng.last_kernel() != LITERAL
    off, ids = _csr(c.exclude)
    for k in (1, 10, 16):
        s, i = _topk(eng, c.users, c.labels, c.GM, c.alpha, k, (off, ids))
        s2, i2 = eng2.topk_users_excluding(users2, k, (_dev(off), _dev(ids)))
        assert np.array_equal(i, i2.cpu().numpy()) and np.array_equal(s, _words(s2)), "I = %d, k = %d with exclusions" % (I, k)
        for q in range(c.n):
            assert not np.isin(i[q], c.exclude[q]).any()
    assert _latched(eng) == (0, 0, 0) and _latched(eng2) == (0, 0, 0)


@pytest.mark.parametrize("I", (257, 16385))
def test_score_profiles_equals_score_pairs_bydish_on_the_rows(served, I):
    from foodrec_amd import _native
    c, eng, rows, eng2 = served(I)
    rng = np.random.default_rng(I)
    for B, bad_at in ((1, None), (300, 17)):
        r, d = rng.integers(0, c.n, B).astype(np.int32), rng.integers(0, I, B).astype(np.int32)
        if bad_at is not None:
            r[bad_at] = c.n
        rt, dt = _dev(r), _dev(d)
        b, keep = _batch(c.users, c.labels, c.GM, c.alpha)
        out = _guarded(B)
        rc = _native.lib().m2d_score_profiles(eng._h, ctypes.byref(b), rt.data_ptr(), dt.data_ptr(), B, out[1:].data_ptr(), _stream())
        assert rc == 0, _native.error_text(eng._h)
        got = _inner(out)
        want = _words(eng2.score_pairs_bydish(rt, dt))
        err = (0, 0, 0) if bad_at is None else (_native.M2D_ERR_BAD_USER_ID, c.n, bad_at)
        assert _latched(eng) == err and _latched(eng2) == err
        assert np.array_equal(got, want), "B = %d: %d words differ" % (B, int((got != want).sum()))


@pytest.mark.parametrize("I", (256, 16385))
def test_topk_markets_profiles_equals_topk_markets_excluding_on_the_rows(served, I):
    from foodrec_amd import _native
    c, eng, rows, eng2 = served(I)
    moff, mids = _csr(c.markets)
    xoff, xids = _csr(c.exclude)
    users2 = _dev(np.arange(c.n, dtype=np.int32))
    mo, mi, xo, xi = _dev(moff), _dev(mids), _dev(xoff), _dev(xids)
    k, mm = 10, 2
    try:
        for shares in (1, 3):
            eng.set_option("market_shares", shares)
            eng2.set_option("market_shares", shares)
            for excl in (False, True):
                b, keep = _batch(c.users, c.labels, c.GM, c.alpha)
                s, i, n, m = _guarded(c.n, k), _guarded(c.n, k), _guarded(c.n), _guarded(c.n, k, mm)
                rc = _native.lib().m2d_topk_markets_profiles(eng._h, ctypes.byref(b), mo.data_ptr(), mi.data_ptr(), mi.numel(),
                                                             xo.data_ptr() if excl else None, xi.data_ptr() if excl else None, k, mm,
                                                             s[1:].data_ptr(), i[1:].data_ptr(), n[1:].data_ptr(), m[1:].data_ptr(), _stream())
                assert rc == 0, _native.error_text(eng._h)
                assert eng.get_option("market_shares_used") == min(shares, -(-I // 256))
                want = eng2.topk_markets_excluding(users2, (mo, mi), (xo, xi) if excl else None, k, mm, return_counts=True, return_missing=True)
                for got, w, what in zip((s, i, n, m), want, ("score words", "ids", "counts", "missing entries")):
                    assert np.array_equal(_inner(got), _words(w)), "I = %d, %d shares, exclusions %s: %s differ" % (I, shares, excl, what)
                assert (_inner(n) > 0).all() and (_inner(m) >= 0).any()        # (an empty market still cooks what lacks two entries)
        assert _latched(eng) == (0, 0, 0) and _latched(eng2) == (0, 0, 0)
    finally:
        eng.set_option("market_shares", 0)
        eng2.set_option("market_shares", 0)


# ---- 6. the view leaves the engine as it found it ------------------------------------------------------------------------------------------------
def test_the_engine_is_as_it_was_after_profile_calls():
    import torch
    from foodrec_amd import _native
    c = pc.served_case(257)
    base = 500
    eng = _served_engine(c, user_base=base)
    try:
        eng.set_option("user_high_table", 1)
        eng.set_option("pm_bf16", 1)
        rng = np.random.default_rng(6)
        B = 2 ** 18 + 77
        users = _dev(np.arange(base, base + pc.N_KNOWN, dtype=np.int32))
        pu, pd = _dev(rng.integers(base, base + pc.N_KNOWN, B).astype(np.int32)), _dev(rng.integers(0, c.I, B).astype(np.int32))

        def snapshot():
            s, i = eng.topk_users(users, 10)
            return [_words(s), i.cpu().numpy(), _words(eng.score_pairs_bydish(pu, pd))]

        def same(a, b):
            return all(np.array_equal(x, y) for x, y in zip(a, b))

        before = snapshot()
        assert np.isfinite(before[2].view(np.float32)).all()
        pusers = np.where(c.users >= 0, c.users + base, -1).astype(np.int32)
        moff, mids = _csr(c.markets)
        first = _topk(eng, pusers, c.labels, c.GM, c.alpha, 10)
        eng.score_profiles(c.labels, _dev(c.GM), [0, 4, 2], [5, 6, 7], users=pusers, alpha=c.alpha)
        eng.topk_markets_profiles(c.labels, _dev(c.GM), (moff, mids), 10, users=pusers, alpha=c.alpha, exclude=c.exclude)
        assert _latched(eng) == (0, 0, 0)
        assert eng.get_option("user_high_table") == 1 and eng.get_option("pm_bf16") == 1 and eng.user_base == base
        assert same(before, snapshot()), "a profile call changed what the user calls return"
        # ... after a call that was refused, one that latched an error, and one refused inside the view
        with pytest.raises(ValueError):
            _topk(eng, pusers, c.labels, c.GM, c.alpha, 0)
        bad = pusers.copy()
        bad[0] = base + pc.N_KNOWN
        _topk(eng, bad, c.labels, c.GM, c.alpha, 10)
        assert _latched(eng) == (_native.M2D_ERR_BAD_USER_ID, base + pc.N_KNOWN, 0)
        assert same(before, snapshot()), "a failed profile call changed what the user calls return"
        again = _topk(eng, pusers, c.labels, c.GM, c.alpha, 10)
        assert same(first, again)
        # a profile call while a table scan is pending scans the REAL table: an inf in Personal_Memory sends retrieval to the literal kernel
        assert eng.last_kernel() != LITERAL
        keepv = eng.pm[8, 0, 0].item()
        eng.pm[8, 0, 0] = float("inf")
        eng.tables_updated()
        _topk(eng, None, c.labels, c.GM, c.alpha, 10)
        assert eng.last_kernel() == LITERAL
        y = c.labels.copy()
        y[1] = 0
        rows = _compose(eng, None, y, c.GM, c.alpha)
        assert np.isnan(rows[1]).all() and _latched(eng) == (0, 0, 0)       # the word is 1: as computed, nothing latched
        eng.pm[8, 0, 0] = keepv
        eng.tables_updated()
        assert same(first, _topk(eng, pusers, c.labels, c.GM, c.alpha, 10)) and eng.last_kernel() != LITERAL
        assert same(before, snapshot())
        torch.cuda.synchronize()
    finally:
        eng.close()


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------------------------
def test_python_surface_and_torch_ops(served):
    import torch
    c, eng, rows, eng2 = served(256)
    gm, y, u = _dev(c.GM), _dev(c.labels), _dev(c.users)
    r = eng.compose_profiles(y, gm, u, c.alpha)
    assert tuple(r.shape) == (c.n, c.C + 1, c.E) and np.array_equal(_words(r).reshape(c.n, -1), rows.view(np.int32))
    assert np.array_equal(_words(torch.ops.m2d.compose_profiles(eng.id, y, gm, u, c.alpha)), _words(r))
    assert np.array_equal(_words(eng.compose_profiles(c.labels, c.GM, c.users.tolist(), c.alpha)), _words(r))     # host arrays, a list of ids
    s, i = _topk(eng, c.users, c.labels, c.GM, c.alpha, 10)
    for got in (eng.topk_profiles(y, gm, 10, u, c.alpha), torch.ops.m2d.topk_profiles(eng.id, y, gm, 10, u, c.alpha)):
        assert np.array_equal(_words(got[0]), s) and np.array_equal(got[1].cpu().numpy(), i)
    off, ids = _csr(c.exclude)
    sx, ix = _topk(eng, c.users, c.labels, c.GM, c.alpha, 10, (off, ids))
    for got in (eng.topk_profiles(y, gm, 10, u, c.alpha, exclude=[x[::-1] for x in c.exclude]),
                torch.ops.m2d.topk_profiles(eng.id, y, gm, 10, u, c.alpha, _dev(off), _dev(ids))):
        assert np.array_equal(_words(got[0]), sx) and np.array_equal(got[1].cpu().numpy(), ix)
    # label-id lists are one-hot rows; guests by default
    lists = [[3, 94], [0], [7, 8, 9], [50], [1, 2]]
    onehot = np.zeros((5, c.L), np.float32)
    for q, l in enumerate(lists):
        onehot[q, l] = 1
    assert np.array_equal(_words(eng.compose_profiles(lists, gm)), _compose(eng, None, onehot, c.GM, 1.0).view(np.int32).reshape(5, c.C + 1, c.E))
    with pytest.raises(IndexError):
        eng.compose_profiles([[c.L]], gm)
    with pytest.raises(ValueError):
        eng.compose_profiles(y, gm[:, :-1])
    with pytest.raises(ValueError):
        eng.topk_profiles(y, gm, 10, u[:-1])
    # score_profiles and topk_markets_profiles against the engine on the rows
    sc = eng.score_profiles(y, gm, [0, 1, 4], [9, 8, 7], users=u, alpha=c.alpha)
    assert np.array_equal(_words(sc), _words(eng2.score_pairs_bydish(_dev(np.asarray([0, 1, 4], np.int32)), _dev(np.asarray([9, 8, 7], np.int32)))))
    got = eng.topk_markets_profiles(y, gm, c.markets, 10, users=u, alpha=c.alpha, exclude=c.exclude, max_missing=1, return_counts=True,
                                    return_missing=True)
    want = eng2.topk_markets_excluding(np.arange(c.n), c.markets, c.exclude, 10, 1, return_counts=True, return_missing=True)
    assert len(got) == 4 and all(np.array_equal(_words(a), _words(b)) for a, b in zip(got, want))
    eng.check()
    eng2.check()


def test_model_topk_for_labels_reads_general_memory_as_write_memory_left_it():
    import torch
    import foodrec_amd
    c = pc.served_case(256)
    args = types.SimpleNamespace(num_categories=c.C, num_users=pc.N_KNOWN, embed_size=c.E, high_level_score_coefficient=pc.COEF,
                                 num_labels=c.L, alpha=0.25, beta_1=0.5, beta_2=0.5)
    model = foodrec_amd.Model(args, c.PM, c.RE, c.CE, c.GM.copy(), device=torch.device("cuda", 0))
    model.set_dish_categories(c.cats)
    model.set_recipes((c.off, c.ids), c.R)
    lists = [[3, 94], [0], [7, 8, 9]]
    onehot = np.zeros((3, c.L), np.float32)
    for q, l in enumerate(lists):
        onehot[q, l] = 1

    def on_the_rows(GM, users, alpha, k, exclude=None):
        rows = _compose(model.engine, users, onehot, GM, alpha)
        eng2 = _served_engine(c, PM=rows.reshape(3, c.C + 1, c.E).copy())
        try:
            u2 = _dev(np.arange(3, dtype=np.int32))
            s, i = eng2.topk_users(u2, k) if exclude is None else eng2.topk_users_excluding(u2, k, exclude)
            return s.cpu().numpy(), i.cpu().numpy()
        finally:
            eng2.close()

    s0, i0 = model.topk_for_labels(lists, k=10)
    w0 = on_the_rows(c.GM, None, 1.0, 10)
    assert np.array_equal(i0, w0[1]) and np.array_equal(s0.view(np.int32), w0[0].view(np.int32))
    # a write that changes General_Memory (and Personal_Memory) is visible to the next call
    B = 6
    rng = np.random.default_rng(3)
    y = np.zeros((B, c.L), np.float32)
    y[np.arange(B), [3, 94, 0, 7, 8, 9]] = 1
    model.write_memory(rng.integers(0, pc.N_KNOWN, B).astype(np.int32), rng.integers(0, c.I, B).astype(np.int32),
                       c.cats[:B].reshape(B, c.C, 1).tolist(), np.ones((B, 1), np.float32), y)
    GM1 = model.general_memory()
    assert not np.array_equal(GM1, c.GM)
    s1, i1 = model.topk_for_labels(lists, k=10)
    w1 = on_the_rows(GM1, None, 1.0, 10)
    assert np.array_equal(i1, w1[1]) and np.array_equal(s1.view(np.int32), w1[0].view(np.int32))
    assert not np.array_equal(s1.view(np.int32), s0.view(np.int32)), "the write did not reach the next guest call"
    # known users take args.alpha and their own block; exclusions by dict; markets
    users = ["4", "1", "4"]
    had = {"4": [int(i1[0, 0]), int(i1[2, 1])], "1": []}
    s2, i2 = model.topk_for_labels(lists, k=5, users=users, exclude=had)
    xo, xi = _csr([sorted(had["4"]), [], sorted(had["4"])])
    w2 = on_the_rows(GM1, np.asarray([4, 1, 4], np.int32), 0.25, 5, (_dev(xo), _dev(xi)))
    assert np.array_equal(i2, w2[1]) and np.array_equal(s2.view(np.int32), w2[0].view(np.int32))
    sm, im = model.topk_for_labels(onehot, k=10, market=[c.markets[0], c.markets[2], []])
    assert (im[:2, 0] >= 0).all() and (im[2] == -1).all() and np.isnan(sm[2]).all()
    with pytest.raises(ValueError):
        model.topk_for_labels(lists, exclude={"4": [1]})
    model.engine.close()
