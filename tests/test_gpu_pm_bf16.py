"""Option "pm_bf16": pair scores served from the bf16 mirror of Personal_Memory.

The contract is exact, and so is every comparison here: the mirror is torch's float32 -> bfloat16 image of the table, and a call it
serves returns, bit for bit and NaN for NaN, what the f32 kernels return on an engine built from the rounded table
(`cases.round_bf16(PM)`, option off).  The tables are scaled so that rounding moves a score by many bounds (pm_bf16_cases.py): a
kernel that read the f32 table would fail the oracle check on the rounded table at more than 85 % of the pairs.
"""
import functools

import numpy as np
import pytest

import pm_bf16_cases as cases
from helpers import assert_scores_close, assert_scores_match_nonfinite, random_case

pytestmark = pytest.mark.gpu

U, I, C = cases.U, cases.I, cases.C


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch


def _engine(PM, RE, CE, coef=0.99, mirror=False, dish=None, **kw):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(PM, RE, CE, coef=coef, **kw)
    if dish is not None:
        eng.set_dish_categories(dish)
    if mirror:
        eng.set_option("pm_bf16", 1)
    return eng


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()             # (a copy: the shared cases are read-only)


def _host(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    """Bit-equal where neither is NaN, NaN at the same positions."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int32), b[~nan].view(np.int32))


def _mirror_bits(eng):
    import torch
    m = eng.personal_memory_bf16()
    assert m.dtype == torch.bfloat16 and tuple(m.shape) == tuple(eng.pm.shape) and m.device == eng.pm.device
    return _host(m.view(torch.int16)).view(np.uint16)


def _assert_mirror_is_torchs(eng, PM, what):
    import torch
    got = _mirror_bits(eng)
    want = torch.as_tensor(PM).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(PM)
    assert np.array_equal(got[~nan], want[~nan]), "%s: %d of %d halves differ" % (what, int((got != want)[~nan].sum()), got.size)
    assert np.all(np.isnan(cases.from_bits(got[nan]))), what


def _name(small, hv=False):
    return "m2d_score_pairs_c4" + ("_small" if small else "") + ("_hv" if hv else "") + "_bf16"


# ---- 1. the mirror ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cx,E", [(4, 4), (4, 12), (4, 36), (4, 64), (4, 200), (4, 256), (2, 5)])
def test_mirror_is_the_rne_image_of_the_table(torch_cuda, Cx, E):
    """U = 257; the planted values of pm_bf16_cases.PLANTED at the first, the last and random elements.  (C = 2, E = 5: 3 855 floats,
    the three behind the last whole float4 take the builder's scalar tail.)"""
    PM, RE, CE, _, _, _ = cases.scaled_case(U, I, Cx, E, 1, 300 + E)
    PM = cases.plant(PM, seed=E)
    eng = _engine(PM, RE, CE)
    _assert_mirror_is_torchs(eng, PM, "E %d" % E)
    want = cases.bf16_bits(PM)
    nan = np.isnan(PM)
    assert np.array_equal(_mirror_bits(eng)[~nan], want[~nan])              # ... and of the numpy form the other tests round with
    eng.close()


def test_mirror_builder_second_sweep(torch_cuda):
    """m2d_build_pm_bf16 runs one float4 per thread on at most 8 blocks of 256 per CU: a table of more than num_cu * 8 * 256 float4
    takes its grid-stride loop round again."""
    E = 64
    num_cu = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    Ux = (num_cu * 8 * 256 * 4) // ((C + 1) * E) + 50
    PM, RE, CE, _, _, _ = cases.scaled_case(Ux, I, C, E, 1, 7)
    PM = cases.plant(PM, seed=1)
    eng = _engine(PM, RE, CE)
    assert eng.get_option("num_cu") == num_cu and PM.size // 4 > num_cu * 8 * 256
    _assert_mirror_is_torchs(eng, PM, "second sweep")
    eng.close()


# ---- 2. scores --------------------------------------------------------------------------------------------------------------
def _check_scores(eng, ref_eng, case, users, items, cats, refs, small, what):
    """(a) the rounded-table engine's bits, (b) the f64 restatement on the rounded table, (c) the kernel's name; `cats` None: masks
    by dish.  (d), the visibility of the rounding in these inputs, is asserted by the caller on the references it holds."""
    u, i = _dev(users), _dev(items)
    if cats is None:
        got, want = eng.score_pairs_bydish(u, i), ref_eng.score_pairs_bydish(u, i)
    else:
        m = _dev(cats)
        got, want = eng.score_pairs(u, i, m), ref_eng.score_pairs(u, i, m)
    eng.check(); ref_eng.check()
    assert eng.last_kernel() == _name(small), (what, eng.last_kernel())
    assert ref_eng.last_kernel() == _name(small)[:-5], (what, ref_eng.last_kernel())
    got, want = _host(got), _host(want)
    assert _same_bits(got, want), "%s: %d of %d scores differ from the rounded-table engine" % (what, int((got != want).sum()), got.size)
    err = assert_scores_close(got, refs, what=what)
    return err


@pytest.mark.parametrize("coef", cases.COEFS)
@pytest.mark.parametrize("E", cases.E_GRID)
def test_scores_are_the_f32_kernels_on_the_rounded_table(torch_cuda, E, coef):
    case = cases.grid_case(E, coef)
    eng = _engine(case.PM, case.RE, case.CE, coef, mirror=True, dish=case.by_dish)
    ref_eng = _engine(case.PMr, case.RE, case.CE, coef, dish=case.by_dish)
    for feed in ("pair", "dish"):
        rounded, unrounded = case.refs[feed]
        share = cases.visible_share(rounded, unrounded)
        print("E %d coef %g %s: rounding visible at %.3f of the pairs" % (E, coef, feed, share))
        assert share >= cases.VISIBLE, (feed, share)                     # (d): reading the f32 table fails (b) at these pairs
        for B in cases.B_GRID:
            err = _check_scores(eng, ref_eng, case, case.users[:B], case.items[:B], case.cats[:B] if feed == "pair" else None,
                                rounded[:B], B <= 8192, "E %d coef %g %s B %d" % (E, coef, feed, B))
            print("  B %d: max |err| against f64 on the rounded table %.2e" % (B, err))
    eng.close(); ref_eng.close()


@functools.lru_cache(maxsize=None)
def _loop_case(B, seed):
    from oracle import m2d_oracle as oracle
    E, coef = 64, 0.5
    PM, RE, CE, users, items, cats = cases.scaled_case(U, I, C, E, B, seed)
    PMr = cases.round_bf16(PM)
    refs = (oracle.inference_f64(PMr, RE, CE, users, items, cats, coef), oracle.inference_f64(PM, RE, CE, users, items, cats, coef))
    import types
    return types.SimpleNamespace(PM=PM, PMr=PMr, RE=RE, CE=CE, users=users, items=items, cats=cats, refs=refs, coef=coef, E=E)


@pytest.mark.parametrize("form", ["throughput", "latency"])
def test_scores_at_the_loop_edges(torch_cuda, form):
    """blocks_per_cu = 1.  Throughput form: 4 num_cu waves of 64 pairs a sweep, B = 2 num_cu 256 + 65 ends in a third sweep with one
    whole chunk and one pair.  Latency form (variant 12): 4 num_cu waves of 64 / 16 pairs a pass at E = 64, B = 20 000 takes five."""
    num_cu = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    B = 2 * num_cu * 256 + 65 if form == "throughput" else 20000
    case = _loop_case(B, 11)
    share = cases.visible_share(*case.refs)
    assert share >= cases.VISIBLE, share
    eng = _engine(case.PM, case.RE, case.CE, case.coef, mirror=True)
    ref_eng = _engine(case.PMr, case.RE, case.CE, case.coef)
    for e in (eng, ref_eng):
        e.set_option("blocks_per_cu", 1)
        e.set_option("variant", 12 if form == "latency" else 0)
    err = _check_scores(eng, ref_eng, case, case.users, case.items, case.cats, case.refs[0], form == "latency", "loop edge " + form)
    print("%s form, B %d: visible share %.3f, max |err| %.2e" % (form, B, share, err))
    eng.close(); ref_eng.close()


# ---- 3. forms agree ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 36])
def test_every_form_returns_the_same_bits(torch_cuda, E):
    case = cases.grid_case(E, 0.5)
    eng = _engine(case.PM, case.RE, case.CE, 0.5, mirror=True, dish=case.by_dish)
    u, i, m = _dev(case.users), _dev(case.items), _dev(case.cats)
    base = {"pair": _host(eng.score_pairs(u, i, m)), "dish": _host(eng.score_pairs_bydish(u, i))}
    assert eng.last_kernel() == _name(False)
    forms = [{"prefetch": pf, "nt_loads": nt} for pf in (1, 2, 4) for nt in (0, 1)]
    forms += [{"skip_masked": 0}, {"skip_masked": 1}, {"variant": 11}, {"variant": 12}, {"blocks_per_cu": 1}, {"blocks_per_cu": 16}]
    defaults = {"prefetch": 2, "nt_loads": 1, "skip_masked": 1, "variant": 0, "blocks_per_cu": 8}
    for form in forms:
        for k, v in form.items():
            eng.set_option(k, v)
        got = {"pair": _host(eng.score_pairs(u, i, m)), "dish": _host(eng.score_pairs_bydish(u, i))}
        assert eng.last_kernel() == _name(form.get("variant") == 12), (form, eng.last_kernel())
        for feed in got:
            assert _same_bits(got[feed], base[feed]), (E, form, feed)
        for k in form:
            eng.set_option(k, defaults[k])
    eng.check()
    eng.close()


# ---- 4. the mirror's own non-finite word ------------------------------------------------------------------------------------
def _nonfinite_inputs(E, B=8193):
    PM, RE, CE, users, items, cats = cases.scaled_case(U, I, C, E, B, 500 + E, zero_rows=False)
    PM = PM.copy()
    return PM, RE, CE, users, items, cats


@pytest.mark.parametrize("E", [64, 36])
def test_nonfinite_values_of_the_table(torch_cuda, E):
    """+inf, -inf and NaN in low-level rows: the engine's word is set by the f32 scan, every row is fetched and multiplied."""
    from oracle import m2d_oracle as oracle
    PM, RE, CE, users, items, cats = _nonfinite_inputs(E)
    PM[3, 1, 1], PM[40, 2, E - 1], PM[77, 4, 0] = np.inf, -np.inf, np.nan
    users[:60:3], users[1:60:3], users[2:60:3] = 3, 40, 77
    PMr = cases.round_bf16(PM)
    ref = oracle.inference_f64(PMr, RE, CE, users, items, cats, 0.5)
    eng, ref_eng = _engine(PM, RE, CE, 0.5, mirror=True), _engine(PMr, RE, CE, 0.5)
    u, i, m = _dev(users), _dev(items), _dev(cats)
    for variant, small in ((11, False), (12, True)):
        for e in (eng, ref_eng):
            e.set_option("variant", variant)
        got, want = _host(eng.score_pairs(u, i, m)), _host(ref_eng.score_pairs(u, i, m))
        assert eng.last_kernel() == _name(small)
        assert _same_bits(got, want), (E, variant)
        assert_scores_match_nonfinite(got, ref, what="E %d variant %d" % (E, variant))
        assert np.isnan(got).sum() > 20 and np.isinf(got).sum() > 0
    eng.close(); ref_eng.close()


@pytest.mark.parametrize("E", [64, 36])
def test_rounding_to_inf_sets_the_mirrors_word(torch_cuda, E):
    """3.4e38 in the row of category 2 of user 9: finite in the f32 table (the engine's word stays clear) and +inf in the mirror.
    The pairs of user 9 that mask category 2 out score 0 * inf = NaN from the mirror -- the graph on the rounded table -- while the
    option-off engine on the unrounded table skips the row and returns finite scores there."""
    PM, RE, CE, users, items, cats = _nonfinite_inputs(E)
    PM[9, 1 + 2, 5] = 3.4e38
    users[:200] = 9
    cats[:200:2, 2] = 0.0; cats[:200:2, 0] = 1.0            # masked out (and a non-empty mask)
    cats[1:200:2, 2] = 1.0
    masked = np.zeros(len(users), bool); masked[:200:2] = True
    PMr = cases.round_bf16(PM)
    assert np.isinf(PMr[9, 3, 5]) and np.isfinite(PM).all()
    eng, ref_eng, plain = _engine(PM, RE, CE, 0.5, mirror=True), _engine(PMr, RE, CE, 0.5), _engine(PM, RE, CE, 0.5)
    u, i, m = _dev(users), _dev(items), _dev(cats)
    for variant, small in ((11, False), (12, True)):
        for e in (eng, ref_eng, plain):
            e.set_option("variant", variant)
        got, want, f32 = (_host(e.score_pairs(u, i, m)) for e in (eng, ref_eng, plain))
        assert eng.last_kernel() == _name(small)
        assert _same_bits(got, want), (E, variant)
        assert np.isnan(got[masked]).all() and np.isfinite(f32[masked]).all(), (E, variant)
        other = users != 9
        assert np.isfinite(got[other]).all()
    eng.close(); ref_eng.close(); plain.close()


# ---- 5. readers after writers -----------------------------------------------------------------------------------------------
def _writer_write_memory(eng, E):
    rng = np.random.default_rng(5)
    B, L = 600, 7
    users = (np.arange(B) % U).astype(np.int32)
    items = rng.integers(0, I, B).astype(np.int32)
    cats = rng.integers(0, 2, (B, C)).astype(np.float32); cats[cats.sum(1) == 0, 0] = 1
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = _dev((rng.standard_normal((L, C + 1, E)) / 4).astype(np.float32))
    eng.write_memory(_dev(users), _dev(items), _dev(cats), _dev(sign), _dev(y), gm, 1.0, 1.0, 0.5, write_pm=True, write_gm=False)


def _writer_train(variant, kernel):
    def run(eng, E):
        rng = np.random.default_rng(11)
        B = 256
        users = (rng.permutation(U)[:B]).astype(np.int32)
        items = rng.integers(0, I, B).astype(np.int32)
        cats = rng.integers(0, 2, (B, C)).astype(np.float32); cats[cats.sum(1) == 0, 0] = 1
        eng.train_begin("sgd", 200.0)
        eng.set_option("variant", variant)
        out = eng.train_step(_dev(users), _dev(items), _dev(cats), _dev(rng.integers(0, 2, B).astype(np.float32)), apply=True)
        eng.check()
        assert eng.last_kernel() == kernel and np.isfinite(_host(out)).all()
        eng.set_option("variant", 0)
        eng.train_end()
    return run


def _writer_in_place(eng, E):
    eng.pm.mul_(-1.37)
    eng.tables_updated()


@pytest.mark.parametrize("writer", [pytest.param(_writer_write_memory, id="write_memory"),
                                    pytest.param(_writer_train(0, "m2d_train_grad_fused"), id="train_step-fused"),
                                    pytest.param(_writer_train(14, "m2d_train_grad"), id="train_step-nine-launch"),
                                    pytest.param(_writer_in_place, id="tables_updated")])
def test_mirror_follows_every_writer(torch_cuda, writer):
    E, coef = 64, 0.5
    PM, RE, CE, users, items, cats = random_case(U, I, C, E, 4000, 21)
    eng = _engine(PM, RE, CE, coef, mirror=True)
    u, i, m = _dev(users), _dev(items), _dev(cats)
    mirror0, scores0 = _mirror_bits(eng), _host(eng.score_pairs(u, i, m))
    assert eng.last_kernel() == _name(True)
    writer(eng, E); eng.check()
    now = tuple(_host(t).copy() for t in (eng.pm, eng.re, eng.ce))
    _assert_mirror_is_torchs(eng, now[0], "after the writer")
    scores1 = _host(eng.score_pairs(u, i, m))
    fresh = _engine(cases.round_bf16(now[0]), now[1], now[2], coef)
    assert _same_bits(scores1, _host(fresh.score_pairs(u, i, m)))
    assert np.mean(_mirror_bits(eng) != mirror0) > 0.25, "the writer left the mirror nearly as it was: a stale mirror could pass"
    with np.errstate(invalid="ignore"):
        assert np.mean(scores1 != scores0) > 0.5
    # option off again: the f32 table, the f32 kernels
    eng.set_option("pm_bf16", 0)
    plain = _engine(*now, coef)
    assert _same_bits(_host(eng.score_pairs(u, i, m)), _host(plain.score_pairs(u, i, m)))
    assert eng.last_kernel() == plain.last_kernel() == "m2d_score_pairs_c4_small"
    assert eng.get_option("pm_bf16") == 0
    for e in (eng, fresh, plain):
        e.close()


# ---- 6. ids -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [100, 8193])
def test_user_base_and_bad_ids(torch_cuda, B):
    case = cases.grid_case(64, 0.5)
    base = 100000
    eng = _engine(case.PM, case.RE, case.CE, 0.5, mirror=True, user_base=base)
    ref_eng = _engine(case.PMr, case.RE, case.CE, 0.5, user_base=base)
    users, items, m = case.users[:B] + base, case.items[:B], _dev(case.cats[:B])
    good = _host(eng.score_pairs(_dev(users), _dev(items), m)); eng.check()
    assert eng.last_kernel() == _name(B <= 8192)
    assert _same_bits(good, _host(ref_eng.score_pairs(_dev(users), _dev(items), m)))
    assert_scores_close(good, case.refs["pair"][0][:B])
    for what, pos, bad_u, bad_i in (("user", 5, base + U, None), ("user", B - 1, base - 1, None), ("item", 9, None, I)):
        uu, ii = users.copy(), items.copy()
        if bad_u is not None:
            uu[pos] = bad_u
        if bad_i is not None:
            ii[pos] = bad_i
        got = _host(eng.score_pairs(_dev(uu), _dev(ii), m))
        with pytest.raises(IndexError, match=r"%s id %d at position %d " % (what, bad_u if bad_u is not None else bad_i, pos)):
            eng.check()
        keep = np.arange(B) != pos
        assert np.isnan(got[pos]) and _same_bits(got[keep], good[keep])
    assert _same_bits(_host(eng.score_pairs(_dev(users), _dev(items), m)), good); eng.check()      # usable afterwards
    eng.close(); ref_eng.close()


# ---- 7. shapes the C = 4 kernels do not cover -------------------------------------------------------------------------------
@pytest.mark.parametrize("Cx,E,B,variant,kernel", [(3, 64, 8193, 0, "m2d_score_pairs_cn"), (3, 64, 100, 0, "m2d_score_pairs_generic"),
                                                   (4, 6, 8193, 0, "m2d_score_pairs_generic"), (4, 64, 8193, 9, "m2d_score_pairs_generic")])
def test_other_shapes_keep_the_f32_kernels(torch_cuda, Cx, E, B, variant, kernel):
    PM, RE, CE, users, items, cats = cases.scaled_case(U, I, Cx, E, B, 40 + E)
    eng = _engine(PM, RE, CE, 0.5)
    eng.set_option("variant", variant)
    u, i, m = _dev(users), _dev(items), _dev(cats)
    off = _host(eng.score_pairs(u, i, m))
    assert eng.last_kernel() == kernel
    eng.set_option("pm_bf16", 1)
    on = _host(eng.score_pairs(u, i, m)); eng.check()
    assert eng.last_kernel() == kernel and _same_bits(on, off)
    eng.close()


# ---- 8. the other entry points ----------------------------------------------------------------------------------------------
def test_ingredient_form(torch_cuda):
    from oracle import m2d_oracle as oracle
    case = cases.grid_case(64, 0.5)
    rng = np.random.default_rng(2)
    R = 50
    ING = rng.standard_normal((R, 64)).astype(np.float32)
    off = np.zeros(I + 1, np.int32); off[1:] = np.cumsum(rng.integers(1, 6, I))
    ids = rng.integers(0, R, off[-1]).astype(np.int32)
    w = rng.uniform(0.5, 2.0, len(ids)).astype(np.float32)
    eng = _engine(case.PM, case.RE, case.CE, 0.5, mirror=True)
    ref_eng = _engine(case.PMr, case.RE, case.CE, 0.5)
    for e in (eng, ref_eng):
        e.set_ingredients(ING, off, ids, w)
    for B in (100, 8193):
        u, i, m = _dev(case.users[:B]), _dev(case.items[:B]), _dev(case.cats[:B])
        got, want = _host(eng.score_pairs_ingredients(u, i, m)), _host(ref_eng.score_pairs_ingredients(u, i, m))
        eng.check()
        assert eng.last_kernel() == _name(B <= 8192, hv=True) and ref_eng.last_kernel() == _name(B <= 8192, hv=True)[:-5]
        assert _same_bits(got, want), B
        ref = oracle.inference_ingredients(case.PMr, case.RE, ING, off, ids, w, case.users[:B], case.items[:B], case.cats[:B], 0.5)
        assert_scores_close(got, ref, what="ingredients B %d" % B)
    eng.close(); ref_eng.close()


@pytest.mark.parametrize("B", [51, 70000])
def test_host_form(torch_cuda, B):
    case = _loop_case(70000, 13)
    eng = _engine(case.PM, case.RE, case.CE, case.coef, mirror=True)
    ref_eng = _engine(case.PMr, case.RE, case.CE, case.coef)
    got = eng.score_pairs_host(case.users[:B], case.items[:B], case.cats[:B])
    assert eng.last_kernel() == _name(B <= 8192)
    assert _same_bits(got, ref_eng.score_pairs_host(case.users[:B], case.items[:B], case.cats[:B]))
    assert_scores_close(got, case.refs[0][:B], what="host B %d" % B)
    eng.close(); ref_eng.close()


# ---- 9. together with user_high_table ---------------------------------------------------------------------------------------
def test_mirror_wins_over_user_high_table(torch_cuda):
    B = 2 ** 18 + 77
    case = cases.grid_case(64, 0.5)
    rng = np.random.default_rng(9)
    users, items = rng.integers(0, U, B).astype(np.int32), rng.integers(0, I, B).astype(np.int32)
    eng = _engine(case.PM, case.RE, case.CE, 0.5, mirror=True, dish=case.by_dish)
    u, i = _dev(users), _dev(items)
    alone = _host(eng.score_pairs_bydish(u, i))
    assert eng.last_kernel() == _name(False)
    eng.set_option("user_high_table", 1)
    both = _host(eng.score_pairs_bydish(u, i)); eng.check()
    assert eng.last_kernel() == _name(False) and _same_bits(both, alone)
    eng.set_option("pm_bf16", 0)
    eng.score_pairs_bydish(u, i)
    assert eng.last_kernel() == "m2d_score_pairs_c4_uh"     # ... which is what runs at this size without the mirror
    eng.close()


# ---- 10. arguments ----------------------------------------------------------------------------------------------------------
def test_argument_checks(torch_cuda):
    from foodrec_amd import _native
    case = cases.grid_case(4, 0.5)
    eng = _engine(case.PM, case.RE, case.CE, 0.5)
    assert eng.get_option("pm_bf16") == 0
    for bad in (2, -1):
        with pytest.raises(ValueError):
            eng.set_option("pm_bf16", bad)
    assert eng.get_option("pm_bf16") == 0
    eng.set_option("pm_bf16", 1)
    assert eng.get_option("pm_bf16") == 1
    assert _native.lib().m2d_pm_bf16(eng._h, None, None) == _native.M2D_ERR_INVALID_ARG
    assert _native.lib().m2d_abi_version() == 2
    eng.close()
