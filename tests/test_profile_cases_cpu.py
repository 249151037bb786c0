"""CPU tests of the profile calls: the surface that can be checked without a GPU -- symbols, the ctypes struct,
the fake kernels -- and the test material of tests/test_gpu_profiles.py itself: float32 == float64 on every exact recipe, the bound's
conditions, the float32 restatement inside the bound and every stand-in outside it (tests/profile_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import profile_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("m2d_compose_profiles", "m2d_topk_profiles", "m2d_score_profiles", "m2d_topk_markets_profiles")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_four_entries_are_declared_bound_and_exported(native_lib):
    from foodrec_amd import _native
    header = _read("include", "m2d.h")
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header), "%s is not declared in include/m2d.h" % name
        assert name in _native.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "m2d_profile_batch" in header and not re.search(r"m2d_profile_batch\s*\(", header)
    assert native_lib.m2d_abi_version() == 2


def test_signatures_match_the_header_argument_counts():
    from foodrec_amd import _native
    header = re.sub(r"/\*.*?\*/", "", _read("include", "m2d.h"), flags=re.S)
    for name in ENTRIES:
        args = re.search(r"\bint %s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name


def test_the_makefile_builds_the_profile_kernels():
    assert re.search(r"^SRCS\s*:=.*\bm2d_profiles\.hip\b", _read("foodrec_amd", "csrc", "Makefile"), flags=re.M)
    src = _read("foodrec_amd", "csrc", "m2d_profiles.hip")
    assert "constexpr int MAXM = %d;" % pc.MAXM in src and "constexpr int KEEP = %d;" % pc.KEEP in src
    assert "fp contract(off)" in src


def test_the_batch_struct_is_forty_bytes_in_the_headers_order():
    from foodrec_amd import _native
    B = _native.ProfileBatch
    assert ctypes.sizeof(B) == 40
    assert [(f[0], getattr(B, f[0]).offset) for f in B._fields_] == [("users", 0), ("labels", 8), ("general_memory", 16), ("n", 24),
                                                                      ("L", 32), ("alpha", 36)]
    header = _read("include", "m2d.h")
    body = re.search(r"typedef struct \{([^}]*)\} m2d_profile_batch;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in B._fields_]


def test_null_handle_and_null_batch_are_refused_without_a_device(native_lib):
    from foodrec_amd import _native
    assert native_lib.m2d_compose_profiles(None, None, None, None) == _native.M2D_ERR_INVALID_ARG
    assert native_lib.m2d_topk_profiles(None, None, 1, None, None, None, None, None) == _native.M2D_ERR_INVALID_ARG
    assert native_lib.m2d_score_profiles(None, None, None, None, 0, None, None) == _native.M2D_ERR_INVALID_ARG
    assert native_lib.m2d_topk_markets_profiles(None, None, None, None, 0, None, None, 1, 0, None, None, None, None, None) == \
        _native.M2D_ERR_INVALID_ARG


def test_fake_kernels_state_the_shapes():
    import torch
    import foodrec_amd  # noqa: F401  (registers the ops)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        y = torch.empty((7, 95), dtype=torch.float32, device="cuda")
        gm = torch.empty((95, 5, 64), dtype=torch.float32, device="cuda")
        u = torch.empty((7,), dtype=torch.int32, device="cuda")
        rows = torch.ops.m2d.compose_profiles(1, y, gm, u, 0.5)
        assert tuple(rows.shape) == (7, 5, 64) and rows.dtype == torch.float32
        s, i = torch.ops.m2d.topk_profiles(1, y, gm, 10)
        assert tuple(s.shape) == (7, 10) == tuple(i.shape) and s.dtype == torch.float32 and i.dtype == torch.int32


def test_python_surface_exists():
    from foodrec_amd import Model, ScoringEngine
    for name in ("compose_profiles", "topk_profiles", "score_profiles", "topk_markets_profiles"):
        assert callable(getattr(ScoringEngine, name))
    assert callable(Model.topk_for_labels)


# ---- the test material ------------------------------------------------------------------------------------------------------------------
def _exact(shape):
    L, E, C, n, mode, base = shape
    return pc.exact_case(L, E, C, pc.second_trip_requests(256) if n is None else n, mode, base)


@pytest.mark.parametrize("shape", pc.EXACT_SHAPES)
def test_exact_recipes_are_exact_in_float32(shape):
    c = _exact(shape)
    r32 = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float32, c.user_base)
    r64 = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float64, c.user_base)
    assert r32.dtype == np.float32 and np.array_equal(r32.astype(np.float64), r64)
    assert np.isfinite(r64).all()
    ys = c.labels.sum(1)
    assert set(np.unique(c.labels)) <= {0.0, 0.5, 1.0, 2.0} and (np.log2(ys) % 1 == 0).all()
    assert c.alpha in pc.EXACT_ALPHAS
    if c.L > 64:
        assert c.labels[0, 64:].any(), "no label past the first mask word"
    assert c.labels[0, c.L - 1] != 0, "the last label is not addressed"


def test_exact_shapes_cover_what_the_kernel_branches_on():
    Ls, Es, Cs, ns = ({s[i] for s in pc.EXACT_SHAPES} for i in range(4))
    assert {1, 63, 64, 65, 95, 256, 257} <= Ls and {4, 6, 60, 64, 68, 200, 256} <= Es and {3, 4} <= Cs and {1, 4, 5, None} <= ns
    assert any(L > 64 * pc.MAXM for L in Ls) and any(E % 4 for E in Es)
    # a lane keeps KEEP columns between test and store; wider rows compute the rest twice: one such row in either form
    assert any((s[2] + 1) * s[1] > 4 * 64 * pc.KEEP for s in pc.EXACT_SHAPES if s[1] % 4 == 0), "no float4 row past the kept columns"
    assert any((s[2] + 1) * s[1] > 64 * pc.KEEP for s in pc.EXACT_SHAPES if s[1] % 4), "no scalar-path row past the kept columns"
    assert {s[4] for s in pc.EXACT_SHAPES} == {"null", "mixed", "known"} and 7000 in {s[5] for s in pc.EXACT_SHAPES}
    assert {pc.EXACT_ALPHAS[(s[0] + s[1]) % 3] for s in pc.EXACT_SHAPES} == set(pc.EXACT_ALPHAS)
    assert pc.second_trip_requests(256) == 8195


@pytest.mark.parametrize("shape", pc.NORMAL_SHAPES)
def test_float32_restatement_is_inside_the_bound(shape):
    c = pc.normal_case(*shape)
    assert pc.bound_conditions(c.labels, c.alpha)
    r32 = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float32, c.user_base)
    r64 = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float64, c.user_base)
    b = pc.bound(c.PM, c.GM, c.labels, c.users, c.alpha, c.user_base)
    assert (np.abs(r32.astype(np.float64) - r64) <= b).all()
    assert (r32.astype(np.float64) != r64).any(), "nothing rounds: this is no normal case"


def test_the_bound_states_its_conditions():
    c = pc.normal_case(*pc.NORMAL_SHAPES[0])
    assert pc.bound_conditions(c.labels, c.alpha)
    neg = c.labels.copy()
    neg[0, np.flatnonzero(neg[0])[0]] *= -1
    assert not pc.bound_conditions(neg, c.alpha)
    assert not pc.bound_conditions(np.zeros_like(c.labels), c.alpha)
    assert not pc.bound_conditions(c.labels, float("inf"))


@pytest.mark.parametrize("standin", pc.STANDINS)
def test_every_standin_changes_every_case_aimed_at_it(standin):
    shapes = pc.aimed_at(standin)
    assert shapes
    for shape in shapes:
        c = pc.normal_case(*shape)
        r64 = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float64, c.user_base)
        wrong = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float32, c.user_base, standin=standin)
        if standin == "fused":       # one rounding fewer stays inside any rounding bound: the witness against Write_Memory compares words
            r32 = pc.restate(c.PM, c.GM, c.labels, c.users, c.alpha, np.float32, c.user_base)
            assert not np.array_equal(wrong.view(np.uint32), r32.view(np.uint32)), shape
        else:
            b = pc.bound(c.PM, c.GM, c.labels, c.users, c.alpha, c.user_base)
            assert (np.abs(wrong.astype(np.float64) - r64) > b).any(), (standin, shape)


def test_served_case_material():
    for I in pc.CATALOGUES:
        c = pc.served_case(I)
        assert set(np.unique(c.cats)) <= {0.0, 1.0} and (c.cats.sum(1) >= 1).all()
        assert [len(x) for x in c.exclude] == list(pc.EXCL_LENS) and all((np.diff(x) > 0).all() for x in c.exclude)
        assert c.off[-1] == len(c.ids) and c.ids.max() < c.R
        assert (c.users == -1).any() and (c.users >= 0).any()
    assert 64 in pc.SERVED_KS and max(pc.SERVED_KS) <= min(pc.CATALOGUES)
