"""Full-catalogue top-k with exclusions: what can be checked without a GPU (header, exports, signature row, argument checks)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "foodrec_amd", "libm2d.so")


def test_header_declares_and_library_exports_topk_users_excluding():
    hdr = open(os.path.join(ROOT, "include", "m2d.h")).read()
    assert re.search(r"int m2d_topk_users_excluding\(m2d_engine \*h, const int32_t \*users, int64_t nU, int32_t k,\s*"
                     r"const int64_t \*excl_off, const int32_t \*excl_ids,\s*float \*out_scores, int32_t \*out_ids, void \*stream\);", hdr)
    assert os.path.exists(LIB), "libm2d.so not built"
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bT m2d_topk_users_excluding\b", syms)


def test_signature_table_has_topk_users_excluding():
    src = open(os.path.join(ROOT, "foodrec_amd", "_native.py")).read()
    assert '"m2d_topk_users_excluding": (_c.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp])' in src


def test_abi_version_stays_2():
    from foodrec_amd import _native
    lib = _native.lib()
    assert lib.m2d_abi_version() == 2
    assert hasattr(lib, "m2d_topk_users_excluding")


def test_option_table_names_the_three_options():
    hdr = open(os.path.join(ROOT, "include", "m2d.h")).read()
    table = hdr[hdr.index("/* Options."):hdr.index("int m2d_set_option(")]
    for name in ("topk_excl_short", "topk_excl_tiles_scanned", "topk_excl_tier"):
        assert re.search(r"^ \* %s\s" % name, table, re.M), name


def test_argument_checks_need_no_device():
    from foodrec_amd.ops import topk_excluding_args
    for k in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError):
            topk_excluding_args(2, k, None)
    assert topk_excluding_args(2, 16, None) == (None, None)
    off, ids = topk_excluding_args(3, 1, [[4, 2, 4], [], [9]])
    assert off.tolist() == [0, 2, 2, 3] and ids.tolist() == [2, 4, 9]
    with pytest.raises(ValueError):
        topk_excluding_args(3, 10, [[1], [2]])                # two lists for three users
    with pytest.raises(IndexError):
        topk_excluding_args(1, 10, [[2 ** 31]])
    with pytest.raises(IndexError):
        topk_excluding_args(1, 10, [[-(2 ** 31) - 1]])


def test_model_topk_checks_its_arguments_before_it_touches_the_engine():
    import foodrec_amd
    m = object.__new__(foodrec_amd.Model)                     # no engine: every check below comes first
    for k in (0, 17):
        with pytest.raises(ValueError):
            m.topk([0, 1], k, exclude=[[1], [2]])
    with pytest.raises(ValueError):
        m.topk([0, 1], 10, exclude=[[1]])                     # one list for two users
    with pytest.raises(IndexError):
        m.topk([0], 10, exclude=[[2 ** 31]])
    with pytest.raises(IndexError):
        m.topk(["7"], 10, exclude={"7": [2 ** 40]})           # the dict form, keyed by the user as given
