"""Full-catalogue rank: what can be checked without a GPU (header, exports, the exclusion CSR, argument checks)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_catalogue_rank():
    hdr = open(os.path.join(ROOT, "include", "m2d.h")).read()
    assert re.search(r"int m2d_catalogue_rank\(m2d_engine \*h, const int32_t \*users, const int32_t \*items, int64_t n,", hdr)
    lib = os.path.join(ROOT, "foodrec_amd", "libm2d.so")
    if not os.path.exists(lib):
        pytest.skip("libm2d.so not built")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bT m2d_catalogue_rank\b", syms)


def test_signature_table_has_catalogue_rank():
    src = open(os.path.join(ROOT, "foodrec_amd", "_native.py")).read()
    assert '"m2d_catalogue_rank": (_c.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp])' in src


def test_exclusion_csr_sorts_dedups_and_range_checks():
    from foodrec_amd.ops import exclusion_csr
    off, ids = exclusion_csr([[5, 3, 5, 1], [], [7, 7], [2]], 4)
    assert off.tolist() == [0, 3, 3, 4, 5]
    assert ids.tolist() == [1, 3, 5, 7, 2]
    assert ids.dtype == np.int32 and off.dtype == np.int64
    off2, ids2 = exclusion_csr((np.array([0, 4, 4, 6, 7]), np.array([5, 3, 5, 1, 7, 7, 2])), 4)
    assert off2.tolist() == off.tolist() and ids2.tolist() == ids.tolist()
    with pytest.raises(IndexError):
        exclusion_csr([[2 ** 31]], 1)
    with pytest.raises(IndexError):
        exclusion_csr([[-(2 ** 31) - 1]], 1)
    with pytest.raises(ValueError):
        exclusion_csr([[1], [2]], 3)
    with pytest.raises(ValueError):
        exclusion_csr((np.array([0, 2]), np.array([1])), 1)


def test_evaluate_model_full_rejects_bad_k():
    import foodrec_amd
    for K in (0, -3, 1.5, True):
        with pytest.raises(ValueError):
            foodrec_amd.evaluate_model_full(None, None, {"0": [1]}, None, K, {})
