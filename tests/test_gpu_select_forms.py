"""GPU tests of the two selection kernels behind m2d_launch_select (foodrec_amd/csrc/m2d_select.hip) on the SAME resident block, through
m2d_select_probe -- form 0: m2d_select_deep (k <= 1 024), form 1: m2d_topk_mlp_select (k <= 64).  Every list, ids as integers and scores
as 32-bit words, equals a plain sort by deep_cases.keys on the host; up to k = 64 the two forms also equal each other.

Shapes: 3 rows; W on both sides of select_threads' switches (256 | 257, 16 384 | 16 385), of the 64-lane slice (63, 64, 65), of the
walk's 256-column step (256 | 257) and of four steps of one wave (1 025); k = 1, min(W, 64) and, form 0, min(W, 1 024).  A block's rows:
one value throughout (the ids decide), NaNs (quiet ones and one with a payload: the word written is the word read) among normals and
infinities, both zeros among both signs.  Up to W = 1 500 the rows are deep_cases.adversarial_rows' ("one value", "tie group of 65",
"both signs, both zeros": their first W columns, the key turned back into a score word); a key folds -0 onto +0 and every NaN onto one,
so those are planted on the score words, as they are on the seeded normals of the wider blocks."""
import functools

import numpy as np
import pytest

import deep_cases as dc

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345                                          # a NaN no kernel computes; as an id: no dish
ROWS = 3
WIDTHS = (1, 63, 64, 65, 256, 257, 1025, 16384, 16385)
PAYLOAD = 0x7FC00123                                         # a NaN with a payload


def _scores_of(key):
    """the score words of real keys (dc.keys' high word undone; -0 and NaN payloads are not in a key)"""
    hi = (np.asarray(key, np.uint64) >> np.uint64(32)).astype(np.uint32)
    w = np.where(hi & np.uint32(0x80000000), hi, ~hi & np.uint32(0x7FFFFFFF))
    w = np.where(hi == np.uint32(0xFFFFFFFF), np.uint32(dc.NAN_WORD), w).astype(np.uint32)
    assert np.array_equal(dc.keys(w, np.arange(w.size)), key)
    return w.view(np.float32)


@functools.lru_cache(maxsize=None)
def _block(W):
    """(block float32 [3, W], its order: score words uint32 and ids int64 [3, min(W, 1024)]) -- computed once, read-only"""
    rng = np.random.default_rng(7000 + W)
    b = rng.standard_normal((ROWS, W)).astype(np.float32)
    b[0] = 0.0
    if W <= 1500:
        adv = {what: key for key, _, what in dc.adversarial_rows(np.random.default_rng(6))}
        b[0] = _scores_of(adv["one value"][:W])
        b[1] = _scores_of(adv["tie group of 65"][:W])
        b[2] = _scores_of(adv["both signs, both zeros"][:W])
    w = b.view(np.uint32)
    b[1, ::4] = np.nan
    w[1, ::8] = PAYLOAD
    b[1, 1::16] = np.inf
    b[1, 2::16] = -np.inf
    b[2, ::7] = 0.0
    b[2, 3::7] = -0.0
    assert np.unique(w[0]).size == 1 and np.isnan(b[1]).any() and (w[2] == 0x80000000).any() == (W > 3) and (w[2] == 0).any()
    want = dc.key_lists(b, min(W, dc.K_MAX))
    for a in (b, want[0], want[1]):
        a.setflags(write=False)
    return b, want


@pytest.fixture(scope="module")
def engine():
    from foodrec_amd import ScoringEngine
    r = dc.nan40_recipe()                                    # any engine: the probe reads the block alone
    eng = ScoringEngine(r.PM, r.RE, r.CE, coef=r.coef)
    yield eng
    eng.close()


def _probe(eng, block, k, form):
    """one m2d_select_probe call into poisoned [rows, k] buffers with a guard row on either side -> (score words, ids)"""
    import torch
    from foodrec_amd import _native
    from foodrec_amd.ops import _stream_ptr
    rows, W = block.shape
    bs = torch.full(((rows + 2) * k,), POISON, dtype=torch.int32, device="cuda")
    bi = torch.full(((rows + 2) * k,), POISON, dtype=torch.int32, device="cuda")
    rc = _native.lib().m2d_select_probe(eng._h, block.data_ptr(), rows, W, k, form, bs.data_ptr() + 4 * k, bi.data_ptr() + 4 * k, _stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (_native.lib().m2d_last_error(eng._h) or b"").decode()
    s, i = bs.cpu().numpy().view(np.uint32).reshape(rows + 2, k), bi.cpu().numpy().reshape(rows + 2, k)
    assert (s[[0, -1]] == POISON).all() and (i[[0, -1]] == POISON).all(), "a guard row was written"
    return s[1:-1], i[1:-1].astype(np.int64)


@pytest.mark.parametrize("W", WIDTHS)
def test_both_forms_list_the_block_in_key_order(engine, W):
    import torch
    b, want = _block(W)
    block = torch.as_tensor(b.copy(), device="cuda")
    got = {}
    for form, ks in ((0, (1, min(W, 64), min(W, 1024))), (1, (1, min(W, 64)))):
        for k in sorted(set(ks)):
            got[form, k] = _probe(engine, block, k, form)
            assert dc.same(got[form, k], (want[0][:, :k], want[1][:, :k])), (W, k, form)
    for k in sorted({1, min(W, 64)}):
        assert dc.same(got[0, k], got[1, k]), (W, k)
    assert np.array_equal(block.cpu().numpy().view(np.uint32), b.view(np.uint32))          # the block is read, never written
