"""Engine state through the C ABI: what a setter leaves behind when it refuses or fails, the option table, and teardown.

The calls go through ``_native.lib()`` with raw pointers: the Python wrapper would make several of these inputs legal (it copies to
an aligned tensor) or raise before the engine sees them.  Shapes are the smallest that exercise the state.

Not covered here, checked by reading ``csrc/m2d_abi.hip``: the setters' HIP-failure exits (an allocation would have to fail)."""
import ctypes

import numpy as np
import pytest
import torch

from foodrec_amd import _native
from foodrec_amd._native import (M2D_ERR_BAD_INGREDIENT, M2D_ERR_INVALID_ARG, M2D_ERR_NOT_CONFIGURED, M2D_OK, M2D_TABLES_DEVICE,
                                 M2D_TABLES_HOST)

pytestmark = pytest.mark.gpu

U, I, C, E, R = 8, 64, 4, 32, 16
K = (C + 1) * E
H1, H2 = 8, 4
B = 12
LEARNER_ADAM = 3
GROUP_MEAN = 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.int32).copy()


class Data:
    """One set of tables, masks, head, ingredient table and recipes, as numpy arrays; every test shares it and leaves it unchanged."""

    def __init__(self):
        rng = np.random.default_rng(20261021)
        f = lambda *s: (rng.standard_normal(s) / 8).astype(np.float32)
        self.pm, self.re, self.ce = f(U, C + 1, E), f(I, E), f(C, E)
        masks = rng.integers(0, 2, (I, C)).astype(np.float32)
        masks[masks.sum(1) == 0, 0] = 1.0
        self.masks = masks
        self.masks2 = np.ascontiguousarray(masks[::-1])              # another legal table: what a refused call offered
        self.users = rng.integers(0, U, B).astype(np.int32)
        self.items = rng.integers(0, I, B).astype(np.int32)
        self.cats = masks[self.items].copy()
        self.labels = rng.integers(0, 2, B).astype(np.float32)
        self.head = [f(K, H1), f(H1), f(H1, H2), f(H2), f(H2)]      # W1, b1, W2, b2, w3
        self.ing = f(R, E)
        self.off = (2 * np.arange(I + 1)).astype(np.int32)          # two ingredients a dish
        self.ids = rng.integers(0, R, 2 * I).astype(np.int32)


@pytest.fixture(scope="module")
def data():
    return Data()


class Engine:
    """A raw handle and the device tensors it borrows (kept alive here)."""

    def __init__(self, d, flags=M2D_TABLES_DEVICE):
        self.lib = _native.lib()
        self.keep = []
        self.h = ctypes.c_void_p()
        tabs = [self.table(t, flags) for t in (d.pm, d.re, d.ce)]
        rc = self.lib.m2d_create(*tabs, U, I, C, E, 0.99, 0, flags, ctypes.byref(self.h))
        assert rc == M2D_OK, _native.error_text(None)

    def table(self, a, flags):
        """What a setter takes for `a`: a device pointer (borrowed) or a host pointer (copied)."""
        if a is None:
            return None
        t = _dev(a) if flags == M2D_TABLES_DEVICE else np.ascontiguousarray(a)
        self.keep.append(t)
        return t.data_ptr() if flags == M2D_TABLES_DEVICE else t.ctypes.data

    def misaligned(self, a):
        """A device copy of `a` that starts 4 bytes into a tensor four floats longer."""
        t = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
        t[1:a.size + 1] = _dev(a.reshape(-1))
        self.keep.append(t)
        return t.data_ptr() + 4

    def text(self):
        return _native.error_text(self.h)

    def ok(self, rc):
        assert rc == M2D_OK, (rc, self.text())

    def check(self):
        return self.lib.m2d_check(self.h, None, None, None)

    def destroy(self):
        torch.cuda.synchronize()
        assert self.lib.m2d_destroy(self.h) == M2D_OK
        self.h = None

    # ---- setters
    def set_masks(self, a, flags=M2D_TABLES_DEVICE):
        return self.lib.m2d_set_dish_categories(self.h, self.table(a, flags), flags)

    def set_head(self, head, flags=M2D_TABLES_DEVICE, ptrs=None):
        p = ptrs or [self.table(a, flags) for a in head]
        return self.lib.m2d_set_mlp_head(self.h, *p, 0.25, H1, H2, flags)

    def set_ingredients(self, d, off=None, ids=None, flags=M2D_TABLES_DEVICE):
        off = d.off if off is None else off
        ids = d.ids if ids is None else ids
        return self.lib.m2d_set_ingredients(self.h, self.table(d.ing, flags), R, self.table(off, flags), self.table(ids, flags), None,
                                            ids.size, flags)

    def set_recipes(self, d, flags=M2D_TABLES_DEVICE):
        return self.lib.m2d_set_recipes(self.h, R, self.table(d.off, flags), self.table(d.ids, flags), d.ids.size, flags)

    # ---- calls; each returns (rc, outputs as int32 words)
    def pairs_call(self, fn, d, *extra):
        out = torch.zeros(B, dtype=torch.float32, device="cuda")
        users, items = _dev(d.users), _dev(d.items)                 # (alive until the call has run)
        rc = fn(self.h, users.data_ptr(), items.data_ptr(), *extra, B, out.data_ptr(), None)
        return rc, _words(out)

    def bydish(self, d):
        return self.pairs_call(self.lib.m2d_score_pairs_bydish, d)

    def pairs_mlp(self, d):
        return self.pairs_call(self.lib.m2d_score_pairs_mlp, d)

    def pairs(self, d):
        cats = _dev(d.cats)
        return self.pairs_call(self.lib.m2d_score_pairs, d, cats.data_ptr())

    def pairs_ingredients(self, d):
        return self.pairs_call(self.lib.m2d_score_pairs_ingredients, d, None)

    def pairs_host(self, d):
        out = np.zeros(B, np.float32)
        rc = self.lib.m2d_score_pairs_host(self.h, d.users.ctypes.data, d.items.ctypes.data, d.cats.ctypes.data, B, out.ctypes.data, None)
        return rc, out.view(np.int32).copy()

    def lists(self, fn, n, k, *args):
        """fn(h, *args, out_scores, out_ids, stream) -> (rc, score words | ids)"""
        s = torch.zeros(n, k, dtype=torch.float32, device="cuda")
        i = torch.zeros(n, k, dtype=torch.int32, device="cuda")
        rc = fn(self.h, *args, s.data_ptr(), i.data_ptr(), None)
        return rc, np.concatenate([_words(s), _words(i)], axis=1)

    def topk(self, k=5):
        users = _dev(np.arange(U, dtype=np.int32))
        return self.lists(self.lib.m2d_topk_users, U, k, users.data_ptr(), U, k)

    def topk_mlp(self, k=5):
        users = _dev(np.arange(U, dtype=np.int32))
        return self.lists(self.lib.m2d_topk_users_mlp, U, k, users.data_ptr(), U, k, 0)

    def rank_mlp(self, d):
        out = torch.zeros(B, dtype=torch.int32, device="cuda")
        users, items = _dev(d.users), _dev(d.items)
        rc = self.lib.m2d_catalogue_rank_mlp(self.h, users.data_ptr(), items.data_ptr(), B, None, None, out.data_ptr(), None, None)
        return rc, _words(out)

    def topk_markets(self, k=4):
        """two requests, each with the whole ingredient range as its market"""
        users = _dev(np.array([1, 6], np.int32))
        off = _dev(np.array([0, R, 2 * R], np.int64))
        ids = _dev(np.tile(np.arange(R, dtype=np.int32), 2))
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        s = torch.zeros(2, k, dtype=torch.float32, device="cuda")
        i = torch.zeros(2, k, dtype=torch.int32, device="cuda")
        rc = self.lib.m2d_topk_markets(self.h, users.data_ptr(), 2, off.data_ptr(), ids.data_ptr(), 2 * R, k, 0, s.data_ptr(), i.data_ptr(),
                                       counts.data_ptr(), None)
        return rc, np.concatenate([_words(s), _words(i)], axis=1)

    def train_begin(self):
        return self.lib.m2d_train_begin(self.h, LEARNER_ADAM, 0.001, 5.0, None)


# ---- 1. dish masks: a refused borrow leaves the previous table, or none

def test_dish_masks_refused_borrow_keeps_previous_table(data):
    e = Engine(data)
    e.ok(e.set_masks(data.masks))
    rc, before = e.bydish(data)
    e.ok(rc)
    assert e.lib.m2d_set_dish_categories(e.h, e.misaligned(data.masks2), M2D_TABLES_DEVICE) == M2D_ERR_INVALID_ARG
    assert "16-byte aligned" in e.text()
    rc, after = e.bydish(data)
    e.ok(rc)
    e.ok(e.check())
    assert np.array_equal(before, after)
    e.destroy()


def test_dish_masks_refused_borrow_on_fresh_engine_leaves_none(data):
    e = Engine(data)
    assert e.lib.m2d_set_dish_categories(e.h, e.misaligned(data.masks), M2D_TABLES_DEVICE) == M2D_ERR_INVALID_ARG
    assert e.bydish(data)[0] == M2D_ERR_NOT_CONFIGURED
    assert e.topk()[0] == M2D_ERR_NOT_CONFIGURED
    e.destroy()


# ---- 2. head: the same for W1 and for W2

@pytest.mark.parametrize("which", [0, 2], ids=["W1", "W2"])
def test_head_refused_borrow_keeps_previous_head(data, which):
    e = Engine(data)
    e.ok(e.set_masks(data.masks))
    e.ok(e.set_head(data.head))
    rc, before = e.pairs_mlp(data)
    e.ok(rc)
    other = [a[::-1].copy() for a in data.head]                     # another legal head: what the refused call offered
    ptrs = [e.table(a, M2D_TABLES_DEVICE) for a in other]
    ptrs[which] = e.misaligned(other[which])
    assert e.set_head(None, ptrs=ptrs) == M2D_ERR_INVALID_ARG
    assert "16-byte aligned" in e.text()
    rc, after = e.pairs_mlp(data)
    e.ok(rc)
    e.ok(e.check())
    assert np.array_equal(before, after)
    e.destroy()


@pytest.mark.parametrize("which", [0, 2], ids=["W1", "W2"])
def test_head_refused_borrow_on_fresh_engine_leaves_none(data, which):
    e = Engine(data)
    e.ok(e.set_masks(data.masks))
    e.ok(e.set_recipes(data))
    ptrs = [e.table(a, M2D_TABLES_DEVICE) for a in data.head]
    ptrs[which] = e.misaligned(data.head[which])
    assert e.set_head(None, ptrs=ptrs) == M2D_ERR_INVALID_ARG
    assert e.pairs_mlp(data)[0] == M2D_ERR_NOT_CONFIGURED
    assert e.topk_mlp()[0] == M2D_ERR_NOT_CONFIGURED
    assert e.rank_mlp(data)[0] == M2D_ERR_NOT_CONFIGURED
    e.ok(e.topk_markets()[0])                                       # not "the MLP head is set"
    e.ok(e.check())
    e.destroy()


# ---- 3. ingredients: a failure after replacement began leaves no table

def _bad_id(d):
    ids = d.ids.copy()
    ids[37] = R
    return dict(ids=ids)


def _not_csr(d):
    off = d.off.copy()
    off[9] = off[10] + 1
    return dict(off=off)


@pytest.mark.parametrize("spoil", [_bad_id, _not_csr], ids=["bad_id", "not_csr"])
def test_ingredients_failed_set_leaves_none(data, spoil):
    plain = Engine(data)                                            # never had ingredients
    plain.ok(plain.set_masks(data.masks))
    rc, want = plain.topk()
    plain.ok(rc)
    e = Engine(data)
    e.ok(e.set_masks(data.masks))
    e.ok(e.set_recipes(data))
    e.ok(e.set_ingredients(data))
    e.ok(e.pairs_ingredients(data)[0])
    assert e.set_ingredients(data, **spoil(data)) == M2D_ERR_BAD_INGREDIENT
    assert e.text().startswith("m2d_set_ingredients: ")
    assert e.pairs_ingredients(data)[0] == M2D_ERR_NOT_CONFIGURED
    e.ok(e.train_begin())                                           # not "the ingredient extension has no training step"
    e.ok(e.lib.m2d_train_end(e.h))
    e.ok(e.topk_markets()[0])                                       # not "the ingredient table is set"
    rc, got = e.topk()
    e.ok(rc)
    e.ok(e.check())
    assert np.array_equal(got, want)
    e.destroy()
    plain.destroy()


# ---- 4. options: the names, defaults and ranges of include/m2d.h, written out

WRITABLE = {            # name: (default, another legal value)
    "prefetch": (2, 4), "nt_loads": (1, 0), "blocks_per_cu": (8, 4), "variant": (0, 9), "topk_bf16x3": (1, 0), "topk_form": (0, 2),
    "topk_prune": (1, 0), "topk_block": (0, 128), "topk_refine": (1, 0), "topk_grouped": (1, 0), "topk_excl_tier": (0, 2),
    "market_shares": (0, 7), "topk_mlp_chunk_pairs": (1 << 22, 4096), "slate_chunk_pairs": (1 << 22, 4096),
    "deep_chunk_pairs": (1 << 22, 4096), "mlp_bf16x3": (1, 0), "mlp_form": (0, 1), "skip_masked": (1, 0), "user_high_table": (0, 1),
    "pm_bf16": (0, 1), "host_zero_copy": (2, 0),
}
RANGES = {              # name: (lowest, highest, the refusal's text)
    "market_shares": (0, 64, "m2d_set_option: market_shares takes 0 ... 64"),
    "topk_mlp_chunk_pairs": (256, 1 << 24, "m2d_set_option: topk_mlp_chunk_pairs takes 256 ... 2^24"),
    "slate_chunk_pairs": (256, 1 << 24, "m2d_set_option: slate_chunk_pairs takes 256 ... 2^24"),
    "deep_chunk_pairs": (256, 1 << 24, "m2d_set_option: deep_chunk_pairs takes 256 ... 2^24"),
    "pm_bf16": (0, 1, "m2d_set_option: pm_bf16 takes 0 or 1"),
}
READ_ONLY = {           # name: value on a fresh engine (None: the device's)
    "num_cu": None, "topk_block_users": 256, "market_shares_used": 0, "topk_mlp_launches": 0, "topk_repaired": 0, "topk_refined": 0,
    "topk_refine_repaired": 0, "topk_tiles_scanned": 0, "topk_tiles_full": 0, "topk_tiles_completed": -1, "rank_tiles_scanned": 0,
    "rank_resolved": 0, "topk_excl_short": 0, "topk_excl_tiles_scanned": 0,
}


def test_options(data):
    e = Engine(data)
    lib = e.lib

    def get(name):
        v = ctypes.c_int64(-12345)
        e.ok(lib.m2d_get_option(e.h, name.encode(), ctypes.byref(v)))
        return v.value

    def set_(name, value):
        return lib.m2d_set_option(e.h, name.encode(), value)

    for name, (default, other) in WRITABLE.items():
        assert get(name) == default, name
        e.ok(set_(name, default))
        assert get(name) == default, name
        e.ok(set_(name, other))
        assert get(name) == other, name
    for name, (lo, hi, text) in RANGES.items():
        held = get(name)
        for value in (lo - 1, hi + 1):
            assert set_(name, value) == M2D_ERR_INVALID_ARG, (name, value)
            assert e.text() == text
            assert get(name) == held, (name, value)
        for value in (lo, hi):
            e.ok(set_(name, value))
            assert get(name) == value, (name, value)
    for name, fresh in READ_ONLY.items():
        value = get(name)
        assert (value > 0) if fresh is None else (value == fresh), (name, value)
        assert set_(name, 1) == M2D_ERR_INVALID_ARG, name
        assert e.text() == "m2d_set_option: unknown option", name
        assert get(name) == value, name
    assert set_("no_such_option", 1) == M2D_ERR_INVALID_ARG
    assert e.text() == "m2d_set_option: unknown option"
    assert lib.m2d_get_option(e.h, b"no_such_option", ctypes.byref(ctypes.c_int64())) == M2D_ERR_INVALID_ARG
    e.destroy()


# ---- 5. lifecycle: every buffer grown once, everything cleared, a second engine in the same process

def _first_three(e, d):
    out = []
    for call in (e.pairs, e.pairs_host, e.bydish):
        rc, words = call(d)
        e.ok(rc)
        out.append(words)
    return out


def test_teardown_and_second_engine(data):
    d = data
    e = Engine(d, M2D_TABLES_HOST)                                  # the engine owns copies of everything it is given
    lib, h = e.lib, e.h
    e.ok(e.set_masks(d.masks, M2D_TABLES_HOST))
    first = _first_three(e, d)

    users = _dev(np.arange(U, dtype=np.int32))
    up, no = users.data_ptr(), None
    pu, pi, pc, pl = _dev(d.users), _dev(d.items), _dev(d.cats), _dev(d.labels)
    e.ok(e.topk()[0])                                               # pattern-grouped
    e.ok(lib.m2d_set_option(h, b"topk_grouped", 0))
    e.ok(e.topk()[0])                                               # dense
    e.ok(lib.m2d_set_option(h, b"topk_grouped", 1))
    xoff = _dev(2 * np.arange(U + 1, dtype=np.int64))
    xids = _dev(np.tile(np.array([3, 40], np.int32), U))
    e.ok(e.lists(lib.m2d_topk_users_excluding, U, 5, up, U, 5, xoff.data_ptr(), xids.data_ptr())[0])
    rank = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.ok(lib.m2d_catalogue_rank(h, pu.data_ptr(), pi.data_ptr(), B, no, no, rank.data_ptr(), no, no))
    slate = _dev(np.arange(0, I, 3, dtype=np.int32))
    nD = slate.numel()
    scores = torch.zeros(U, nD, dtype=torch.float32, device="cuda")
    e.ok(lib.m2d_score_slate(h, up, U, slate.data_ptr(), nD, scores.data_ptr(), no))
    e.ok(e.lists(lib.m2d_topk_slate, U, 5, up, U, slate.data_ptr(), nD, 5)[0])
    e.ok(e.lists(lib.m2d_topk_users_deep, U, 20, up, U, 20, no, no)[0])
    members = _dev(np.array([[0, 1, 2, -1], [5, -1, -1, -1]], np.int32))
    e.ok(e.lists(lib.m2d_topk_groups, 2, 20, members.data_ptr(), 2, 4, GROUP_MEAN, 20, no, no)[0])
    e.ok(e.set_recipes(d, M2D_TABLES_HOST))
    market = _dev(np.arange(R, dtype=np.int32))
    cook = torch.zeros(I, dtype=torch.int32, device="cuda")
    count = ctypes.c_int64(-1)
    e.ok(lib.m2d_cookable_dishes(h, market.data_ptr(), R, 0, cook.data_ptr(), no, ctypes.byref(count), no))
    assert count.value == I                                         # the whole ingredient range is at the market
    e.ok(e.topk_markets()[0])
    gm = _dev((np.random.default_rng(5).standard_normal((3, C + 1, E)) / 8).astype(np.float32))
    labels = _dev(np.array([[1, 0, 1], [0, 1, 0]], np.float32))
    batch = _native.ProfileBatch(users=None, labels=labels.data_ptr(), general_memory=gm.data_ptr(), n=2, L=3, alpha=0.5)
    e.ok(e.lists(lib.m2d_topk_profiles, 2, 5, ctypes.byref(batch), 5, no, no)[0])
    e.ok(e.set_head(d.head, M2D_TABLES_HOST))
    e.ok(e.pairs_mlp(d)[0])
    e.ok(e.topk_mlp()[0])
    e.ok(e.rank_mlp(d)[0])
    e.ok(lib.m2d_clear_mlp_head(h))
    e.ok(e.set_ingredients(d, flags=M2D_TABLES_HOST))
    e.ok(e.pairs_ingredients(d)[0])
    e.ok(lib.m2d_clear_ingredients(h))
    e.ok(e.train_begin())
    e.ok(lib.m2d_train_step(h, pu.data_ptr(), pi.data_ptr(), pc.data_ptr(), pl.data_ptr(), B, 1, no, no))
    e.ok(e.check())
    torch.cuda.synchronize()

    e.ok(lib.m2d_train_end(h))
    e.ok(lib.m2d_clear_recipes(h))
    e.ok(lib.m2d_clear_ingredients(h))
    e.ok(lib.m2d_clear_mlp_head(h))
    e.destroy()

    e2 = Engine(d, M2D_TABLES_HOST)
    e2.ok(e2.set_masks(d.masks, M2D_TABLES_HOST))
    second = _first_three(e2, d)
    e2.ok(e2.check())
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    e2.destroy()
