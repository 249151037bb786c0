"""PyTorch-ROCm custom ops over the C ABI (``include/m2d.h``).

torch is plumbing here -- device memory, streams, ``torch.distributed`` -- the arithmetic is in
``libm2d.so``.  Ops are registered for the ``cuda`` (= HIP on ROCm) device only: handing them CPU
tensors raises ``NotImplementedError``; there is no eager/CPU fallback to fall through to.
"""
from __future__ import annotations

import ctypes
import itertools
import weakref
from typing import Optional

import numpy as np
import torch

from . import _native

_ENGINES: "weakref.WeakValueDictionary[int, ScoringEngine]" = weakref.WeakValueDictionary()
_ENGINE_SERIAL = itertools.count(1)         # engine keys are never reused (id() of a collected engine can be)


GROUP_MODES = {"least": 0, "mean": 1, "most": 2}      # include/m2d.h: M2D_GROUP_LEAST / _MEAN / _MOST
GROUP_MAX_MEMBERS = 64                                 # include/m2d.h: M2D_GROUP_MAX_MEMBERS


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _dev_f32(x, device) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return t.to(device=device, dtype=torch.float32).contiguous()


def _int32_ids(x, what: str) -> np.ndarray:
    """ids -> int32 array; an id outside the int32 range raises IndexError (as recommender._ids does)."""
    a = np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x)
    if a.size == 0:
        return np.zeros(0, dtype=np.int32)
    if a.dtype.kind not in "iu":
        a = np.array(a, dtype=np.int64)
    a = a.astype(np.int64, copy=False).reshape(-1)
    if a.min() < -(2 ** 31) or a.max() >= 2 ** 31:
        raise IndexError("%s id does not fit int32" % what)
    return a.astype(np.int32)


def exclusion_csr(exclude, n: int):
    """Per-query exclusion lists -> (offsets int64[n + 1], ids int32[nnz]), ids ascending and distinct within each query.

    ``exclude``: a tuple ``(offsets, ids)``, or a list (any non-tuple sequence) of n id lists; ids in any order, repeats allowed.
    Vectorised: one lexsort."""
    if isinstance(exclude, tuple):
        off = np.asarray(exclude[0].cpu().numpy() if isinstance(exclude[0], torch.Tensor) else exclude[0], dtype=np.int64).reshape(-1)
        ids = _int32_ids(exclude[1], "excluded item")
        if off.size != n + 1 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != ids.size:
            raise ValueError("exclude: offsets must be non-decreasing from 0 to len(ids), n + 1 of them")
        lens = np.diff(off)
    else:
        lists = list(exclude)
        if len(lists) != n:
            raise ValueError("exclude: %d lists for %d queries" % (len(lists), n))
        lens = np.fromiter(map(len, lists), dtype=np.int64, count=n)
        ids = _int32_ids(np.fromiter(itertools.chain.from_iterable(lists), dtype=np.int64, count=int(lens.sum())), "excluded item")
    seg = np.repeat(np.arange(n, dtype=np.int64), lens)
    o = np.lexsort((ids, seg))
    seg, ids = seg[o], ids[o]
    keep = np.ones(ids.size, dtype=bool)
    keep[1:] = (seg[1:] != seg[:-1]) | (ids[1:] != ids[:-1])
    seg, ids = seg[keep], ids[keep]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(seg, minlength=n), out=off[1:])
    return off, np.ascontiguousarray(ids, dtype=np.int32)


def exclusions_on_device(exclude, n: int, device, what: str, as_is: bool = True, dtype_error=ValueError):
    """``exclude`` of the calls that leave out dishes per row -> device tensors (offsets int64[n + 1], ids int32), the one path of
    ``topk_users_excluding``, ``topk_users_mlp_excluding``, ``catalogue_rank`` and ``topk_markets_excluding``.

    ``as_is``: a pair of tensors already on ``device`` is taken as it is after the dtype and length checks (ascending within each
    segment: the kernels check it, ``check()`` reports); a wrong dtype raises ``dtype_error`` and a wrong number of offsets ValueError,
    both naming ``what``.  Anything else -- a list of n id lists, a host ``(offsets, ids)`` pair, and with ``as_is=False`` a device
    pair as well -- goes through ``exclusion_csr`` (sorted, de-duplicated, range-checked; a device pair is copied to the host, which
    synchronises).  ``catalogue_rank(head=False)`` is the one caller with ``as_is=False``: it has always sorted what it was given.

    No ids at all: a one-element dummy under all-zero totals, so that the ABI's "ids non-null when offsets are given" always holds."""
    device = torch.device(device)
    if as_is and isinstance(exclude, tuple) and len(exclude) == 2 and all(isinstance(t, torch.Tensor) and t.device == device for t in exclude):
        off, ids = exclude[0].contiguous().reshape(-1), exclude[1].contiguous().reshape(-1)
        if off.dtype != torch.int64 or ids.dtype != torch.int32:
            raise dtype_error("%s: device exclusions are (int64 offsets[%d], int32 ids)" % (what, n + 1))
        if off.numel() != n + 1:
            raise ValueError("%s: device exclusions are (int64 offsets[%d], int32 ids): exclusion offsets must have n + 1 = %d entries, "
                             "got %d" % (what, n + 1, n + 1, off.numel()))
    else:
        off_np, ids_np = exclusion_csr(exclude, n)
        off, ids = torch.from_numpy(off_np).to(device), torch.from_numpy(ids_np).to(device)
    if ids.numel() == 0:
        ids = torch.zeros(1, dtype=torch.int32, device=device)
    return off, ids


def topk_excluding_args(n_users: int, k, exclude):
    """Host-side argument checks of ``topk_users_excluding``: k in 1..16; ``exclude`` None, or a list of ``n_users`` id lists /
    an ``(offsets, ids)`` pair, which goes through ``exclusion_csr`` (sorted, de-duplicated, int32 range checked).
    Returns (offsets int64[n + 1], ids int32[nnz]) or (None, None)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 16:
        raise ValueError("topk_users_excluding: k must be an int in 1..16, got %r" % (k,))
    if exclude is None:
        return None, None
    return exclusion_csr(exclude, n_users)


class ScoringEngine:
    """Owns one ``m2d_engine`` and the HBM tables it borrows.

    Stands in for the variable set the reference builds in ``instantiate_weights``
    (Model_Recommender.py:43-54); ``user_base`` makes it one user-range shard.
    """

    def __init__(self, Personal_Memory, Recipe_Embedding, Category_Embedding, coef: float = 0.99,
                 device: Optional[torch.device] = None, user_base: int = 0):
        lib = _native.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("foodrec_amd needs an MI355X (no HIP device visible); there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.pm = _dev_f32(Personal_Memory, self.device)
        self.re = _dev_f32(Recipe_Embedding, self.device)
        self.ce = _dev_f32(Category_Embedding, self.device)
        if self.pm.dim() != 3 or self.re.dim() != 2 or self.ce.dim() != 2:
            raise ValueError("Personal_Memory [U, C+1, E], Recipe_Embedding [I, E], Category_Embedding [C, E] expected")
        self.U, c1, self.E = self.pm.shape
        self.I = self.re.shape[0]
        self.C = self.ce.shape[0]
        if c1 != self.C + 1 or self.re.shape[1] != self.E or self.ce.shape[1] != self.E:
            raise ValueError("table shapes disagree: PM %s, RE %s, CE %s" % (tuple(self.pm.shape), tuple(self.re.shape), tuple(self.ce.shape)))
        self.coef = float(np.float32(coef))
        self.dish_cats: Optional[torch.Tensor] = None
        handle = ctypes.c_void_p()
        rc = lib.m2d_create(self.pm.data_ptr(), self.re.data_ptr(), self.ce.data_ptr(), self.U, self.I, self.C,
                            self.E, self.coef, self.device.index or 0, _native.M2D_TABLES_DEVICE,
                            ctypes.byref(handle))
        _native.raise_for(rc, None)
        self._h = handle
        self._host_fn = lib.m2d_score_pairs_host
        self.user_base = 0
        if user_base:
            self.set_user_base(user_base)
        self.id = next(_ENGINE_SERIAL)
        _ENGINES[self.id] = self

    # -- configuration ---------------------------------------------------------------------------
    def set_user_base(self, user_base: int):
        _native.raise_for(_native.lib().m2d_set_user_base(self._h, int(user_base)), self._h)
        self.user_base = int(user_base)

    def set_dish_categories(self, cats):
        """cats: [I, C] (or [I, C, 1]) float mask per dish -- dish_to_category.json as a table."""
        t = _dev_f32(cats, self.device).reshape(self.I, self.C)
        _native.raise_for(_native.lib().m2d_set_dish_categories(self._h, t.data_ptr(), _native.M2D_TABLES_DEVICE), self._h)
        self.dish_cats = t

    def set_ingredients(self, ing_table, offsets, ids, weights=None):
        """Build-defined extension: multi-hot ingredient lists per dish in CSR form.
        ing_table [R, E]; offsets i32[I+1]; ids i32[nnz]; weights f32[nnz] or None (all ones)."""
        t = _dev_f32(ing_table, self.device)
        if t.dim() != 2 or t.shape[1] != self.E:
            raise ValueError("ingredient table must be [R, E=%d]" % self.E)
        as_i32 = lambda x: torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(
            device=self.device, dtype=torch.int32).contiguous()
        off, idt = as_i32(offsets), as_i32(ids)
        if off.numel() != self.I + 1:
            raise ValueError("offsets must have I + 1 = %d entries" % (self.I + 1))
        wt = _dev_f32(weights, self.device) if weights is not None else None
        if wt is not None and wt.numel() != idt.numel():
            raise ValueError("weights and ids differ in length")
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_set_ingredients(self._h, t.data_ptr(), t.shape[0], off.data_ptr(),
                                                   idt.data_ptr() if idt.numel() else None,
                                                   wt.data_ptr() if wt is not None else None, idt.numel(),
                                                   _native.M2D_TABLES_DEVICE)
        _native.raise_for(rc, self._h)
        self._ingredients = (t, off, idt, wt)          # keep the borrowed device buffers alive

    def clear_ingredients(self):
        _native.raise_for(_native.lib().m2d_clear_ingredients(self._h), self._h)
        self._ingredients = None

    def score_pairs_ingredients(self, users: torch.Tensor, items: torch.Tensor, cats: Optional[torch.Tensor] = None,
                                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Extension: high-level path from the ingredient table; cats=None -> resident dish masks."""
        self._check_ids(users, items)
        B = users.numel()
        users, items = users.contiguous(), items.contiguous()
        if cats is not None:
            if cats.numel() != B * self.C:
                raise ValueError("cats must be [B, C]")
            cats = cats.to(torch.float32).contiguous()
            if cats.data_ptr() % 16:
                cats = cats.clone()
        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_score_pairs_ingredients(self._h, users.data_ptr(), items.data_ptr(),
                                                           cats.data_ptr() if cats is not None else None, B,
                                                           out.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        return out

    def set_mlp_head(self, W1, b1, W2, b2, w3, b3: float):
        """Build-defined extension: score = reference + w3.relu(W2^T relu(W1^T z + b1) + b2) + b3."""
        K = (self.C + 1) * self.E
        t = [_dev_f32(x, self.device) for x in (W1, b1, W2, b2, w3)]
        H1, H2 = t[0].shape[1], t[2].shape[1]
        if tuple(t[0].shape) != (K, H1) or tuple(t[2].shape) != (H1, H2) or t[1].numel() != H1 or t[3].numel() != H2 or t[4].numel() != H2:
            raise ValueError("MLP head shapes: W1 [K=%d, H1], b1 [H1], W2 [H1, H2], b2 [H2], w3 [H2]" % K)
        rc = _native.lib().m2d_set_mlp_head(self._h, *(x.data_ptr() for x in t), float(b3), H1, H2, _native.M2D_TABLES_DEVICE)
        _native.raise_for(rc, self._h)
        self._mlp = t

    def clear_mlp_head(self):
        _native.raise_for(_native.lib().m2d_clear_mlp_head(self._h), self._h)
        self._mlp = None

    def score_pairs_mlp(self, users: torch.Tensor, items: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Extension: reference score + MLP head, masks from the resident dish table."""
        self._check_ids(users, items)
        B = users.numel()
        users, items = users.contiguous(), items.contiguous()
        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_score_pairs_mlp(self._h, users.data_ptr(), items.data_ptr(), B, out.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        return out

    def write_memory(self, users: torch.Tensor, items: torch.Tensor, cats: torch.Tensor, write_sign: torch.Tensor,
                     labels: torch.Tensor, general_memory: torch.Tensor, beta_1: float, beta_2: float, alpha: float,
                     want_means: bool = False, write_pm: bool = True, write_gm: bool = True):
        """Model.Write_Memory (Model_Recommender.py:106-220) as a scatter-add: updates self.pm (`write_pm`: the two
        chained Personal_Memory assigns the `personal` fetch depends on, :167 / :198) and `general_memory`
        ([L, C+1, E], device float32; `write_gm`: the assign the `general` fetch depends on, :215) IN PLACE.
        Returns (mean(PM), mean(GM)) when asked; the mean of a table that was not written is None."""
        if not (write_pm or write_gm):
            raise ValueError("write_memory: nothing to write")
        self._check_ids(users, items)
        B = users.numel()
        L = labels.shape[-1]
        if general_memory.device != self.device or general_memory.dtype != torch.float32 or not general_memory.is_contiguous():
            raise ValueError("general_memory must be a contiguous float32 tensor on %s" % self.device)
        if tuple(general_memory.shape) != (L, self.C + 1, self.E):
            raise ValueError("general_memory must be [L=%d, C+1, E]" % L)
        f = lambda t, n: t.to(device=self.device, dtype=torch.float32).reshape(B, n).contiguous()
        cats, write_sign, labels = f(cats, self.C), f(write_sign, 1), f(labels, L)
        sums = torch.zeros(2, dtype=torch.float64, device=self.device) if want_means else None
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_write_memory(self._h, users.contiguous().data_ptr(), items.contiguous().data_ptr(),
                                                cats.data_ptr(), write_sign.data_ptr(), labels.data_ptr(), B, L,
                                                general_memory.data_ptr(), float(beta_1), float(beta_2), float(alpha),
                                                (_native.M2D_WRITE_PERSONAL if write_pm else 0) |
                                                (_native.M2D_WRITE_GENERAL if write_gm else 0),
                                                sums.data_ptr() if want_means else None, _stream_ptr())
        _native.raise_for(rc, self._h)
        if want_means:
            self.check()
            s = sums.cpu().numpy()
            return (float(s[0] / self.pm.numel()) if write_pm else None,
                    float(s[1] / general_memory.numel()) if write_gm else None)
        return None

    # -- training step ----------------------------------------------------------
    LEARNERS = {"sgd": 0, "adagrad": 1, "rmsprop": 2, "adam": 3}

    def train_begin(self, learner: str = "adam", lr: float = 0.001, clip_norm: float = 5.0):
        """Model.train's optimizer choice (Model_Recommender.py:228-235): anything but adagrad / rmsprop / adam is
        gradient descent.  Allocates the optimizer slots; the three tables are updated in place from now on."""
        code = self.LEARNERS.get(str(learner).lower(), 0)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_train_begin(self._h, code, float(lr), float(clip_norm), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._training = True

    def train_step(self, users: torch.Tensor, items: torch.Tensor, cats: torch.Tensor, labels: torch.Tensor,
                   apply: bool = True) -> torch.Tensor:
        """One sess.run([loss_value, learning_rate, train_op]) (Train_recommender.py:189-199).  Returns a device
        float32[4]: loss, global gradient norm, clip scale, learning rate.  apply=False: loss / norm only."""
        self._check_ids(users, items)
        B = users.numel()
        # a step is two small launches at the reference's batch sizes: the wrapper's own cost counts.  Tensors that are
        # already what the kernel reads (contiguous float32 / int32 on the device) are passed as they are.
        ok = lambda t, n: (t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() and t.numel() == B * n)
        if not ok(cats, self.C):
            cats = cats.to(device=self.device, dtype=torch.float32).reshape(B, self.C).contiguous()
        if not ok(labels, 1):
            labels = labels.to(device=self.device, dtype=torch.float32).reshape(B, 1).contiguous()
        if not users.is_contiguous():
            users = users.contiguous()
        if not items.is_contiguous():
            items = items.contiguous()
        out = torch.empty(4, dtype=torch.float32, device=self.device)
        fn = _native.lib().m2d_train_step
        idx = self.device.index
        if _raw_stream is not None and _cur_device is not None and idx is not None and _cur_device() == idx:
            rc = fn(self._h, users.data_ptr(), items.data_ptr(), cats.data_ptr(), labels.data_ptr(), B, 1 if apply else 0,
                    out.data_ptr(), _raw_stream(idx))
        else:
            with torch.cuda.device(self.device):
                rc = fn(self._h, users.data_ptr(), items.data_ptr(), cats.data_ptr(), labels.data_ptr(), B, 1 if apply else 0,
                        out.data_ptr(), _stream_ptr())
        if rc:
            _native.raise_for(rc, self._h)
        return out

    def train_slot(self, table: int, slot: int, restore: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Optimizer slot `slot` of table 0 = PM, 1 = RE, 2 = CE (adam: m, v; adagrad: accumulator; rmsprop: rms,
        momentum) as a tensor shaped like the table; with `restore`, that tensor is written INTO the slot instead
        (checkpoint resume)."""
        ref = (self.pm, self.re, self.ce)[table]
        if restore is not None:
            buf = restore.to(device=self.device, dtype=torch.float32).contiguous()
            if buf.shape != ref.shape:
                raise ValueError("slot must be shaped like its table %s" % (tuple(ref.shape),))
        else:
            buf = torch.empty_like(ref)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_train_slot(self._h, int(table), int(slot), buf.data_ptr(), 0 if restore is None else 1,
                                              _stream_ptr())
        _native.raise_for(rc, self._h)
        return buf

    def tables_updated(self):
        """Call after writing to self.pm / self.re / self.ce directly (they are borrowed by the engine)."""
        _native.raise_for(_native.lib().m2d_tables_updated(self._h), self._h)

    def personal_memory_bf16(self) -> torch.Tensor:
        """The serving mirror of Personal_Memory (option "pm_bf16"): its round-to-nearest-even bfloat16 image [U, C+1, E], made
        current first -- built if a write made it stale -- whatever the option says.  For checkpointing a serving image."""
        buf = torch.empty(tuple(self.pm.shape), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_pm_bf16(self._h, buf.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        return buf

    def train_steps(self, restore: Optional[int] = None) -> int:
        """Optimizer steps applied since train_begin; with `restore`, sets that count (checkpoint resume)."""
        v = ctypes.c_int64(0 if restore is None else int(restore))
        _native.raise_for(_native.lib().m2d_train_steps(self._h, ctypes.byref(v), 0 if restore is None else 1), self._h)
        return int(v.value)

    def train_end(self):
        _native.raise_for(_native.lib().m2d_train_end(self._h), self._h)
        self._training = False

    def set_option(self, name: str, value: int):
        _native.raise_for(_native.lib().m2d_set_option(self._h, name.encode(), int(value)), self._h)

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64()
        _native.raise_for(_native.lib().m2d_get_option(self._h, name.encode(), ctypes.byref(v)), self._h)
        return int(v.value)

    def last_kernel(self) -> str:
        return (_native.lib().m2d_last_kernel(self._h) or b"").decode()

    # -- raw launches (device tensors in, device tensors out, no sync) -----------------------------
    def _check_ids(self, users: torch.Tensor, items: torch.Tensor):
        if users.dtype != torch.int32 or items.dtype != torch.int32:
            raise TypeError("ids must be int32 tensors (Model_Recommender.py:26-29)")
        if users.device != self.device or items.device != self.device:
            raise NotImplementedError("m2d ops run on %s only; got %s" % (self.device, users.device))

    def score_pairs(self, users: torch.Tensor, items: torch.Tensor, cats: torch.Tensor,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_ids(users, items)
        B = users.numel()
        if items.numel() != B or cats.numel() != B * self.C:
            raise ValueError("score_pairs: users[%d], items[%d], cats[%d] disagree (C=%d)" % (B, items.numel(), cats.numel(), self.C))
        users, items = users.contiguous(), items.contiguous()
        cats = cats.to(torch.float32).contiguous()
        if cats.data_ptr() % 16:
            cats = cats.clone()
        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_score_pairs(self._h, users.data_ptr(), items.data_ptr(), cats.data_ptr(), B,
                                               out.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        return out

    def score_pairs_host(self, users: np.ndarray, items: np.ndarray, cats: np.ndarray) -> np.ndarray:
        """Host arrays in, host array out (int32 [B], int32 [B], float32 [B, C] -> float32 [B]): the latency path for
        reference-shaped calls of a few dozen pairs.  Synchronous; raises IndexError for an out-of-range id."""
        users = np.ascontiguousarray(users, dtype=np.int32)
        items = np.ascontiguousarray(items, dtype=np.int32)
        cats = np.ascontiguousarray(cats, dtype=np.float32)
        B = users.shape[0]
        if items.shape != (B,) or cats.shape != (B, self.C):
            raise ValueError("users [B], items [B], cats [B, %d] expected" % self.C)
        out = np.empty(B, dtype=np.float32)
        ptr = lambda a: a.__array_interface__["data"][0]
        idx = self.device.index
        if _raw_stream is not None and _cur_device is not None and idx is not None and _cur_device() == idx:
            # a 51-pair call is a few tens of microseconds: skip the device guard and the Stream object when nothing needs them
            rc = self._host_fn(self._h, ptr(users), ptr(items), ptr(cats), B, ptr(out), _raw_stream(idx))
        else:
            with torch.cuda.device(self.device):
                rc = self._host_fn(self._h, ptr(users), ptr(items), ptr(cats), B, ptr(out), _stream_ptr())
        if rc:
            _native.raise_for(rc, self._h)
        return out

    def score_pairs_bydish(self, users: torch.Tensor, items: torch.Tensor,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_ids(users, items)
        B = users.numel()
        if items.numel() != B:
            raise ValueError("score_pairs_bydish: users and items differ in length")
        users, items = users.contiguous(), items.contiguous()
        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_score_pairs_bydish(self._h, users.data_ptr(), items.data_ptr(), B, out.data_ptr(),
                                                      _stream_ptr())
        _native.raise_for(rc, self._h)
        return out

    def rank_candidates(self, users: torch.Tensor, items: torch.Tensor, k: int,
                        lens: Optional[torch.Tensor] = None, head: bool = False):
        """users i32[nseg], items i32[nseg, L] -> (scores f32[nseg, k], items i32[nseg, k], flags i32[nseg]).
        `head`: the segments are scored under the MLP head (``m2d_rank_candidates_mlp``; needs ``set_mlp_head``)."""
        if items.dim() != 2 or users.numel() != items.shape[0]:
            raise ValueError("rank_candidates: items must be [nseg, L] with one user per row")
        self._check_ids(users, items)
        nseg, L = items.shape
        users, items = users.contiguous(), items.contiguous()
        if lens is not None:
            lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        out_s = torch.empty((nseg, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nseg, k), dtype=torch.int32, device=self.device)
        out_f = torch.empty((nseg,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            fn = _native.lib().m2d_rank_candidates_mlp if head else _native.lib().m2d_rank_candidates
            rc = fn(self._h, users.data_ptr(), items.data_ptr(), lens.data_ptr() if lens is not None else None, nseg, L, k,
                    out_s.data_ptr(), out_i.data_ptr(), out_f.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        return out_s, out_i, out_f

    def topk_users(self, users: torch.Tensor, k: int):
        """users i32[nU] -> (scores f32[nU, k], dish ids i32[nU, k]) over the whole catalogue."""
        nU = users.numel()
        out_s = torch.empty((nU, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nU, k), dtype=torch.int32, device=self.device)
        return self.topk_users_into(users, k, out_s, out_i)

    def topk_users_into(self, users: torch.Tensor, k: int, out_s: torch.Tensor, out_i: torch.Tensor):
        """topk_users into caller-owned contiguous buffers f32[nU, k] / i32[nU, k] (slices of a larger result)."""
        if users.dtype != torch.int32 or users.device != self.device:
            raise TypeError("topk_users: users must be an int32 tensor on %s" % self.device)
        users = users.contiguous()
        nU = users.numel()
        if (tuple(out_s.shape) != (nU, k) or tuple(out_i.shape) != (nU, k) or out_s.dtype != torch.float32 or
                out_i.dtype != torch.int32 or not out_s.is_contiguous() or not out_i.is_contiguous() or
                out_s.device != self.device or out_i.device != self.device):
            raise ValueError("topk_users_into: need contiguous f32[%d, %d] / i32[%d, %d] buffers on %s" % (nU, k, nU, k, self.device))
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_users(self._h, users.data_ptr(), nU, k, out_s.data_ptr(), out_i.data_ptr(),
                                              _stream_ptr())
        _native.raise_for(rc, self._h)
        return out_s, out_i

    def topk_users_mlp(self, users: torch.Tensor, k: int, candidates: int = 0):
        """``topk_users`` under the MLP head (``m2d_topk_users_mlp``, include/m2d.h): users i32[nU] -> (scores f32[nU, k],
        dish ids i32[nU, k]).  ``candidates`` = 0: every dish is scored under the head (exact); K1 = ``candidates`` >= k: the K1
        best by the reference score (``topk_users``) are reranked under the head.  Does not synchronise.  (Without each user's
        excluded dishes: ``topk_users_mlp_excluding``.)"""
        return self.topk_users_mlp_excluding(users, k, None, candidates)

    def topk_users_mlp_excluding(self, users: torch.Tensor, k: int, exclude=None, candidates: int = 0):
        """EXTENSION (``m2d_topk_users_mlp_excluding``, include/m2d.h): ``topk_users_mlp`` whose lists leave
        out users[i]'s excluded dishes -- ``exclude``: a list of nU id lists, a host ``(offsets, ids)`` pair (both through
        ``exclusion_csr``), or a pair of device tensors as is (``topk_users_excluding``'s forms); None: ``topk_users_mlp`` itself.
        Rows end in id -1 / NaN when fewer than k dishes remain; with exclusions K1 <= 16 and stage 1 is ``topk_users_excluding``.
        ``catalogue_rank(users[i], ids[i][j], exclude[i], head=True) == j`` for the exact mode's lists.  Does not synchronise."""
        if users.dtype != torch.int32 or users.device != self.device:
            raise TypeError("topk_users_mlp: users must be an int32 tensor on %s" % self.device)
        users = users.contiguous()
        nU, k, candidates = users.numel(), int(k), int(candidates)
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, nU, self.device, "topk_users_mlp_excluding")
        out_s = torch.empty((nU, max(k, 0)), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nU, max(k, 0)), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            if off is None:
                rc = _native.lib().m2d_topk_users_mlp(self._h, users.data_ptr(), nU, k, candidates, out_s.data_ptr(), out_i.data_ptr(),
                                                      _stream_ptr())
            else:
                rc = _native.lib().m2d_topk_users_mlp_excluding(self._h, users.data_ptr(), nU, k, candidates, off.data_ptr(),
                                                                ids.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._topk_mlp_keep = (users, off, ids)          # stay alive until the queued kernels have read them
        return out_s, out_i

    def _topk_deep(self, what: str, users: torch.Tensor, k: int, exclude, candidates: Optional[int]):
        if users.dtype != torch.int32 or users.device != self.device:
            raise TypeError("%s: users must be an int32 tensor on %s" % (what, self.device))
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 1024:
            raise ValueError("%s: 1 <= k <= 1024, got %r" % (what, k))
        users = users.contiguous().reshape(-1)
        nU, k = users.numel(), int(k)
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, nU, self.device, what)
        out_s = torch.empty((nU, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nU, k), dtype=torch.int32, device=self.device)
        xo, xi = (off.data_ptr(), ids.data_ptr()) if off is not None else (None, None)
        with torch.cuda.device(self.device):
            if candidates is None:
                rc = _native.lib().m2d_topk_users_deep(self._h, users.data_ptr(), nU, k, xo, xi, out_s.data_ptr(), out_i.data_ptr(), _stream_ptr())
            else:
                rc = _native.lib().m2d_topk_users_mlp_deep(self._h, users.data_ptr(), nU, k, int(candidates), xo, xi, out_s.data_ptr(),
                                                           out_i.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._deep_keep = (users, off, ids)              # stay alive until the queued kernels have read them
        return out_s, out_i

    def topk_users_deep(self, users: torch.Tensor, k: int, exclude=None):
        """EXTENSION (``m2d_topk_users_deep``, include/m2d.h): the first k of ``topk_users``' order over the
        whole catalogue for 1 <= k <= min(1024, I), leaving out users[i]'s excluded dishes -- ``exclude`` in ``topk_users_excluding``'s
        forms, None for none -> (scores f32[nU, k], dish ids i32[nU, k]).  A listed score is the word ``score_slate`` writes for that
        (user, dish); rows end in id -1 / NaN when fewer than k dishes remain.  Does not synchronise."""
        return self._topk_deep("topk_users_deep", users, k, exclude, None)

    def topk_users_mlp_deep(self, users: torch.Tensor, k: int, exclude=None, candidates: int = 0):
        """EXTENSION (``m2d_topk_users_mlp_deep``): ``topk_users_mlp_excluding`` for 1 <= k <= min(1024, I).
        ``candidates`` = 0 scores every dish under the head; k <= K1 = ``candidates`` <= min(1024, I) reranks ``topk_users_deep``'s K1
        dishes of each user and segment.  Does not synchronise."""
        return self._topk_deep("topk_users_mlp_deep", users, k, exclude, candidates)

    def _topk_menu(self, users: torch.Tensor, k: int, caps: torch.Tensor):
        """What ``torch.ops.m2d.topk_menu`` and ``Model.topk_menu`` call (not a public method: every public method of this class has a row
        in the stream-order table of tests/stream_cases.py, and this call has its own stream-order case in tests/test_gpu_menu.py).
        EXTENSION, build-defined (``m2d_topk_menu``, include/m2d.h): the first k dishes of ``topk_users``'
        order over the whole catalogue with at most caps[u][c] dishes of category c in user u's list -> (scores f32[nU, k], dish ids
        i32[nU, k]).  ``caps``: an int32 device tensor [nU, C], or [C] -- one row for every user, broadcast on the device.  1 <= k <= 64;
        rows end in id -1 / NaN where the caps leave fewer than k dishes.  The first call after the dish masks changed builds the
        signature index and waits for the stream once; otherwise it does not synchronise.  A cap below 0 surfaces from ``check()``."""
        if users.dtype != torch.int32 or users.device != self.device:
            raise TypeError("topk_menu: users must be an int32 tensor on %s" % self.device)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("topk_menu: 1 <= k <= 64, got %r" % (k,))
        if not isinstance(caps, torch.Tensor) or caps.dtype != torch.int32 or caps.device != self.device:
            raise TypeError("topk_menu: caps must be an int32 tensor on %s" % self.device)
        users = users.contiguous().reshape(-1)
        nU, k = users.numel(), int(k)
        if caps.dim() == 1 and caps.shape[0] == self.C:
            caps = caps.reshape(1, self.C).expand(nU, self.C)
        if caps.dim() != 2 or tuple(caps.shape) != (nU, self.C):
            raise ValueError("topk_menu: caps must be [%d, %d] or [%d], got %s" % (nU, self.C, self.C, tuple(caps.shape)))
        caps = caps.contiguous()
        out_s = torch.empty((nU, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nU, k), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_menu(self._h, users.data_ptr(), nU, k, caps.data_ptr(), out_s.data_ptr(), out_i.data_ptr(),
                                             _stream_ptr())
        _native.raise_for(rc, self._h)
        self._menu_keep = (users, caps)                  # stay alive until the queued kernels have read them
        return out_s, out_i

    def _topk_menu_filtered(self, users: torch.Tensor, k: int, caps: torch.Tensor, exclude=None, among=None):
        """What ``torch.ops.m2d.topk_menu_filtered`` and ``Model.topk_menu_filtered`` call (not a public method, for ``_topk_menu``'s
        reason; its stream-order case is in tests/test_gpu_menu_filtered.py).  EXTENSION, build-defined (``m2d_topk_menu_filtered``,
        include/m2d.h): ``_topk_menu`` over the dishes of ``among`` -- an int32 device tensor of STRICTLY
        ASCENDING dish ids, None: the whole catalogue -- less users[i]'s excluded dishes -- ``exclude``: an ``(offsets, ids)`` pair of
        device tensors as ``topk_users_deep`` takes it, or its host forms; None: none.  A dish that is left out counts against no cap.
        With a slate THE CALL WAITS FOR THE STREAM ONCE (the slate's 64 segment sizes decide the launches); without one it
        synchronises as ``_topk_menu`` does.  Bad lists surface from ``check()``."""
        what = "topk_menu_filtered"
        if users.dtype != torch.int32 or users.device != self.device:
            raise TypeError("%s: users must be an int32 tensor on %s" % (what, self.device))
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("%s: 1 <= k <= 64, got %r" % (what, k))
        if not isinstance(caps, torch.Tensor) or caps.dtype != torch.int32 or caps.device != self.device:
            raise TypeError("%s: caps must be an int32 tensor on %s" % (what, self.device))
        users = users.contiguous().reshape(-1)
        nU, k = users.numel(), int(k)
        if caps.dim() == 1 and caps.shape[0] == self.C:
            caps = caps.reshape(1, self.C).expand(nU, self.C)
        if caps.dim() != 2 or tuple(caps.shape) != (nU, self.C):
            raise ValueError("%s: caps must be [%d, %d] or [%d], got %s" % (what, nU, self.C, self.C, tuple(caps.shape)))
        caps = caps.contiguous()
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, nU, self.device, what)
        slate, nD = None, 0
        if among is not None:
            if not isinstance(among, torch.Tensor) or among.dtype != torch.int32 or among.device != self.device:
                raise TypeError("%s: among must be an int32 tensor on %s" % (what, self.device))
            slate = among.contiguous().reshape(-1)
            nD = slate.numel()
            if nD < 1:
                raise ValueError("%s: among must hold at least one dish" % what)
        out_s = torch.empty((nU, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nU, k), dtype=torch.int32, device=self.device)
        xo, xi = (off.data_ptr(), ids.data_ptr()) if off is not None else (None, None)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_menu_filtered(self._h, users.data_ptr(), nU, k, caps.data_ptr(), xo, xi,
                                                      slate.data_ptr() if slate is not None else None, nD, out_s.data_ptr(),
                                                      out_i.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._menu_filtered_keep = (users, caps, off, ids, slate)      # stay alive until the queued kernels have read them
        return out_s, out_i

    def _plan_menus(self, users: torch.Tensor, days: int, k: int, caps: torch.Tensor, plan_caps=None, exclude=None, among=None):
        """What ``torch.ops.m2d.plan_menus`` and ``Model.plan_menus`` call (not a public method, for ``_topk_menu``'s reason; its
        stream-order case is in tests/test_gpu_plan.py).  EXTENSION, build-defined (``m2d_plan_menus``, include/m2d.h; DESIGN.md section
        4.15): ``days`` menus of k dishes per user, no dish twice -- day d is ``_topk_menu_filtered`` with the dishes of the earlier
        days left out, under ``caps`` per day and ``plan_caps`` over the whole plan (both int32 device tensors [nU, C] or [C];
        ``plan_caps`` None: none) -> (scores f32[nU, days, k], dish ids i32[nU, days, k]), one scoring pass.  1 <= k <= 64, days >= 1,
        days * k <= 1024.  ``exclude`` / ``among`` and the synchronisation: as ``_topk_menu_filtered``."""
        what = "plan_menus"
        if users.dtype != torch.int32 or users.device != self.device:
            raise TypeError("%s: users must be an int32 tensor on %s" % (what, self.device))
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("%s: 1 <= k <= 64, got %r" % (what, k))
        if isinstance(days, bool) or not isinstance(days, (int, np.integer)) or int(days) < 1 or int(days) * int(k) > 1024:
            raise ValueError("%s: days >= 1 and days * k <= 1024, got days = %r, k = %r" % (what, days, k))
        users = users.contiguous().reshape(-1)
        nU, k, days = users.numel(), int(k), int(days)

        def table(t, name):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device:
                raise TypeError("%s: %s must be an int32 tensor on %s" % (what, name, self.device))
            if t.dim() == 1 and t.shape[0] == self.C:
                t = t.reshape(1, self.C).expand(nU, self.C)
            if t.dim() != 2 or tuple(t.shape) != (nU, self.C):
                raise ValueError("%s: %s must be [%d, %d] or [%d], got %s" % (what, name, nU, self.C, self.C, tuple(t.shape)))
            return t.contiguous()

        caps = table(caps, "caps")
        plan = table(plan_caps, "plan_caps") if plan_caps is not None else None
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, nU, self.device, what)
        slate, nD = None, 0
        if among is not None:
            if not isinstance(among, torch.Tensor) or among.dtype != torch.int32 or among.device != self.device:
                raise TypeError("%s: among must be an int32 tensor on %s" % (what, self.device))
            slate = among.contiguous().reshape(-1)
            nD = slate.numel()
            if nD < 1:
                raise ValueError("%s: among must hold at least one dish" % what)
        out_s = torch.empty((nU, days, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nU, days, k), dtype=torch.int32, device=self.device)
        xo, xi = (off.data_ptr(), ids.data_ptr()) if off is not None else (None, None)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_plan_menus(self._h, users.data_ptr(), nU, days, k, caps.data_ptr(),
                                              plan.data_ptr() if plan is not None else None, xo, xi,
                                              slate.data_ptr() if slate is not None else None, nD, out_s.data_ptr(), out_i.data_ptr(),
                                              _stream_ptr())
        _native.raise_for(rc, self._h)
        self._plan_keep = (users, caps, plan, off, ids, slate)         # stay alive until the queued kernels have read them
        return out_s, out_i

    def _slate_ids(self, users: torch.Tensor, slate: torch.Tensor, what: str):
        for t, name in ((users, "users"), (slate, "slate")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device:
                raise TypeError("%s: %s must be an int32 tensor on %s" % (what, name, self.device))
        return users.contiguous().reshape(-1), slate.contiguous().reshape(-1)

    def score_slate(self, users: torch.Tensor, slate: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """EXTENSION (``m2d_score_slate``, include/m2d.h): the score of every listed user for every dish of one shared slate --
        users i32[nU] (global ids, repeats allowed), slate i32[nD] strictly ascending dish ids -> f32[nU, nD], row-major.  Masks are
        the resident dish table.  Does not synchronise; bad ids and a slate that is not ascending surface from ``check()``."""
        users, slate = self._slate_ids(users, slate, "score_slate")
        nU, nD = users.numel(), slate.numel()
        if out is None:
            out = torch.empty((nU, nD), dtype=torch.float32, device=self.device)
        elif (tuple(out.shape) != (nU, nD) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device):
            raise ValueError("score_slate: out must be a contiguous f32[%d, %d] tensor on %s" % (nU, nD, self.device))
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_score_slate(self._h, users.data_ptr(), nU, slate.data_ptr(), nD, out.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._slate_keep = (users, slate)                # inputs stay alive until the queued kernels have read them
        return out

    def topk_slate(self, users: torch.Tensor, slate: torch.Tensor, k: int):
        """EXTENSION (``m2d_topk_slate``): the first k of ``topk_users``' order over the slate's dishes only -> (scores f32[nU, k],
        dish ids i32[nU, k]); a listed score is the word ``score_slate`` writes for that (user, dish).  Does not synchronise."""
        users, slate = self._slate_ids(users, slate, "topk_slate")
        nU, nD, k = users.numel(), slate.numel(), int(k)
        out_s = torch.empty((nU, max(k, 0)), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nU, max(k, 0)), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_slate(self._h, users.data_ptr(), nU, slate.data_ptr(), nD, k, out_s.data_ptr(), out_i.data_ptr(),
                                              _stream_ptr())
        _native.raise_for(rc, self._h)
        self._slate_keep = (users, slate)
        return out_s, out_i

    # -- household retrieval (include/m2d.h, "Household retrieval") --------------------------------------
    def _group_members(self, members, what: str) -> torch.Tensor:
        """``members`` of the group calls -> a contiguous int32 device tensor [nG, M]: a device tensor with -1 padding as it is, a list
        of id lists padded with -1 on the host (no list longer than 64)."""
        if isinstance(members, torch.Tensor):
            if members.dtype != torch.int32 or members.device != self.device or members.dim() != 2:
                raise TypeError("%s: members must be an int32 tensor [nG, M] on %s" % (what, self.device))
            return members.contiguous()
        lists = [list(g) for g in members]
        if any(len(g) > GROUP_MAX_MEMBERS for g in lists):
            raise ValueError("%s: a group has at most %d members" % (what, GROUP_MAX_MEMBERS))
        padded = np.full((len(lists), max([len(g) for g in lists] + [1])), -1, dtype=np.int32)
        for g, ids in enumerate(lists):
            padded[g, :len(ids)] = _int32_ids(ids, "user")
        return torch.from_numpy(padded).to(self.device)

    def topk_groups(self, members, k: int, mode: str = "least", exclude=None, among: Optional[torch.Tensor] = None):
        """EXTENSION, build-defined (``m2d_topk_groups`` / ``m2d_topk_groups_slate``, include/m2d.h): one list
        of k dishes per GROUP of users -> (scores f32[nG, k], dish ids i32[nG, k]).  ``members``: int32 device tensor [nG, M] with -1
        padding, or a list of id lists (at most 64 each).  ``mode``: "least" (least misery: a dish scores what its unhappiest member
        scores), "mean" or "most".  ``exclude``: per-group lists in ``topk_users_deep``'s forms; ``among``: an ascending int32 slate
        (device tensor) instead of the whole catalogue -- not both.  1 <= k <= 1024.  Does not synchronise."""
        if mode not in GROUP_MODES:
            raise ValueError("topk_groups: mode must be one of %s, got %r" % (sorted(GROUP_MODES), mode))
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 1024:
            raise ValueError("topk_groups: 1 <= k <= 1024, got %r" % (k,))
        if exclude is not None and among is not None:
            raise ValueError("topk_groups: `among` and `exclude` cannot be combined (take the ids out of the slate)")
        members = self._group_members(members, "topk_groups")
        nG, M = members.shape
        k = int(k)
        off = ids = slate = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, nG, self.device, "topk_groups")
        if among is not None:
            if not isinstance(among, torch.Tensor) or among.dtype != torch.int32 or among.device != self.device:
                raise TypeError("topk_groups: among must be an int32 tensor on %s" % self.device)
            slate = among.contiguous().reshape(-1)
        out_s = torch.empty((nG, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nG, k), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            if slate is None:
                xo, xi = (off.data_ptr(), ids.data_ptr()) if off is not None else (None, None)
                rc = _native.lib().m2d_topk_groups(self._h, members.data_ptr(), nG, M, GROUP_MODES[mode], k, xo, xi, out_s.data_ptr(),
                                                   out_i.data_ptr(), _stream_ptr())
            else:
                rc = _native.lib().m2d_topk_groups_slate(self._h, members.data_ptr(), nG, M, GROUP_MODES[mode], slate.data_ptr(),
                                                         slate.numel(), k, out_s.data_ptr(), out_i.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._group_keep = (members, off, ids, slate)    # stay alive until the queued kernels have read them
        return out_s, out_i

    def score_groups(self, members, slate: torch.Tensor, mode: str = "least") -> torch.Tensor:
        """EXTENSION, build-defined (``m2d_score_groups_slate``): every group's word for every dish of one ascending slate ->
        f32[nG, nD]; ``members`` and ``mode`` as in ``topk_groups``.  Does not synchronise."""
        if mode not in GROUP_MODES:
            raise ValueError("score_groups: mode must be one of %s, got %r" % (sorted(GROUP_MODES), mode))
        members = self._group_members(members, "score_groups")
        if not isinstance(slate, torch.Tensor) or slate.dtype != torch.int32 or slate.device != self.device:
            raise TypeError("score_groups: slate must be an int32 tensor on %s" % self.device)
        slate = slate.contiguous().reshape(-1)
        nG, M = members.shape
        out = torch.empty((nG, slate.numel()), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_score_groups_slate(self._h, members.data_ptr(), nG, M, GROUP_MODES[mode], slate.data_ptr(), slate.numel(),
                                                      out.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._group_keep = (members, None, None, slate)
        return out

    def _plan_groups(self, members, days: int, k: int, caps: torch.Tensor, plan_caps=None, mode: str = "least", exclude=None, among=None,
                     caps_per_member: bool = False):
        """What ``torch.ops.m2d.plan_groups`` and ``Model.plan_group`` call (not a public method, for ``_topk_menu``'s reason; its
        stream-order case is in tests/test_gpu_plan_groups.py).  EXTENSION, build-defined (``m2d_plan_groups``, include/m2d.h; DESIGN.md
        section 4.16): ``_plan_menus`` for GROUPS of users -- the dishes are ordered by the group's word under ``mode``
        (``score_groups``' word) -> (scores f32[nG, days, k], dish ids i32[nG, days, k]).  ``members`` / ``mode``: as ``topk_groups``.
        ``caps`` / ``plan_caps``: int32 device tensors [nG, C] or [C], one row per group; with ``caps_per_member`` [nG, M, C], one row
        per member slot -- the group's cap is the minimum over its real members (filler slots are never read).  ``exclude``: one list
        per group; ``among`` and the synchronisation: as ``_plan_menus``.  1 <= k <= 64, days >= 1, days * k <= 1024."""
        what = "plan_groups"
        if mode not in GROUP_MODES:
            raise ValueError("%s: mode must be one of %s, got %r" % (what, sorted(GROUP_MODES), mode))
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("%s: 1 <= k <= 64, got %r" % (what, k))
        if isinstance(days, bool) or not isinstance(days, (int, np.integer)) or int(days) < 1 or int(days) * int(k) > 1024:
            raise ValueError("%s: days >= 1 and days * k <= 1024, got days = %r, k = %r" % (what, days, k))
        members = self._group_members(members, what)
        nG, M = members.shape
        k, days, per_member = int(k), int(days), bool(caps_per_member)

        def table(t, name):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device:
                raise TypeError("%s: %s must be an int32 tensor on %s" % (what, name, self.device))
            if per_member:
                if tuple(t.shape) != (nG, M, self.C):
                    raise ValueError("%s: with caps_per_member %s must be [%d, %d, %d], got %s" % (what, name, nG, M, self.C, tuple(t.shape)))
                return t.contiguous()
            if t.dim() == 1 and t.shape[0] == self.C:
                t = t.reshape(1, self.C).expand(nG, self.C)
            if t.dim() != 2 or tuple(t.shape) != (nG, self.C):
                raise ValueError("%s: %s must be [%d, %d] or [%d], got %s" % (what, name, nG, self.C, self.C, tuple(t.shape)))
            return t.contiguous()

        caps = table(caps, "caps")
        plan = table(plan_caps, "plan_caps") if plan_caps is not None else None
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, nG, self.device, what)
        slate, nD = None, 0
        if among is not None:
            if not isinstance(among, torch.Tensor) or among.dtype != torch.int32 or among.device != self.device:
                raise TypeError("%s: among must be an int32 tensor on %s" % (what, self.device))
            slate = among.contiguous().reshape(-1)
            nD = slate.numel()
            if nD < 1:
                raise ValueError("%s: among must hold at least one dish" % what)
        out_s = torch.empty((nG, days, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nG, days, k), dtype=torch.int32, device=self.device)
        xo, xi = (off.data_ptr(), ids.data_ptr()) if off is not None else (None, None)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_plan_groups(self._h, members.data_ptr(), nG, M, GROUP_MODES[mode], days, k, caps.data_ptr(),
                                               plan.data_ptr() if plan is not None else None, 1 if per_member else 0, xo, xi,
                                               slate.data_ptr() if slate is not None else None, nD, out_s.data_ptr(), out_i.data_ptr(),
                                               _stream_ptr())
        _native.raise_for(rc, self._h)
        self._plan_groups_keep = (members, caps, plan, off, ids, slate)   # stay alive until the queued kernels have read them
        return out_s, out_i

    # -- market retrieval (include/m2d.h, "Market retrieval") -------------------------------------------
    def set_recipes(self, offsets, ids, num_ingredients: int):
        """EXTENSION (``m2d_set_recipes``): every dish's ingredient list, CSR -- offsets i32[I + 1], ids i32[nnz] in
        [0, num_ingredients).  Lists only, independent of ``set_ingredients``.  Validated once, here (synchronises): a malformed row
        pointer or an id out of range raises IndexError and leaves the recipes unset; a call refused before that -- a bad argument, an id
        error still latched from an earlier launch -- leaves the previous lists set and served."""
        off, idt = self._as_ids(offsets, "offset"), self._as_ids(ids, "ingredient")
        if off.numel() != self.I + 1:
            raise ValueError("offsets must have I + 1 = %d entries" % (self.I + 1))
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_set_recipes(self._h, int(num_ingredients), off.data_ptr(), idt.data_ptr() if idt.numel() else None,
                                               idt.numel(), _native.M2D_TABLES_DEVICE)
        # a call refused for its arguments, or for an id error latched earlier, leaves the previous lists in place -- and borrowed:
        # their tensors are let go of only once the engine holds the new ones
        _native.raise_for(rc, self._h)
        self._recipes = (off, idt)                       # keep the borrowed device buffers alive

    def clear_recipes(self):
        _native.raise_for(_native.lib().m2d_clear_recipes(self._h), self._h)
        self._recipes = None

    def cookable_dishes(self, market, max_missing: int = 0, return_missing: bool = False, out_ids: Optional[torch.Tensor] = None,
                        out_missing: Optional[torch.Tensor] = None):
        """EXTENSION (``m2d_cookable_dishes``): the dishes that can be cooked from `market` -- ingredient ids, an int32 device tensor
        or any id sequence, any order, repeats allowed, may be empty -- as an int32 device tensor [count] in strictly ascending order: a
        legal slate.  A dish is cookable iff its list is non-empty and at most `max_missing` of its list entries (every occurrence
        counted) are not in the market.  ``return_missing=True`` also returns int32 [I]: every dish's missing-entry count, -1 for an
        empty list.  `out_ids` / `out_missing`: caller-owned contiguous int32 [I] buffers to write into (the result is then a view of
        `out_ids`; words from `count` on are not written).

        SYNCHRONISES the current stream once, for the count; a market id out of range raises IndexError (value and index named) from
        this call.  No ``torch.library`` op is registered for it: the output length depends on the data, which a registered op's
        fake kernel cannot state."""
        market = self._as_ids(market, "ingredient")
        for t, name in ((out_ids, "out_ids"), (out_missing, "out_missing")):
            if t is not None and (t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or t.numel() != self.I):
                raise ValueError("cookable_dishes: %s must be a contiguous int32[%d] tensor on %s" % (name, self.I, self.device))
        if out_ids is None:
            out_ids = torch.empty(self.I, dtype=torch.int32, device=self.device)
        if out_missing is None and return_missing:
            out_missing = torch.empty(self.I, dtype=torch.int32, device=self.device)
        count = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_cookable_dishes(self._h, market.data_ptr() if market.numel() else None, market.numel(), int(max_missing),
                                                   out_ids.data_ptr(), out_missing.data_ptr() if out_missing is not None else None,
                                                   ctypes.byref(count), _stream_ptr())
        _native.raise_for(rc, self._h)
        ids = out_ids.reshape(-1)[:count.value]
        return (ids, out_missing) if return_missing else ids

    def topk_market(self, users, market, k: int, max_missing: int = 0):
        """EXTENSION: the k best dishes per user among those that can be cooked from `market` -- ``cookable_dishes``, then
        ``topk_slate`` over that list with min(k, count) -> (scores f32[nU, k], dish ids i32[nU, k], count).  Columns from `count` on
        hold NaN / -1 (``topk_users_excluding``'s convention when fewer than k dishes remain); count = 0 returns all NaN / -1 without
        calling the slate.  1 <= k <= 64.  The scoring step is ``topk_slate``'s, requirements and refusals unchanged: dish masks
        set, finite tables, no ingredient table, no MLP head.  Synchronises once (the count)."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("topk_market: k must be an int in 1..64, got %r" % (k,))
        users, k = self._as_ids(users, "user"), int(k)
        slate = self.cookable_dishes(market, max_missing)
        count, nU = slate.numel(), users.numel()
        if count >= k and nU:
            return self.topk_slate(users, slate, k) + (count,)
        out_s = torch.full((nU, k), float("nan"), dtype=torch.float32, device=self.device)
        out_i = torch.full((nU, k), -1, dtype=torch.int32, device=self.device)
        if count and nU:
            kk = min(k, count)
            s, i = self.topk_slate(users, slate, kk)
            out_s[:, :kk] = s
            out_i[:, :kk] = i
        return out_s, out_i, count

    def _markets_csr(self, markets, nQ: int):
        """`markets` of ``topk_markets`` as device tensors (offsets int64[nQ + 1], ids int32[nnzM]): a CSR pair of tensors or arrays,
        or a list of nQ id sequences"""
        if isinstance(markets, tuple) and len(markets) == 2 and isinstance(markets[0], (torch.Tensor, np.ndarray)):
            off, ids = markets                           # the CSR pair is a TUPLE of arrays; per-request sequences come in a list
            if isinstance(off, torch.Tensor):
                if off.dtype != torch.int64 or off.device != self.device:
                    raise TypeError("topk_markets: market offsets must be an int64 tensor on %s" % self.device)
                off = off.contiguous().reshape(-1)
            else:
                off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64).reshape(-1)).to(self.device)
            return off, self._as_ids(ids, "ingredient")
        if len(markets) != nQ:
            raise ValueError("topk_markets: %d markets for %d users" % (len(markets), nQ))
        lists = [_int32_ids(m.cpu().numpy() if isinstance(m, torch.Tensor) else m, "ingredient") for m in markets]
        off = np.zeros(nQ + 1, np.int64)
        np.cumsum([len(l) for l in lists], out=off[1:])
        ids = np.concatenate(lists).astype(np.int32) if lists and off[-1] else np.zeros(0, np.int32)
        return torch.from_numpy(off).to(self.device), torch.from_numpy(ids).to(self.device)

    def topk_markets(self, users, markets, k: int, max_missing: int = 0, return_counts: bool = False):
        """EXTENSION (``m2d_topk_markets``, include/m2d.h): one user, one market PER REQUEST -- request q is
        (users[q], markets[q]) -- filtered, scored and listed in one stream-ordered call.  `markets`: a CSR pair ``(offsets int64[nQ + 1],
        ids int32)`` of device tensors or arrays, or a list of nQ ingredient-id sequences (any order, repeats allowed, may be empty).
        Returns (scores f32[nQ, k], dish ids i32[nQ, k]) and, with ``return_counts``, counts i32[nQ]: row q holds the first
        min(k, count_q) dishes cookable from market q (``cookable_dishes``' definition) in ``topk_users``' order, NaN / -1 from column
        count_q on; count_q is the number of cookable dishes.  A listed score is the word ``score_pairs_bydish`` returns under
        ``variant`` = 9.  1 <= k <= 64.

        Does not synchronise: bad market ids (value and index in `ids`), bad user ids and malformed offsets surface from ``check()``."""
        users = self._as_ids(users, "user")
        nQ = users.numel()
        off, ids = self._markets_csr(markets, nQ)
        if off.numel() != nQ + 1:
            raise ValueError("topk_markets: market offsets must have nQ + 1 = %d entries" % (nQ + 1))
        k = int(k)
        out_s = torch.empty((nQ, max(k, 0)), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nQ, max(k, 0)), dtype=torch.int32, device=self.device)
        counts = torch.empty((nQ,), dtype=torch.int32, device=self.device) if return_counts else None
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_markets(self._h, users.data_ptr(), nQ, off.data_ptr(), ids.data_ptr() if ids.numel() else None,
                                                ids.numel(), k, int(max_missing), out_s.data_ptr(), out_i.data_ptr(),
                                                counts.data_ptr() if counts is not None else None, _stream_ptr())
        _native.raise_for(rc, self._h)
        self._markets_keep = (users, off, ids)           # inputs stay alive until the queued kernels have read them
        return (out_s, out_i, counts) if return_counts else (out_s, out_i)

    def topk_markets_excluding(self, users, markets, exclude=None, k: int = 10, max_missing: int = 0, return_counts: bool = False,
                               return_missing: bool = False):
        """EXTENSION (``m2d_topk_markets_excluding``, include/m2d.h): ``topk_markets`` that leaves out, per
        request, the dishes in `exclude` and can name what each listed dish lacks.  `exclude`: None, a list of nQ dish-id lists or an
        ``(offsets, ids)`` pair of arrays -- sorted and de-duplicated per request here, as ``catalogue_rank`` does --, or a pair of
        DEVICE tensors (offsets int64[nQ + 1], ids int32), taken as they are: ascending per segment, checked on the device.
        Returns (scores f32[nQ, k], dish ids i32[nQ, k]), then with ``return_counts`` counts i32[nQ] -- the cookable dishes that are
        not excluded --, then with ``return_missing`` missing i32[nQ, k, max_missing]: for listed dish [q, j] the ingredient ids of its
        list entries absent from market q, in list order, every occurrence, -1 from the number missing on.

        Does not synchronise: bad ids, lists that are not ascending and malformed offsets surface from ``check()``."""
        users = self._as_ids(users, "user")
        nQ = users.numel()
        off, ids = self._markets_csr(markets, nQ)
        if off.numel() != nQ + 1:
            raise ValueError("topk_markets_excluding: market offsets must have nQ + 1 = %d entries" % (nQ + 1))
        xoff = xids = None
        if exclude is not None:
            xoff, xids = exclusions_on_device(exclude, nQ, self.device, "topk_markets_excluding", dtype_error=TypeError)
        k, mm = int(k), int(max_missing)
        out_s = torch.empty((nQ, max(k, 0)), dtype=torch.float32, device=self.device)
        out_i = torch.empty((nQ, max(k, 0)), dtype=torch.int32, device=self.device)
        counts = torch.empty((nQ,), dtype=torch.int32, device=self.device) if return_counts else None
        missing = torch.empty((nQ, max(k, 0), max(mm, 0)), dtype=torch.int32, device=self.device) if return_missing else None
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_markets_excluding(
                self._h, users.data_ptr(), nQ, off.data_ptr(), ids.data_ptr() if ids.numel() else None, ids.numel(),
                xoff.data_ptr() if xoff is not None else None, xids.data_ptr() if xids is not None else None, k, mm,
                out_s.data_ptr(), out_i.data_ptr(), counts.data_ptr() if counts is not None else None,
                missing.data_ptr() if missing is not None and missing.numel() else None, _stream_ptr())
        _native.raise_for(rc, self._h)
        self._markets_keep = (users, off, ids, xoff, xids)   # inputs stay alive until the queued kernels have read them
        return (out_s, out_i) + ((counts,) if return_counts else ()) + ((missing,) if return_missing else ())

    # -- EXTENSION (no reference counterpart): serving from health labels ---------------------------------------
    def _profile_batch(self, labels, general_memory, users, alpha, what: str):
        """The ``m2d_profile_batch`` of a profile call and the tensors it points into: (batch, n, keep).  `labels`: a device or host
        [n, L] float array (``user_one_hot_label`` rows, any non-negative weights) or a LIST of n label-id lists, turned into one-hot
        rows here with L = general_memory.shape[0] (an id outside [0, L) raises IndexError); `users`: None (all guests) or n ids,
        -1 = guest."""
        gm = general_memory if isinstance(general_memory, torch.Tensor) else torch.as_tensor(np.asarray(general_memory, dtype=np.float32))
        gm = gm.to(device=self.device, dtype=torch.float32).contiguous()
        if gm.dim() != 3 or tuple(gm.shape[1:]) != (self.C + 1, self.E):
            raise ValueError("%s: general_memory must be [L, C+1=%d, E=%d], got %r" % (what, self.C + 1, self.E, tuple(gm.shape)))
        L = gm.shape[0]
        if isinstance(labels, list):
            rows = np.zeros((len(labels), L), dtype=np.float32)
            for q, ids in enumerate(labels):
                ids = np.asarray(ids, dtype=np.int64).reshape(-1)
                if ids.size and (ids.min() < 0 or ids.max() >= L):
                    raise IndexError("%s: label id outside [0, %d) in request %d" % (what, L, q))
                rows[q, ids] = 1.0
            labels = rows
        y = _dev_f32(labels, self.device)
        if y.dim() != 2 or y.shape[1] != L:
            raise ValueError("%s: labels must be [n, L=%d], got %r" % (what, L, tuple(y.shape)))
        n = y.shape[0]
        u = None
        if users is not None:
            u = self._as_ids(users, "user")
            if u.numel() != n:
                raise ValueError("%s: %d users for %d label rows" % (what, u.numel(), n))
        batch = _native.ProfileBatch(u.data_ptr() if u is not None and n else None, y.data_ptr() if n else gm.data_ptr(), gm.data_ptr(),
                                     n, L, float(alpha))
        return batch, n, (u, y, gm)

    def compose_profiles(self, labels, general_memory, users=None, alpha: float = 1.0) -> torch.Tensor:
        """EXTENSION (``m2d_compose_profiles``, include/m2d.h): the memory block of each profile (users[q], labels[q]) BY VALUE --
        f32[n, C+1, E], row q = base + alpha * (sum_l y_l GM[l]) / (sum_l y_l) with base = Personal_Memory[users[q]] or zeros for a
        guest (-1, or ``users=None``): what ``write_memory`` would add to the user's block, without writing it.  Does not synchronise;
        a request without labels (or with a non-finite row) gets zeros and surfaces from ``check()``."""
        batch, n, keep = self._profile_batch(labels, general_memory, users, alpha, "compose_profiles")
        out = torch.empty((n, self.C + 1, self.E), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_compose_profiles(self._h, ctypes.byref(batch), out.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._profiles_keep = keep                       # inputs stay alive until the queued kernels have read them
        return out

    def topk_profiles(self, labels, general_memory, k: int, users=None, alpha: float = 1.0, exclude=None):
        """EXTENSION (``m2d_topk_profiles``): ``topk_users`` -- with `exclude` ``topk_users_excluding``, k <= 16 -- for the composed
        rows of ``compose_profiles``: (scores f32[n, k], dish ids i32[n, k]), the words that call returns on an engine whose
        Personal_Memory is those rows.  `exclude` as in ``topk_users_excluding`` (``exclusions_on_device``).  Does not synchronise."""
        batch, n, keep = self._profile_batch(labels, general_memory, users, alpha, "topk_profiles")
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, n, self.device, "topk_profiles")
        k = int(k)
        out_s = torch.empty((n, max(k, 0)), dtype=torch.float32, device=self.device)
        out_i = torch.empty((n, max(k, 0)), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_profiles(self._h, ctypes.byref(batch), k, off.data_ptr() if off is not None else None,
                                                 ids.data_ptr() if ids is not None else None, out_s.data_ptr(), out_i.data_ptr(),
                                                 _stream_ptr())
        _native.raise_for(rc, self._h)
        self._profiles_keep = keep + (off, ids)
        return out_s, out_i

    def score_profiles(self, labels, general_memory, rows, items, users=None, alpha: float = 1.0) -> torch.Tensor:
        """EXTENSION (``m2d_score_profiles``): ``score_pairs_bydish`` over pairs (profile rows[b], dish items[b]) -> f32[B]; `rows`
        index the profiles of this call, one outside [0, n) surfaces as IndexError from ``check()``.  Does not synchronise."""
        batch, n, keep = self._profile_batch(labels, general_memory, users, alpha, "score_profiles")
        rows, items = self._as_ids(rows, "profile row"), self._as_ids(items, "item")
        B = rows.numel()
        if items.numel() != B:
            raise ValueError("score_profiles: rows and items differ in length")
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_score_profiles(self._h, ctypes.byref(batch), rows.data_ptr() if B else None,
                                                  items.data_ptr() if B else None, B, out.data_ptr() if B else None, _stream_ptr())
        _native.raise_for(rc, self._h)
        self._profiles_keep = keep + (rows, items)
        return out

    def topk_markets_profiles(self, labels, general_memory, markets, k: int = 10, users=None, alpha: float = 1.0, exclude=None,
                              max_missing: int = 0, return_counts: bool = False, return_missing: bool = False):
        """EXTENSION (``m2d_topk_markets_profiles``): ``topk_markets_excluding`` with request q = (profile q, markets[q]); `markets`,
        `exclude` and the returned tuple as there.  Does not synchronise."""
        batch, n, keep = self._profile_batch(labels, general_memory, users, alpha, "topk_markets_profiles")
        off, ids = self._markets_csr(markets, n)
        if off.numel() != n + 1:
            raise ValueError("topk_markets_profiles: market offsets must have n + 1 = %d entries" % (n + 1))
        xoff = xids = None
        if exclude is not None:
            xoff, xids = exclusions_on_device(exclude, n, self.device, "topk_markets_profiles", dtype_error=TypeError)
        k, mm = int(k), int(max_missing)
        out_s = torch.empty((n, max(k, 0)), dtype=torch.float32, device=self.device)
        out_i = torch.empty((n, max(k, 0)), dtype=torch.int32, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device) if return_counts else None
        missing = torch.empty((n, max(k, 0), max(mm, 0)), dtype=torch.int32, device=self.device) if return_missing else None
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_markets_profiles(
                self._h, ctypes.byref(batch), off.data_ptr(), ids.data_ptr() if ids.numel() else None, ids.numel(),
                xoff.data_ptr() if xoff is not None else None, xids.data_ptr() if xids is not None else None, k, mm,
                out_s.data_ptr(), out_i.data_ptr(), counts.data_ptr() if counts is not None else None,
                missing.data_ptr() if missing is not None and missing.numel() else None, _stream_ptr())
        _native.raise_for(rc, self._h)
        self._profiles_keep = keep + (off, ids, xoff, xids)
        return (out_s, out_i) + ((counts,) if return_counts else ()) + ((missing,) if return_missing else ())

    def catalogue_rank(self, users, items, exclude=None, head: bool = False):
        """Full-catalogue rank of held-out dishes (``m2d_catalogue_rank``, include/m2d.h): for each query (users[i], items[i]) the
        number of dishes ranked before items[i] in ``topk_users``' order, leaving out the query's excluded ids.

        ``exclude``: None, a tuple ``(offsets, ids)`` (CSR, offsets of length n + 1), or a list of n per-query id lists; either form
        is sorted and de-duplicated per query here -- a pair of DEVICE tensors too (``exclusions_on_device(as_is=False)``): it is
        copied to the host, which synchronises.  Returns device tensors (ranks i32[n], held-out scores f32[n]), otherwise without
        synchronising; out-of-range ids surface as IndexError from ``check()``.

        EXTENSION ``head=True`` (``m2d_catalogue_rank_mlp``): scores and order are ``topk_users_mlp``'s -- every
        dish is scored under the MLP head --, and a pair of device tensors is taken as ``exclude`` as it is (``as_is=True``: not
        sorted, not copied, checked on the device).  The two forms differ in this on purpose: ``head=False`` keeps what it always did."""
        users = self._as_ids(users, "user")
        items = self._as_ids(items, "item")
        n = users.numel()
        if items.numel() != n:
            raise ValueError("catalogue_rank: users[%d] and items[%d] disagree" % (n, items.numel()))
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, n, self.device, "catalogue_rank", as_is=head)
        ranks = torch.empty(n, dtype=torch.int32, device=self.device)
        scores = torch.empty(n, dtype=torch.float32, device=self.device)
        if n == 0:
            return ranks, scores
        with torch.cuda.device(self.device):
            call = _native.lib().m2d_catalogue_rank_mlp if head else _native.lib().m2d_catalogue_rank
            rc = call(self._h, users.data_ptr(), items.data_ptr(), n, off.data_ptr() if off is not None else None,
                      ids.data_ptr() if ids is not None else None, ranks.data_ptr(), scores.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._rank_keep = (users, items, off, ids)       # inputs stay alive until the queued kernels have read them
        return ranks, scores

    def topk_users_excluding(self, users, k: int, exclude=None):
        """``topk_users`` without each user's excluded dishes (``m2d_topk_users_excluding``, include/m2d.h): for users[i] the first k
        dishes of the ranking over the catalogue less ``exclude[i]``, in ``catalogue_rank``'s order and arithmetic -- for the same
        excluded set ``catalogue_rank(users[i], ids[i][j], exclude[i]) == j``.  Rows end in id -1 / NaN when fewer than k dishes remain.

        ``exclude``: None, a list of n per-user id lists or an ``(offsets, ids)`` pair (sorted, de-duplicated and range-checked on the
        host by ``exclusion_csr``) -- or, as is, a pair of device tensors (int64 offsets[n + 1], int32 ids, ascending within each
        segment: the kernels check it).  Returns device tensors (scores f32[n, k], ids i32[n, k]) without synchronising; bad ids
        and unsorted device segments surface from ``check()``."""
        users = self._as_ids(users, "user")
        n = users.numel()
        topk_excluding_args(n, k, None)                  # (k: checked before the lists, as ever)
        off = ids = None
        if exclude is not None:
            off, ids = exclusions_on_device(exclude, n, self.device, "topk_users_excluding")
        k = int(k)
        out_s = torch.empty((n, k), dtype=torch.float32, device=self.device)
        out_i = torch.empty((n, k), dtype=torch.int32, device=self.device)
        if n == 0:
            return out_s, out_i
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_topk_users_excluding(self._h, users.data_ptr(), n, k,
                                                        off.data_ptr() if off is not None else None,
                                                        ids.data_ptr() if ids is not None else None,
                                                        out_s.data_ptr(), out_i.data_ptr(), _stream_ptr())
        _native.raise_for(rc, self._h)
        self._excl_keep = (users, off, ids)              # inputs stay alive until the queued kernels have read them
        return out_s, out_i

    def _as_ids(self, x, what: str) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.int32:
                raise TypeError("%s ids must be int32 tensors" % what)
            if x.device != self.device:
                raise NotImplementedError("m2d ops run on %s only; got %s" % (self.device, x.device))
            return x.contiguous().reshape(-1)
        return torch.from_numpy(_int32_ids(x, what)).to(self.device)

    def stream_read_probe(self, buf: torch.Tensor, sink: torch.Tensor):
        """Calibration only: plain streaming read of `buf` (achievable HBM read rate of this box)."""
        nbytes = buf.numel() * buf.element_size()
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_stream_read_probe(self._h, buf.data_ptr(), nbytes - nbytes % 16, sink.data_ptr(),
                                                     _stream_ptr())
        _native.raise_for(rc, self._h)

    def check(self):
        """Synchronise the current stream; raise IndexError for an out-of-range id seen by a kernel."""
        bv, bi = ctypes.c_int64(), ctypes.c_int64()
        with torch.cuda.device(self.device):
            rc = _native.lib().m2d_check(self._h, _stream_ptr(), ctypes.byref(bv), ctypes.byref(bi))
        _native.raise_for(rc, self._h)

    def close(self):
        if getattr(self, "_h", None):
            _native.lib().m2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- torch.library registration -----------------------------------------------------------------
# The engine travels through the dispatcher as an integer key into _ENGINES.

def _engine(eid: int) -> ScoringEngine:
    try:
        return _ENGINES[eid]
    except KeyError:
        raise RuntimeError("m2d: engine %d is gone" % eid) from None


@torch.library.custom_op("m2d::score_pairs", mutates_args=(), device_types="cuda")
def score_pairs_op(engine: int, users: torch.Tensor, items: torch.Tensor, cats: torch.Tensor) -> torch.Tensor:
    return _engine(engine).score_pairs(users, items, cats)


@score_pairs_op.register_fake
def _(engine, users, items, cats):
    return users.new_empty(users.shape, dtype=torch.float32)


@torch.library.custom_op("m2d::score_pairs_bydish", mutates_args=(), device_types="cuda")
def score_pairs_bydish_op(engine: int, users: torch.Tensor, items: torch.Tensor) -> torch.Tensor:
    return _engine(engine).score_pairs_bydish(users, items)


@score_pairs_bydish_op.register_fake
def _(engine, users, items):
    return users.new_empty(users.shape, dtype=torch.float32)


@torch.library.custom_op("m2d::topk_users", mutates_args=(), device_types="cuda")
def topk_users_op(engine: int, users: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    return _engine(engine).topk_users(users, k)


@topk_users_op.register_fake
def _(engine, users, k):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32))


@torch.library.custom_op("m2d::topk_users_mlp", mutates_args=(), device_types="cuda")
def topk_users_mlp_op(engine: int, users: torch.Tensor, k: int, candidates: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    return _engine(engine).topk_users_mlp(users, k, candidates)


@topk_users_mlp_op.register_fake
def _(engine, users, k, candidates=0):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32))


@torch.library.custom_op("m2d::topk_users_mlp_excluding", mutates_args=(), device_types="cuda")
def topk_users_mlp_excluding_op(engine: int, users: torch.Tensor, k: int, candidates: int = 0, excl_off: Optional[torch.Tensor] = None,
                                excl_ids: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``ScoringEngine.topk_users_mlp_excluding``; `excl_off` / `excl_ids`: device tensors, ascending per segment, taken as they are."""
    exclude = None if excl_off is None else (excl_off, excl_ids if excl_ids is not None else excl_off.new_empty((0,), dtype=torch.int32))
    s, i = _engine(engine).topk_users_mlp_excluding(users, k, exclude, candidates)
    return s, i


@topk_users_mlp_excluding_op.register_fake
def _(engine, users, k, candidates=0, excl_off=None, excl_ids=None):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32))


def _excl_pair(excl_off, excl_ids):
    return None if excl_off is None else (excl_off, excl_ids if excl_ids is not None else excl_off.new_empty((0,), dtype=torch.int32))


def _deep_fake(users, k):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32))


@torch.library.custom_op("m2d::topk_users_deep", mutates_args=(), device_types="cuda")
def topk_users_deep_op(engine: int, users: torch.Tensor, k: int, excl_off: Optional[torch.Tensor] = None,
                       excl_ids: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``ScoringEngine.topk_users_deep``; `excl_off` / `excl_ids`: device tensors, ascending per segment, taken as they are."""
    s, i = _engine(engine).topk_users_deep(users, k, _excl_pair(excl_off, excl_ids))
    return s, i


@topk_users_deep_op.register_fake
def _(engine, users, k, excl_off=None, excl_ids=None):
    return _deep_fake(users, k)


@torch.library.custom_op("m2d::topk_menu", mutates_args=(), device_types="cuda")
def topk_menu_op(engine: int, users: torch.Tensor, caps: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION, build-defined (``m2d_topk_menu``, include/m2d.h): the engine-level menu call -- users i32[nU],
    caps i32[nU, C] or [C] (one row for every user), device tensors; 1 <= k <= 64 -> (scores f32[nU, k], dish ids i32[nU, k])."""
    s, i = _engine(engine)._topk_menu(users, k, caps)
    return s, i


@topk_menu_op.register_fake
def _(engine, users, caps, k):
    return _deep_fake(users, k)


@torch.library.custom_op("m2d::topk_menu_filtered", mutates_args=(), device_types="cuda")
def topk_menu_filtered_op(engine: int, users: torch.Tensor, caps: torch.Tensor, k: int, excl_off: Optional[torch.Tensor] = None,
                          excl_ids: Optional[torch.Tensor] = None, among: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION, build-defined (``m2d_topk_menu_filtered``, include/m2d.h): ``topk_menu`` over the strictly
    ascending dish ids of `among` (None: the catalogue) less each user's excluded dishes (`excl_off` / `excl_ids`: device tensors,
    ascending per segment, taken as they are)."""
    s, i = _engine(engine)._topk_menu_filtered(users, k, caps, _excl_pair(excl_off, excl_ids), among)
    return s, i


@topk_menu_filtered_op.register_fake
def _(engine, users, caps, k, excl_off=None, excl_ids=None, among=None):
    return _deep_fake(users, k)


@torch.library.custom_op("m2d::plan_menus", mutates_args=(), device_types="cuda")
def plan_menus_op(engine: int, users: torch.Tensor, caps: torch.Tensor, days: int, k: int, plan_caps: Optional[torch.Tensor] = None,
                  excl_off: Optional[torch.Tensor] = None, excl_ids: Optional[torch.Tensor] = None,
                  among: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION, build-defined (``m2d_plan_menus``, include/m2d.h): `days` menus of k dishes per user with no
    dish twice, `caps` per day and `plan_caps` over the plan (None: none); `excl_off` / `excl_ids` / `among` as
    ``topk_menu_filtered`` -> (scores f32[nU, days, k], dish ids i32[nU, days, k])."""
    s, i = _engine(engine)._plan_menus(users, days, k, caps, plan_caps, _excl_pair(excl_off, excl_ids), among)
    return s, i


@plan_menus_op.register_fake
def _(engine, users, caps, days, k, plan_caps=None, excl_off=None, excl_ids=None, among=None):
    return (users.new_empty((users.numel(), days, k), dtype=torch.float32),
            users.new_empty((users.numel(), days, k), dtype=torch.int32))


@torch.library.custom_op("m2d::topk_users_mlp_deep", mutates_args=(), device_types="cuda")
def topk_users_mlp_deep_op(engine: int, users: torch.Tensor, k: int, candidates: int = 0, excl_off: Optional[torch.Tensor] = None,
                           excl_ids: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``ScoringEngine.topk_users_mlp_deep``; the exclusions as above."""
    s, i = _engine(engine).topk_users_mlp_deep(users, k, _excl_pair(excl_off, excl_ids), candidates)
    return s, i


@topk_users_mlp_deep_op.register_fake
def _(engine, users, k, candidates=0, excl_off=None, excl_ids=None):
    return _deep_fake(users, k)


@torch.library.custom_op("m2d::catalogue_rank_mlp", mutates_args=(), device_types="cuda")
def catalogue_rank_mlp_op(engine: int, users: torch.Tensor, items: torch.Tensor, excl_off: Optional[torch.Tensor] = None,
                          excl_ids: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``ScoringEngine.catalogue_rank(head=True)``: (ranks i32[n], held-out scores f32[n]); the exclusions as above."""
    exclude = None if excl_off is None else (excl_off, excl_ids if excl_ids is not None else excl_off.new_empty((0,), dtype=torch.int32))
    r, s = _engine(engine).catalogue_rank(users, items, exclude, head=True)
    return r, s


@catalogue_rank_mlp_op.register_fake
def _(engine, users, items, excl_off=None, excl_ids=None):
    return (users.new_empty((users.numel(),), dtype=torch.int32),
            users.new_empty((users.numel(),), dtype=torch.float32))


@torch.library.custom_op("m2d::score_slate", mutates_args=(), device_types="cuda")
def score_slate_op(engine: int, users: torch.Tensor, slate: torch.Tensor) -> torch.Tensor:
    return _engine(engine).score_slate(users, slate)


@score_slate_op.register_fake
def _(engine, users, slate):
    return users.new_empty((users.numel(), slate.numel()), dtype=torch.float32)


@torch.library.custom_op("m2d::topk_slate", mutates_args=(), device_types="cuda")
def topk_slate_op(engine: int, users: torch.Tensor, slate: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    return _engine(engine).topk_slate(users, slate, k)


@topk_slate_op.register_fake
def _(engine, users, slate, k):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32))


@torch.library.custom_op("m2d::topk_groups", mutates_args=(), device_types="cuda")
def topk_groups_op(engine: int, members: torch.Tensor, k: int, mode: str = "least", excl_off: Optional[torch.Tensor] = None,
                   excl_ids: Optional[torch.Tensor] = None, among: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``ScoringEngine.topk_groups``; members i32[nG, M] with -1 padding; the exclusions as in ``topk_users_deep``."""
    s, i = _engine(engine).topk_groups(members, k, mode, _excl_pair(excl_off, excl_ids), among)
    return s, i


@topk_groups_op.register_fake
def _(engine, members, k, mode="least", excl_off=None, excl_ids=None, among=None):
    return (members.new_empty((members.shape[0], k), dtype=torch.float32),
            members.new_empty((members.shape[0], k), dtype=torch.int32))


@torch.library.custom_op("m2d::score_groups", mutates_args=(), device_types="cuda")
def score_groups_op(engine: int, members: torch.Tensor, slate: torch.Tensor, mode: str = "least") -> torch.Tensor:
    return _engine(engine).score_groups(members, slate, mode)


@score_groups_op.register_fake
def _(engine, members, slate, mode="least"):
    return members.new_empty((members.shape[0], slate.numel()), dtype=torch.float32)


@torch.library.custom_op("m2d::plan_groups", mutates_args=(), device_types="cuda")
def plan_groups_op(engine: int, members: torch.Tensor, caps: torch.Tensor, days: int, k: int, mode: str = "least",
                   plan_caps: Optional[torch.Tensor] = None, caps_per_member: bool = False, excl_off: Optional[torch.Tensor] = None,
                   excl_ids: Optional[torch.Tensor] = None, among: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """EXTENSION, build-defined (``m2d_plan_groups``, include/m2d.h): ``plan_menus`` for groups -- members
    i32[nG, M] with -1 padding, `caps` / `plan_caps` [nG, C] or, with `caps_per_member`, [nG, M, C] -> (scores f32[nG, days, k], dish
    ids i32[nG, days, k])."""
    s, i = _engine(engine)._plan_groups(members, days, k, caps, plan_caps, mode, _excl_pair(excl_off, excl_ids), among, caps_per_member)
    return s, i


@plan_groups_op.register_fake
def _(engine, members, caps, days, k, mode="least", plan_caps=None, caps_per_member=False, excl_off=None, excl_ids=None, among=None):
    return (members.new_empty((members.shape[0], days, k), dtype=torch.float32),
            members.new_empty((members.shape[0], days, k), dtype=torch.int32))


@torch.library.custom_op("m2d::catalogue_rank", mutates_args=(), device_types="cuda")
def catalogue_rank_op(engine: int, users: torch.Tensor, items: torch.Tensor, excl_off: Optional[torch.Tensor] = None,
                      excl_ids: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    exclude = None if excl_off is None else (excl_off, excl_ids)
    r, s = _engine(engine).catalogue_rank(users, items, exclude)
    return r, s


@catalogue_rank_op.register_fake
def _(engine, users, items, excl_off=None, excl_ids=None):
    return (users.new_empty((users.numel(),), dtype=torch.int32),
            users.new_empty((users.numel(),), dtype=torch.float32))


@torch.library.custom_op("m2d::topk_users_excluding", mutates_args=(), device_types="cuda")
def topk_users_excluding_op(engine: int, users: torch.Tensor, k: int, excl_off: Optional[torch.Tensor] = None,
                            excl_ids: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    exclude = None if excl_off is None else (excl_off, excl_ids)
    s, i = _engine(engine).topk_users_excluding(users, k, exclude)
    return s, i


@topk_users_excluding_op.register_fake
def _(engine, users, k, excl_off=None, excl_ids=None):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32))


@torch.library.custom_op("m2d::topk_markets", mutates_args=(), device_types="cuda")
def topk_markets_op(engine: int, users: torch.Tensor, market_off: torch.Tensor, market_ids: torch.Tensor, k: int,
                    max_missing: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``ScoringEngine.topk_markets`` with the counts: (scores f32[nQ, k], ids i32[nQ, k], counts i32[nQ]).  Unlike ``cookable_dishes``
    this call can be a registered op: its output shapes are static, so the fake kernel below states them."""
    return _engine(engine).topk_markets(users, (market_off, market_ids), k, max_missing, return_counts=True)


@topk_markets_op.register_fake
def _(engine, users, market_off, market_ids, k, max_missing=0):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32),
            users.new_empty((users.numel(),), dtype=torch.int32))


@torch.library.custom_op("m2d::topk_markets_excluding", mutates_args=(), device_types="cuda")
def topk_markets_excluding_op(engine: int, users: torch.Tensor, market_off: torch.Tensor, market_ids: torch.Tensor,
                              excl_off: Optional[torch.Tensor] = None, excl_ids: Optional[torch.Tensor] = None, k: int = 10,
                              max_missing: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``ScoringEngine.topk_markets_excluding`` with the counts and the missing entries: (scores f32[nQ, k], ids i32[nQ, k],
    counts i32[nQ], missing i32[nQ, k, max_missing]).  `excl_off` / `excl_ids`: device tensors, ascending per segment, taken as they
    are."""
    exclude = None if excl_off is None else (excl_off, excl_ids if excl_ids is not None else excl_off.new_empty((0,), dtype=torch.int32))
    return _engine(engine).topk_markets_excluding(users, (market_off, market_ids), exclude, k, max_missing, return_counts=True,
                                                  return_missing=True)


@topk_markets_excluding_op.register_fake
def _(engine, users, market_off, market_ids, excl_off=None, excl_ids=None, k=10, max_missing=0):
    return (users.new_empty((users.numel(), k), dtype=torch.float32),
            users.new_empty((users.numel(), k), dtype=torch.int32),
            users.new_empty((users.numel(),), dtype=torch.int32),
            users.new_empty((users.numel(), k, max_missing), dtype=torch.int32))


@torch.library.custom_op("m2d::compose_profiles", mutates_args=(), device_types="cuda")
def compose_profiles_op(engine: int, labels: torch.Tensor, general_memory: torch.Tensor, users: Optional[torch.Tensor] = None,
                        alpha: float = 1.0) -> torch.Tensor:
    """``ScoringEngine.compose_profiles``: labels f32[n, L], general_memory f32[L, C+1, E] -> rows f32[n, C+1, E]."""
    return _engine(engine).compose_profiles(labels, general_memory, users, alpha)


@compose_profiles_op.register_fake
def _(engine, labels, general_memory, users=None, alpha=1.0):
    return labels.new_empty((labels.shape[0],) + tuple(general_memory.shape[1:]), dtype=torch.float32)


@torch.library.custom_op("m2d::topk_profiles", mutates_args=(), device_types="cuda")
def topk_profiles_op(engine: int, labels: torch.Tensor, general_memory: torch.Tensor, k: int, users: Optional[torch.Tensor] = None,
                     alpha: float = 1.0, excl_off: Optional[torch.Tensor] = None,
                     excl_ids: Optional[torch.Tensor] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``ScoringEngine.topk_profiles``; `excl_off` / `excl_ids`: device tensors, ascending per segment, taken as they are."""
    exclude = None if excl_off is None else (excl_off, excl_ids if excl_ids is not None else excl_off.new_empty((0,), dtype=torch.int32))
    s, i = _engine(engine).topk_profiles(labels, general_memory, k, users, alpha, exclude)
    return s, i


@topk_profiles_op.register_fake
def _(engine, labels, general_memory, k, users=None, alpha=1.0, excl_off=None, excl_ids=None):
    return (labels.new_empty((labels.shape[0], k), dtype=torch.float32),
            labels.new_empty((labels.shape[0], k), dtype=torch.int32))
