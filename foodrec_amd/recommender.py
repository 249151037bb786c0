"""Host-side mirror of the reference's model-build / predict surface.

Reference: ``Code/Recommender/Model_Recommender.py`` (``Model.__init__`` :5-41, ``inference`` :56-97)
and its one call site ``sess.run([model.logits], feed_dict)`` (``evaluate.py:55-59``).  The same
constructor signature and attribute names are kept so reference-style driver code reads the same;
the graph itself is replaced by one fused HIP kernel behind ``include/m2d.h``.

The forward (scoring) path is the product.  The training-side fetches of the
reference's driver (Train_recommender.py:180-199) -- ``loss_value``, ``learning_rate``, ``train_op``
(Model_Recommender.py:99-104, :223-241; section 8f row N4) and ``personal`` / ``general``
(``Write_Memory``, :106-220; row N2) -- are served by the same engine through ``Session.run``.
"""
from __future__ import annotations

import itertools
from typing import Optional, Sequence

import numpy as np
import torch

from .ops import ScoringEngine


class _Placeholder:
    """Stands where the reference has a ``tf.placeholder`` (Model_Recommender.py:26-35): a feed_dict key."""

    def __init__(self, name: str, used: bool):
        self.name = name
        self.affects_logits = used

    def __repr__(self):
        return "<placeholder %s>" % self.name


class _ScalarFetch(float):
    """``model.learning_rate``: a number (args.lr) that can also be named in ``sess.run`` fetches
    (Model_Recommender.py:11, :227; Train_recommender.py:190)."""


class _Fetch:
    def __init__(self, name: str):
        self.name = name

    def __repr__(self):
        return "<fetch %s>" % self.name


def _ids(x, what: str) -> np.ndarray:
    """int32 feed conversion; ids reach the reference as Python ``str`` keys (evaluate.py:28, :41)."""
    if isinstance(x, torch.Tensor):
        return x
    if isinstance(x, np.ndarray) and x.dtype.kind in "iu":
        a = x.astype(np.int64, copy=False).reshape(-1)
    else:
        try:
            a = np.array(x, dtype=np.int64).reshape(-1)     # ints and decimal strings alike, one C loop
        except (ValueError, TypeError, OverflowError):
            a = np.fromiter((int(v) for v in x), dtype=np.int64, count=len(x))
    if a.size and (a.min() < -(2 ** 31) or a.max() >= 2 ** 31):
        raise IndexError("%s id does not fit int32" % what)
    return a.astype(np.int32)


def _exclusion_lists(exclude, users, what: str) -> list:
    """`exclude` of `topk`, `topk_head`, `topk_markets_excluding` and the full evaluation -> one id list per user: a dict is read
    by the user as given in `users` (a missing key excludes nothing), a list has to be aligned with `users`."""
    if isinstance(exclude, dict):
        return [exclude.get(u, ()) for u in users]
    if len(exclude) != len(users):
        raise ValueError("%s: %d exclusion lists for %d users" % (what, len(exclude), len(users)))
    return list(exclude)


def _mask(categories, C: int, B: int):
    """[B, C, 1] nested lists (dish_to_category.json values, evaluate.py:43) or [B, C] -> f32 [B, C]."""
    if isinstance(categories, torch.Tensor):
        m = categories.to(torch.float32)
    elif (isinstance(categories, list) and len(categories) == B and B > 0 and isinstance(categories[0], list)
          and len(categories[0]) == C and isinstance(categories[0][0], list)):
        # the reference's own feed, [B][C][1] Python lists: flattening through iterators is ~5x faster than
        # np.asarray on three levels of nesting (this conversion was half the cost of a 51-pair predict call)
        it = itertools.chain.from_iterable(itertools.chain.from_iterable(categories))
        try:
            m = np.fromiter(it, dtype=np.float32, count=B * C).reshape(B, C)
        except (ValueError, TypeError):
            m = None
        if m is None or next(it, None) is not None or sum(map(len, categories)) != B * C:
            m = np.asarray(categories, dtype=np.float32)    # ragged or deeper than expected: let numpy say what is wrong
    else:
        m = np.asarray(categories, dtype=np.float32)
    if m.ndim == 3 and m.shape[2] == 1:
        m = m.reshape(m.shape[0], m.shape[1])
    if m.ndim != 2 or m.shape[1] != C or m.shape[0] != B:
        raise ValueError("categories must be [B=%d, C=%d, 1] or [B, C]; got %r" % (B, C, tuple(m.shape)))
    return m


def _float_rows(x, B: int, width) -> np.ndarray:
    """[B][width] nested lists (the driver's label / one-hot / write-sign feeds) or arrays -> float32 ndarray.  Lists of
    lists go through one flat iterator (a third faster than np.asarray on two levels of nesting)."""
    if isinstance(x, list) and len(x) == B and B > 0 and isinstance(x[0], list):
        try:
            a = np.fromiter(itertools.chain.from_iterable(x), dtype=np.float32, count=-1)
            w_ = a.size // B
            if a.size == B * w_ and (width is None or w_ == width) and set(map(len, x)) == {w_}:
                return a.reshape(B, w_)
        except (ValueError, TypeError):
            pass
    return np.asarray(x, dtype=np.float32)


class Model:
    """``Model(args, Personal_Memory, Recipe_Embedding, Category_Embedding, General_Memory)``.

    ``args`` needs the attributes the reference constructor reads (Model_Recommender.py:6-24):
    ``num_categories, num_users, embed_size, high_level_score_coefficient`` are used; ``learner,
    num_labels, lr, decay_steps, decay_rate, beta_1, beta_2, alpha`` are recorded when present.
    Tables are numpy (or torch) arrays and are copied to HBM once; the caller keeps its host copies.
    ``General_Memory`` is accepted for signature parity; the forward never reads it (``write_memory`` does, and the build-defined
    ``topk_for_labels`` serves from it).
    """

    def __init__(self, args, Personal_Memory, Recipe_Embedding, Category_Embedding, General_Memory=None,
                 device: Optional[torch.device] = None, user_base: int = 0):
        for name in ("learner", "num_labels", "lr", "decay_steps", "decay_rate", "beta_1", "beta_2", "alpha"):
            setattr(self, name if name != "lr" else "learning_rate", getattr(args, name, None))
        self.num_categories = int(args.num_categories)
        self.num_users = int(args.num_users)
        self.embed_size = int(args.embed_size)
        self.high_level_score_coefficient = float(np.float32(args.high_level_score_coefficient))
        self.General_Memory = General_Memory

        # the input contract (Model_Recommender.py:26-35); only three feeds reach the logits
        self.user_input = _Placeholder("user_input", True)
        self.item_input = _Placeholder("item_input", True)
        self.categories = _Placeholder("categories", True)
        self.labels = _Placeholder("labels", False)
        self.write_sign = _Placeholder("write_sign", False)
        self.user_one_hot_label = _Placeholder("user_labels", False)
        self.dropout_keep_prob = _Placeholder("dropout_keep_prob", False)
        self.is_training_flag = _Placeholder("is_training_flag", False)
        self.logits = _Fetch("logits")
        # training-side fetches (Model_Recommender.py:38-41, :13); Global_Step never moves in the reference
        # (apply_gradients is called without it, :240), so learning_rate stays args.lr
        self.loss_value = _Fetch("loss_value")
        self.train_op = _Fetch("train_op")
        self.personal = _Fetch("personal")
        self.general = _Fetch("general")
        self.learning_rate = _ScalarFetch(0.001 if self.learning_rate is None else self.learning_rate)   # --lr default
        self.global_step = 0
        self.epoch_step = 0
        self.epoch_increment = _Fetch("epoch_increment")
        self._train_started = False

        pm_shape = tuple(Personal_Memory.shape)
        if len(pm_shape) != 3 or pm_shape[1] != self.num_categories + 1 or pm_shape[2] != self.embed_size:
            raise ValueError("Personal_Memory %r does not match num_categories=%d, embed_size=%d"
                             % (pm_shape, self.num_categories, self.embed_size))
        if user_base == 0 and pm_shape[0] != self.num_users:
            raise ValueError("Personal_Memory has %d users, args.num_users = %d" % (pm_shape[0], self.num_users))
        self.engine = ScoringEngine(Personal_Memory, Recipe_Embedding, Category_Embedding,
                                    coef=self.high_level_score_coefficient, device=device, user_base=user_base)
        self.device = self.engine.device
        self._gm_dev = None             # General_Memory on the device, created by the first personal / general fetch

    # -- predict ------------------------------------------------------------------------------------
    def predict_device(self, user_input, item_input, categories) -> torch.Tensor:
        """Scores as a device tensor, no synchronisation (stream-ordered)."""
        ut, dt, mt = self._feeds(user_input, item_input, categories)
        return torch.ops.m2d.score_pairs(self.engine.id, ut, dt, mt)

    def predict(self, user_input, item_input, categories, **ignored) -> np.ndarray:
        """``sess.run([model.logits], feed_dict)[0]`` (evaluate.py:55-59): float32 ``ndarray [B]``.

        Extra reference feeds (``labels``, ``dropout_keep_prob``, ``is_training_flag`` ...) are accepted
        and ignored: no op in the reference's forward reads them.  An out-of-range id raises
        ``IndexError`` (TF-CPU ``GatherV2`` raises ``InvalidArgumentError``)."""
        if any(isinstance(x, torch.Tensor) for x in (user_input, item_input, categories)):
            out = self.predict_device(user_input, item_input, categories)      # torch custom op, stream-ordered
            self.engine.check()
            return out.cpu().numpy()
        # host data (the reference's own feeds): one staged copy in, one out (m2d_score_pairs_host)
        u, d = _ids(user_input, "user"), _ids(item_input, "item")
        if len(d) != len(u):
            raise ValueError("user_input and item_input differ in length")
        return self.engine.score_pairs_host(u, d, _mask(categories, self.num_categories, len(u)))

    # -- training side -----------------------------------------------------
    def _feeds(self, user_input, item_input, categories):
        u, d = _ids(user_input, "user"), _ids(item_input, "item")
        B = len(u)
        if len(d) != B:
            raise ValueError("user_input and item_input differ in length")
        m = _mask(categories, self.num_categories, B)
        dev = self.device
        ut = u.to(dev, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(dev)
        dt = d.to(dev, torch.int32) if isinstance(d, torch.Tensor) else torch.from_numpy(d).to(dev)
        mt = m.to(dev) if isinstance(m, torch.Tensor) else torch.from_numpy(m).to(dev)
        return ut, dt, mt

    def _device_batch(self, user_input, item_input, categories, floats):
        """Host feeds of one driver batch (Train_recommender.py:189-194) -> device tensors through ONE staged copy:
        users | items | masks | each entry of `floats` (name -> (feed, width)) packed into a single buffer.  Returns
        (users, items, masks, {name: tensor [B, width]}); feeds that are already tensors take `_feeds`."""
        extras = [(k, v, wd) for k, (v, wd) in floats.items()]
        if any(isinstance(x, torch.Tensor) for x in (user_input, item_input, categories)) or \
                any(isinstance(v, torch.Tensor) for _, v, _ in extras):
            ut, dt, mt = self._feeds(user_input, item_input, categories)
            B = ut.numel()
            out = {}
            for k, v, wd in extras:
                t = v if isinstance(v, torch.Tensor) else torch.as_tensor(_float_rows(v, B, wd))
                out[k] = t.to(self.device, torch.float32).reshape(B, t.numel() // B if B else 0)
            return ut, dt, mt, out
        u, d = _ids(user_input, "user"), _ids(item_input, "item")
        B = len(u)
        if len(d) != B:
            raise ValueError("user_input and item_input differ in length")
        m = _mask(categories, self.num_categories, B)
        C = self.num_categories
        rows = [_float_rows(v, B, wd) for _, v, wd in extras]
        up = lambda n: (n + 3) & ~3                            # every section starts on a 16-byte boundary
        Bp = up(B)
        o_m = 2 * Bp
        pos = o_m + up(B * C)
        spans = []
        for r in rows:
            spans.append((pos, r.size))
            pos += up(r.size)
        buf = np.zeros(pos, dtype=np.float32)
        ib = buf.view(np.int32)
        ib[:B] = u
        ib[Bp:Bp + B] = d
        buf[o_m:o_m + B * C] = m.reshape(-1)
        for r, (a, n) in zip(rows, spans):
            buf[a:a + n] = r.reshape(-1)
        t = torch.from_numpy(buf).to(self.device)
        it = t.view(torch.int32)
        out = {k: t[a:a + n].reshape(B, n // B if B else 0) for (k, _, _), (a, n) in zip(extras, spans)}
        return it[:B], it[Bp:Bp + B], t[o_m:o_m + B * C].reshape(B, C), out

    def train_step(self, user_input, item_input, categories, labels, apply: bool = True):
        """``sess.run([model.loss_value, model.learning_rate, model.train_op], feed_dict)``
        (Train_recommender.py:189-199): returns ``(loss, learning_rate)`` as Python floats; with ``apply=False``
        only the loss is evaluated.  The optimizer is ``args.learner`` at ``args.lr`` (Model_Recommender.py:223-241)."""
        if not self._train_started:
            self.engine.train_begin(self.learner or "sgd", float(self.learning_rate), 5.0)
            self._train_started = True
        ut, dt, mt = self._feeds(user_input, item_input, categories)
        y = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels, dtype=np.float32))
        out = self.engine.train_step(ut, dt, mt, y.reshape(-1), apply=apply)
        self.engine.check()
        loss, _norm, _scale, lr = (float(v) for v in out.cpu().numpy())
        return loss, lr

    def write_memory(self, user_input, item_input, categories, write_sign, user_one_hot_label,
                     personal: bool = True, general: bool = True):
        """The ``personal`` / ``general`` fetches (``Write_Memory``, Model_Recommender.py:106-220).  As in the reference
        graph each fetch pulls in only the assigns it depends on: ``personal`` the two chained Personal_Memory assigns
        (:167, :198), ``general`` the General_Memory assign (:215).  Updates those tables in place and returns
        ``(mean(Personal_Memory), mean(General_Memory))`` with ``None`` for a table that was not fetched."""
        if self._gm_dev is None:
            if self.General_Memory is None:
                raise ValueError("Model was built without General_Memory")
            self._gm_dev = torch.as_tensor(np.asarray(self.General_Memory, dtype=np.float32)).to(self.device).contiguous()
        ut, dt, mt = self._feeds(user_input, item_input, categories)
        B = ut.numel()
        as_t = lambda v, wd: v if isinstance(v, torch.Tensor) else torch.as_tensor(_float_rows(v, B, wd))
        sign = as_t(write_sign, 1).reshape(B)
        y = as_t(user_one_hot_label, None).reshape(B, -1)
        return self.engine.write_memory(ut, dt, mt, sign, y, self._gm_dev, float(self.beta_1), float(self.beta_2),
                                        float(self.alpha), want_means=True, write_pm=personal, write_gm=general)

    # -- checkpoint (stands where the driver uses tf.train.Saver, Train_recommender.py:145-149, :218-222) ----------
    _TABLE_FILES = ("Personal_Memory", "Recipe_Embedding", "Category_Embedding", "General_Memory")

    def save(self, path: str):
        """One ``.npz``: the four tables under the names of the reference's ``.npy`` files (so each can be re-saved
        with ``np.save`` and fed back to the reference), plus the optimizer's slots and step count once training has
        started."""
        self.engine.check()
        data = {"Personal_Memory": self.engine.pm.cpu().numpy(), "Recipe_Embedding": self.engine.re.cpu().numpy(),
                "Category_Embedding": self.engine.ce.cpu().numpy(), "epoch_step": np.int64(self.epoch_step)}
        if self.General_Memory is not None:
            data["General_Memory"] = self.general_memory()
        if self._train_started:
            data["learner"] = np.str_(str(self.learner or "sgd").lower())
            data["steps"] = np.int64(self.engine.train_steps())
            for tb in range(3):
                for sl in range(2):
                    try:
                        data["slot_%d_%d" % (tb, sl)] = self.engine.train_slot(tb, sl).cpu().numpy()
                    except ValueError:                      # this learner has no such slot
                        pass
        np.savez(path, **data)

    def restore(self, path: str):
        """Load what `save` wrote INTO this model (same shapes): tables in place on the device, optimizer state if the
        file has it and the learner matches."""
        z = np.load(path if str(path).endswith(".npz") else str(path) + ".npz")
        for name, dst in (("Personal_Memory", self.engine.pm), ("Recipe_Embedding", self.engine.re),
                          ("Category_Embedding", self.engine.ce)):
            src = torch.from_numpy(z[name])
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError("%s in the checkpoint is %r, the model has %r" % (name, tuple(src.shape), tuple(dst.shape)))
            dst.copy_(src)
        self.engine.tables_updated()
        if "General_Memory" in z.files:
            self.General_Memory = z["General_Memory"]
            self._gm_dev = None
        self.epoch_step = int(z["epoch_step"]) if "epoch_step" in z.files else 0
        if "steps" in z.files:
            if str(z["learner"]) != str(self.learner or "sgd").lower():
                raise ValueError("checkpoint was trained with %s, this model uses %s" % (z["learner"], self.learner))
            self.engine.train_begin(self.learner or "sgd", float(self.learning_rate), 5.0)
            self._train_started = True
            self.engine.train_steps(restore=int(z["steps"]))
            for key in z.files:
                if key.startswith("slot_"):
                    _, tb, sl = key.split("_")
                    self.engine.train_slot(int(tb), int(sl), restore=torch.from_numpy(z[key]))
        self.engine.check()

    def general_memory(self) -> np.ndarray:
        """General_Memory as it stands (host copy)."""
        return np.asarray(self.General_Memory, dtype=np.float32) if self._gm_dev is None else self._gm_dev.cpu().numpy()

    # -- resident dish -> category table (dish_to_category.json) --------------------------------------
    def set_dish_categories(self, dish_to_category, num_dishes: Optional[int] = None):
        """Accepts the JSON dict ``{str(dish): [[m0], [m1], ...]}`` (Train_recommender.py:132) or an
        ``[I, C]`` array.  Dishes missing from the dict get an all-zero mask (their score is NaN, as a
        zero mask gives in the reference)."""
        I = self.engine.I if num_dishes is None else num_dishes
        if isinstance(dish_to_category, dict):
            table = np.zeros((I, self.num_categories), dtype=np.float32)
            for key, val in dish_to_category.items():
                d = int(key)
                if 0 <= d < I:
                    table[d] = np.asarray(val, dtype=np.float32).reshape(-1)
        else:
            table = np.asarray(dish_to_category, dtype=np.float32).reshape(I, self.num_categories)
        self.engine.set_dish_categories(table)
        return table


    # -- retrieval and build-defined extensions (no reference counterpart; DESIGN.md sections 4.3-4.4, 8) ---
    def _slate(self, users, dishes):
        """(users, sorted distinct dish ids) as int32 device tensors, and each given dish's column among the distinct ones"""
        u, d = _ids(users, "user"), _ids(dishes, "item")
        ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        d = d.cpu().numpy() if isinstance(d, torch.Tensor) else d
        distinct, col = np.unique(np.asarray(d, dtype=np.int32).reshape(-1), return_inverse=True)
        return ut, torch.from_numpy(distinct).to(self.device), col.reshape(-1)

    def score_slate(self, users, dishes) -> np.ndarray:
        """EXTENSION (no reference counterpart): what each of `users` scores for each of `dishes` -- one shared list, the dishes
        that can be cooked from today's market, a shared negative pool, an editorial list.  Ids as str or int, in any order, repeats
        allowed; returns float32 [len(users), len(dishes)] with the columns in the order given.  Needs `set_dish_categories`.
        (``ScoringEngine.score_slate``, which takes the sorted distinct ids.)"""
        ut, slate, col = self._slate(users, dishes)
        out = torch.ops.m2d.score_slate(self.engine.id, ut, slate)
        self.engine.check()
        return out.cpu().numpy()[:, col]

    def set_recipes(self, dish_to_ingredients, num_ingredients: int):
        """EXTENSION: every dish's ingredient list, for `cookable` and `topk(market=...)` -- a dict ``{str(dish): [ingredient ids]}``
        (dishes missing from it get an empty list and are never cookable; a key outside the catalogue raises IndexError) or an ``(offsets, ids)`` CSR pair; ids in
        [0, num_ingredients), repeats allowed.  Independent of `set_ingredients`.  (``ScoringEngine.set_recipes``.)"""
        I = self.engine.I
        if isinstance(dish_to_ingredients, dict):
            lists = [()] * I
            for key, val in dish_to_ingredients.items():
                d = int(key)
                if not 0 <= d < I:
                    raise IndexError("set_recipes: dish id %d is outside the catalogue [0, %d)" % (d, I))
                lists[d] = val
            off = np.zeros(I + 1, dtype=np.int64)
            np.cumsum([len(l) for l in lists], out=off[1:])
            ids = _ids([v for l in lists for v in l], "ingredient")
            if off[-1] >= 2 ** 31:
                raise ValueError("set_recipes: more than 2^31 - 1 list entries")
            off = off.astype(np.int32)
        else:
            off, ids = dish_to_ingredients
        self.engine.set_recipes(off, ids, num_ingredients)

    def cookable(self, market, max_missing: int = 0) -> np.ndarray:
        """EXTENSION: the dishes that can be cooked from `market` (ingredient ids as str or int, any order, repeats allowed) with at
        most `max_missing` list entries absent, as a sorted numpy int32 array.  Needs `set_recipes`."""
        m = _ids(market, "ingredient")
        mt = m.to(self.device, torch.int32) if isinstance(m, torch.Tensor) else torch.from_numpy(m).to(self.device)
        return self.engine.cookable_dishes(mt, max_missing).cpu().numpy()

    def topk_markets(self, users, markets, k: int = 10, max_missing: int = 0):
        """EXTENSION: one user, one market per request -- `users` as str or int, `markets` a list of ingredient-id sequences (str or
        int, any order, repeats allowed, may be empty) aligned with `users`.  Returns numpy (scores float32 [n, k], dish ids int32
        [n, k], counts int32 [n]): row q lists the k best dishes that can be cooked from markets[q] for users[q]
        (``ScoringEngine.topk_markets``: one call for the whole batch, `cookable`'s definition, `topk`'s order), id -1 / NaN from
        column counts[q] on; counts[q] is the number of cookable dishes.  k <= 64.  Needs `set_dish_categories` and `set_recipes`."""
        u = _ids(users, "user")
        n = u.numel() if isinstance(u, torch.Tensor) else len(u)
        if len(markets) != n:
            raise ValueError("topk_markets: %d markets for %d users" % (len(markets), n))
        lists = [_ids(m, "ingredient") for m in markets]
        lists = [m.cpu().numpy().astype(np.int32) if isinstance(m, torch.Tensor) else m for m in lists]
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(m) for m in lists], out=off[1:])
        ids = np.concatenate(lists).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
        dev = lambda a: a.to(self.device) if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(self.device)
        s, i, c = torch.ops.m2d.topk_markets(self.engine.id, dev(u).to(torch.int32), dev(off), dev(ids), int(k), int(max_missing))
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()

    def topk_markets_excluding(self, users, markets, exclude=None, k: int = 10, max_missing: int = 0, missing: bool = False):
        """EXTENSION: `topk_markets` that leaves out what each shopper has already had and can say what to buy.  `exclude`: a dict
        keyed by the user as given in `users` (a missing key excludes nothing) or a list aligned with `users`, of dish ids (str or
        int, any order, repeats allowed), as in `topk`; None excludes nothing.  Returns numpy (scores [n, k], dish ids [n, k], counts
        [n]) -- counts[q] is the number of cookable dishes that are not excluded -- and with `missing=True` a fourth array int32
        [n, k, max_missing]: for listed dish [q, j] the ingredient ids of its list entries that markets[q] lacks, in list order, every
        occurrence, -1 from the number missing on.  (``ScoringEngine.topk_markets_excluding``, one call for the whole batch.)"""
        u = _ids(users, "user")
        n = u.numel() if isinstance(u, torch.Tensor) else len(u)
        if len(markets) != n:
            raise ValueError("topk_markets_excluding: %d markets for %d users" % (len(markets), n))
        lists = [_ids(m, "ingredient") for m in markets]
        lists = [m.cpu().numpy().astype(np.int32) if isinstance(m, torch.Tensor) else m for m in lists]
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(m) for m in lists], out=off[1:])
        ids = np.concatenate(lists).astype(np.int32) if off[-1] else np.zeros(0, np.int32)
        dev = lambda a: a.to(self.device) if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(self.device)
        xoff = xids = None
        if exclude is not None:
            from .ops import exclusion_csr
            had = [_ids(x, "item") for x in _exclusion_lists(exclude, users, "topk_markets_excluding")]
            had = [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in had]
            xo, xi = exclusion_csr(had, n)                   # sorted and de-duplicated per request
            xoff, xids = dev(xo), dev(xi)
        s, i, c, m = torch.ops.m2d.topk_markets_excluding(self.engine.id, dev(u).to(torch.int32), dev(off), dev(ids), xoff, xids, int(k),
                                                          int(max_missing))
        self.engine.check()
        out = (s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy())
        return out + (m.cpu().numpy(),) if missing else out

    def topk(self, users, k: int = 10, exclude=None, head: bool = False, candidates: int = 0, among=None, market=None,
             max_missing: int = 0):
        """The k best dishes of every user in `users` over the whole catalogue -- the ranking rule of
        evaluate.py:63 applied to all dishes instead of 51 candidates.  Needs `set_dish_categories`.
        Returns (scores float32 [n, k], dish ids int32 [n, k]).

        `exclude` leaves out dishes per user (the ones already had): a dict such as ``Dataset.trainMatrix`` keyed by the user as
        given in `users` (a missing key excludes nothing), or a list aligned with `users`.  The lists are then those
        ``evaluate_model_full`` measures (``ScoringEngine.topk_users_excluding``: k <= 16; rows end in id -1 / NaN when fewer than k
        dishes remain).  None: the unfiltered lists, as before.

        EXTENSION, `head=True`: the lists under the MLP head (`set_mlp_head`), the score `predict_extended(head=True)` returns --
        `candidates` = 0 scores every dish under the head, K1 = `candidates` >= k reranks the K1 best by the reference score
        (``ScoringEngine.topk_users_mlp``).  `head=True` with `exclude` raises here: the lists under the head without the dishes
        already had are `topk_head`'s.

        EXTENSION, `among=dishes`: the k best among those dishes only (str or int ids, any order, repeats ignored;
        ``ScoringEngine.topk_slate``) -- the same order, the scores `score_slate` returns.  `among` with `exclude` or `head=True`
        raises.

        EXTENSION, `market=ingredients`: the k best among the dishes that can be cooked from those ingredients (`set_recipes`;
        `cookable(market, max_missing)` is the list), k <= 64 -- ``ScoringEngine.topk_market``: `among`'s order and scores; rows end in
        id -1 / NaN when fewer than k dishes are cookable.  `market` with `exclude`, `head=True`, `candidates` or `among` raises."""
        if market is not None:
            for name, given in (("exclude", exclude is not None), ("head=True", head), ("candidates", bool(candidates)), ("among", among is not None)):
                if given:
                    raise ValueError("topk: market together with %s is not supported" % name)
            u, m = _ids(users, "user"), _ids(market, "ingredient")
            dev = lambda a: a.to(self.device, torch.int32) if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(self.device)
            s, i, _ = self.engine.topk_market(dev(u), dev(m), k, max_missing)
            self.engine.check()
            return s.cpu().numpy(), i.cpu().numpy()
        if among is not None:
            if exclude is not None or head or candidates:
                raise ValueError("topk: among together with exclude or head=True (or its candidates) is not supported")
            ut, slate, _ = self._slate(users, among)
            s, i = torch.ops.m2d.topk_slate(self.engine.id, ut, slate, int(k))
            self.engine.check()
            return s.cpu().numpy(), i.cpu().numpy()
        if head and exclude is not None:
            raise ValueError("topk: head=True together with exclude is not supported (exclusions under the MLP head): "
                             "topk_head(users, k, exclude) serves them")
        if candidates and not head:
            raise ValueError("topk: candidates is the head's rerank width; it needs head=True")
        if exclude is not None:
            from .ops import topk_excluding_args
            off, ids = topk_excluding_args(len(users), k, _exclusion_lists(exclude, users, "topk"))
        u = _ids(users, "user")
        ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        if exclude is not None:
            s, i = self.engine.topk_users_excluding(ut, int(k), (torch.from_numpy(off).to(self.device), torch.from_numpy(ids).to(self.device)))
        elif head:
            s, i = torch.ops.m2d.topk_users_mlp(self.engine.id, ut, int(k), int(candidates))
        else:
            s, i = torch.ops.m2d.topk_users(self.engine.id, ut, int(k))
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def topk_for_labels(self, labels, k: int = 10, users=None, exclude=None, market=None, max_missing: int = 0, alpha=None):
        """EXTENSION (no reference counterpart): the k best dishes for people described by their HEALTH LABELS --
        `labels` a list of label-id lists (one per request) or an [n, num_labels] array of ``user_one_hot_label`` rows.  Each request's
        memory block is alpha * (the label-weighted mean of General_Memory's rows), on top of Personal_Memory[users[q]] when `users`
        names a known user (str or int; -1 or ``users=None``: a guest): what ``write_memory`` would add to that user's block,
        served without writing it.  General_Memory is read as it stands: a ``write_memory`` is visible to the next call.
        `alpha`: 1 for guests, ``args.alpha`` when `users` is given.  `exclude`: a list of dish-id lists aligned with the requests, or a
        dict keyed by the user as given in `users` (then k <= 16, as in `topk`).  `market`: a list of ingredient-id sequences, one per
        request -- the lists are then those of `topk_markets_excluding` (k <= 64, `max_missing` as there), rows ending in -1 / NaN.
        Returns (scores float32 [n, k], dish ids int32 [n, k]).  (``ScoringEngine.topk_profiles`` / ``topk_markets_profiles``.)"""
        if self._gm_dev is None:
            if self.General_Memory is None:
                raise ValueError("Model was built without General_Memory")
            self._gm_dev = torch.as_tensor(np.asarray(self.General_Memory, dtype=np.float32)).to(self.device).contiguous()
        if not isinstance(labels, list):
            labels = labels if isinstance(labels, torch.Tensor) else np.asarray(labels, dtype=np.float32)
        n = len(labels)
        if alpha is None:
            alpha = 1.0 if users is None else float(self.alpha)
        ut = None
        if users is not None:
            u = _ids(users, "user")
            ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        had = None
        if exclude is not None:
            if isinstance(exclude, dict) and users is None:
                raise ValueError("topk_for_labels: a dict of exclusions is keyed by user; guests take a list aligned with the requests")
            had = [_ids(x, "item") for x in _exclusion_lists(exclude, users if users is not None else range(n), "topk_for_labels")]
            had = [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in had]
        if market is not None:
            if len(market) != n:
                raise ValueError("topk_for_labels: %d markets for %d requests" % (len(market), n))
            lists = [_ids(m, "ingredient") for m in market]
            lists = [m.cpu().numpy().astype(np.int32) if isinstance(m, torch.Tensor) else m for m in lists]
            s, i = self.engine.topk_markets_profiles(labels, self._gm_dev, lists, int(k), ut, alpha, had, int(max_missing))
        else:
            s, i = self.engine.topk_profiles(labels, self._gm_dev, int(k), ut, alpha, had)
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def topk_head(self, users, k: int = 10, exclude=None, candidates: int = 0):
        """EXTENSION: the k best dishes of every user under the MLP head (`set_mlp_head`), leaving out `exclude`'s dishes per user -- a
        dict keyed by the user as given in `users` (a missing key excludes nothing) or a list aligned with `users`, as in `topk`; None
        excludes nothing.  k <= 64; rows end in id -1 / NaN when fewer than k dishes remain.  `candidates` = 0 scores every dish under
        the head; K1 = `candidates` >= k (K1 <= 16 with exclusions) reranks the K1 best by the reference score among the dishes left
        (``ScoringEngine.topk_users_mlp_excluding``).  Returns (scores float32 [n, k], dish ids int32 [n, k])."""
        if exclude is not None:
            exclude = _exclusion_lists(exclude, users, "topk_head")
        u = _ids(users, "user")
        ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        s, i = self.engine.topk_users_mlp_excluding(ut, int(k), exclude, int(candidates))
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def topk_deep(self, users, k: int = 100, exclude=None, head: bool = False, candidates: int = 0):
        """EXTENSION (DESIGN.md sections 4.11, 8.8): deep lists -- the k best dishes of every user over the whole catalogue for
        1 <= k <= 1024, leaving out `exclude`'s dishes per user (a dict keyed by the user as given in `users`, or a list aligned
        with `users`, as in `topk`; None excludes nothing).  The order is `topk`'s; a listed score is the word `score_slate` returns
        for that (user, dish); rows end in id -1 / NaN when fewer than k dishes remain (``ScoringEngine.topk_users_deep``).
        `head=True`: the lists under the MLP head -- `candidates` = 0 scores every dish under the head, k <= K1 = `candidates` <= 1024
        reranks the K1 best of the lists above (``ScoringEngine.topk_users_mlp_deep``).  Returns (scores float32 [n, k], dish ids
        int32 [n, k])."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 1024:
            raise ValueError("topk_deep: 1 <= k <= 1024, got %r" % (k,))
        if candidates and not head:
            raise ValueError("topk_deep: candidates is the head's rerank width; it needs head=True")
        if exclude is not None:
            exclude = _exclusion_lists(exclude, users, "topk_deep")
        u = _ids(users, "user")
        ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        if head:
            s, i = self.engine.topk_users_mlp_deep(ut, int(k), exclude, int(candidates))
        else:
            s, i = self.engine.topk_users_deep(ut, int(k), exclude)
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def _cap_row(self, spec, k: int, what: str) -> list:
        """one cap row as C ints: None is uncapped (k everywhere), a dict {category index: cap} caps what it names, a sequence is the row"""
        C = self.engine.C
        if spec is None:
            return [k] * C
        if isinstance(spec, dict):
            r = [k] * C
            for c, cap in spec.items():
                if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < C:
                    raise ValueError(what + ": category index %r outside [0, %d)" % (c, C))
                r[int(c)] = int(cap)
            return r
        r = [int(cap) for cap in spec]
        if len(r) != C:
            raise ValueError(what + ": a cap row has %d entries for %d categories" % (len(r), C))
        return r

    def _menu_caps(self, caps, k: int, n: int, what: str) -> torch.Tensor:
        """`caps` of `topk_menu` and `topk_menu_filtered` -> an int32 device tensor [n, C], or [C] (one row for every user)"""
        C = self.engine.C

        def row(spec):
            return self._cap_row(spec, k, what)

        per_user = (isinstance(caps, (list, tuple)) and len(caps) > 0
                    and all(c is None or isinstance(c, (dict, list, tuple, np.ndarray)) for c in caps))
        if per_user:
            if len(caps) != n:
                raise ValueError(what + ": %d cap rows for %d users" % (len(caps), n))
            table = np.asarray([row(c) for c in caps], dtype=np.int64).reshape(n, C)
        else:
            table = np.asarray(row(caps), dtype=np.int64).reshape(C)
        if table.size and (table.min() < 0 or table.max() > np.iinfo(np.int32).max):
            raise ValueError(what + ": caps must be >= 0")
        return torch.from_numpy(table.astype(np.int32)).to(self.device)

    def topk_menu(self, users, k: int = 10, caps=None):
        """EXTENSION, build-defined (no reference counterpart): a MENU per user -- the k best dishes over the
        whole catalogue in `topk`'s order with at most cap[c] dishes of category c in a list (a dish counts in every category of its
        mask).  `caps`: a dict {category index: cap} (missing categories are uncapped), a list of C ints, or a list of either aligned
        with `users`; None is uncapped.  1 <= k <= 64; rows end in id -1 / NaN where the caps leave fewer than k dishes.  Returns
        numpy (scores float32 [n, k], dish ids int32 [n, k]).  (``torch.ops.m2d.topk_menu``.)"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("topk_menu: 1 <= k <= 64, got %r" % (k,))
        k = int(k)
        u = _ids(users, "user")
        ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        table = self._menu_caps(caps, k, int(ut.numel()), "topk_menu")
        s, i = self.engine._topk_menu(ut, k, table)
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def topk_menu_filtered(self, users, k: int = 10, caps=None, exclude=None, among=None, market=None, max_missing: int = 0):
        """EXTENSION, build-defined (no reference counterpart): `topk_menu` chosen from what the shopper may
        have today -- `among=dishes`: those dishes only (str or int ids, any order, repeats ignored, as in `topk`);
        `market=ingredients`: the dishes `cookable(market, max_missing)` lists; neither: the whole catalogue -- and leaving out what
        they have already had -- `exclude`: a dict keyed by the user as given in `users` (a missing key excludes nothing) or a list
        aligned with `users`, as in `topk_deep`; an excluded dish outside the slate is ignored.  A dish that is left out counts against
        no cap.  `caps` as in `topk_menu`.  `among` together with `market` raises; `exclude` goes with either (exclusions are per
        user: they cannot be taken out of a shared slate).  1 <= k <= 64; rows end in id -1 / NaN where fewer than k dishes can be
        taken -- all of them when the slate is empty (the engine is not called).  Returns numpy (scores float32 [n, k], dish ids int32
        [n, k]).  (``torch.ops.m2d.topk_menu_filtered``.)"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("topk_menu_filtered: 1 <= k <= 64, got %r" % (k,))
        k = int(k)
        if among is not None and market is not None:
            raise ValueError("topk_menu_filtered: among together with market is not supported")
        u = _ids(users, "user")
        ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        n = int(ut.numel())
        table = self._menu_caps(caps, k, n, "topk_menu_filtered")
        off = ids = None
        if exclude is not None:
            from .ops import exclusions_on_device
            had = [_ids(x, "item") for x in _exclusion_lists(exclude, users, "topk_menu_filtered")]
            had = [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in had]
            off, ids = exclusions_on_device(had, n, self.device, "topk_menu_filtered")      # sorted and de-duplicated per user
        slate = None
        if market is not None:
            slate = np.asarray(self.cookable(market, max_missing), dtype=np.int32)
        elif among is not None:
            d = _ids(among, "item")
            slate = np.unique(np.asarray(d.cpu().numpy() if isinstance(d, torch.Tensor) else d, dtype=np.int32).reshape(-1))
        if slate is not None and slate.size == 0:
            return np.full((n, k), np.nan, dtype=np.float32), np.full((n, k), -1, dtype=np.int32)
        st = None if slate is None else torch.from_numpy(slate).to(self.device)
        s, i = torch.ops.m2d.topk_menu_filtered(self.engine.id, ut, table, k, off, ids, st)
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def plan_menus(self, users, days: int = 7, k: int = 3, caps=None, plan_caps=None, exclude=None, among=None, market=None,
                   max_missing: int = 0):
        """EXTENSION, build-defined (no reference counterpart): a MEAL PLAN per user -- `days` menus of k dishes,
        no dish twice: day d is `topk_menu_filtered` with the dishes of the earlier days left out.  `caps` (as in `topk_menu`) hold on
        every day; `plan_caps` (the same forms, missing categories bounded by days * k) hold over the whole plan -- "fish at most twice
        this week" is ``plan_caps={fish: 2}``; None: no plan cap.  `exclude` / `among` / `market` / `max_missing` as in
        `topk_menu_filtered`.  1 <= k <= 64, days >= 1, days * k <= 1024.  A day's row ends in id -1 / NaN where it cannot take k dishes
        -- all of them when the slate is empty (the engine is not called).  Returns numpy (scores float32 [n, days, k], dish ids int32
        [n, days, k]).  (``torch.ops.m2d.plan_menus``.)"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("plan_menus: 1 <= k <= 64, got %r" % (k,))
        if isinstance(days, bool) or not isinstance(days, (int, np.integer)) or int(days) < 1 or int(days) * int(k) > 1024:
            raise ValueError("plan_menus: days >= 1 and days * k <= 1024, got days = %r, k = %r" % (days, k))
        k, days = int(k), int(days)
        if among is not None and market is not None:
            raise ValueError("plan_menus: among together with market is not supported")
        u = _ids(users, "user")
        ut = u.to(self.device, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(self.device)
        n = int(ut.numel())
        table = self._menu_caps(caps, k, n, "plan_menus")
        plan = None if plan_caps is None else self._menu_caps(plan_caps, days * k, n, "plan_menus")
        off = ids = None
        if exclude is not None:
            from .ops import exclusions_on_device
            had = [_ids(x, "item") for x in _exclusion_lists(exclude, users, "plan_menus")]
            had = [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in had]
            off, ids = exclusions_on_device(had, n, self.device, "plan_menus")      # sorted and de-duplicated per user
        slate = None
        if market is not None:
            slate = np.asarray(self.cookable(market, max_missing), dtype=np.int32)
        elif among is not None:
            d = _ids(among, "item")
            slate = np.unique(np.asarray(d.cpu().numpy() if isinstance(d, torch.Tensor) else d, dtype=np.int32).reshape(-1))
        if slate is not None and slate.size == 0:
            return np.full((n, days, k), np.nan, dtype=np.float32), np.full((n, days, k), -1, dtype=np.int32)
        st = None if slate is None else torch.from_numpy(slate).to(self.device)
        s, i = torch.ops.m2d.plan_menus(self.engine.id, ut, table, days, k, plan, off, ids, st)
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def topk_group(self, groups, k: int = 10, mode: str = "least", exclude=None, among=None, market=None, max_missing: int = 0):
        """EXTENSION, build-defined (no reference counterpart): ONE list of k dishes per household -- `groups` a
        list of lists of user ids (str or int, at most 64 each, repeats count twice in the mean).  `mode`: "least" (least misery: a
        dish is worth what its unhappiest member scores), "mean" or "most".  `exclude`: a list of dish-id lists aligned with `groups`,
        or a dict keyed by user (str or int, whichever form `groups` uses) -- a group then leaves out the sorted union of its members' lists.  `among`: the dishes to choose from,
        as in `topk`.  `market=ingredients`: `cookable(market, max_missing)` is the slate; rows end in id -1 / NaN when fewer than k
        dishes are cookable.  `market` with `among` or `exclude`, and `among` with `exclude`, raise.  1 <= k <= 1024.  Returns numpy
        (scores float32 [nG, k], dish ids int32 [nG, k]).  (``ScoringEngine.topk_groups``.)"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 1024:
            raise ValueError("topk_group: 1 <= k <= 1024, got %r" % (k,))
        k = int(k)
        if market is not None and (among is not None or exclude is not None):
            raise ValueError("topk_group: market together with among or exclude is not supported")
        if among is not None and exclude is not None:
            raise ValueError("topk_group: among together with exclude is not supported (take the dishes out of `among`)")
        groups = [list(g) for g in groups]
        members = []
        for g in groups:
            m = _ids(g, "user")
            members.append((m.cpu().numpy() if isinstance(m, torch.Tensor) else m).tolist())
        if exclude is not None:
            if isinstance(exclude, dict):                    # keys and members are compared as ints: "7" and 7 are the same user
                by_user = {int(u): x for u, x in exclude.items()}
                exclude = [sorted({int(d) for u in m for d in by_user.get(u, ())}) for m in members]
            elif len(exclude) != len(groups):
                raise ValueError("topk_group: %d exclusion lists for %d groups" % (len(exclude), len(groups)))
            else:
                exclude = [(lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x)(_ids(x, "item")) for x in exclude]
        slate = None
        if market is not None:
            slate = np.asarray(self.cookable(market, max_missing), dtype=np.int32)
        elif among is not None:
            d = _ids(among, "item")
            slate = np.unique(np.asarray(d.cpu().numpy() if isinstance(d, torch.Tensor) else d, dtype=np.int32).reshape(-1))
        if slate is None:
            s, i = self.engine.topk_groups(members, k, mode, exclude)
            self.engine.check()
            return s.cpu().numpy(), i.cpu().numpy()
        out_s = np.full((len(groups), k), np.nan, dtype=np.float32)
        out_i = np.full((len(groups), k), -1, dtype=np.int32)
        kk = min(k, int(slate.size))
        if market is None and kk < k:
            raise ValueError("topk_group: k = %d exceeds the %d distinct dishes of `among`" % (k, slate.size))
        if kk:
            s, i = self.engine.topk_groups(members, kk, mode, None, torch.from_numpy(slate).to(self.device))
            self.engine.check()
            out_s[:, :kk], out_i[:, :kk] = s.cpu().numpy(), i.cpu().numpy()
        return out_s, out_i

    def plan_group(self, groups, days: int = 7, k: int = 3, mode: str = "least", caps=None, plan_caps=None, member_caps=None,
                   member_plan_caps=None, exclude=None, among=None, market=None, max_missing: int = 0):
        """EXTENSION, build-defined (no reference counterpart): a MEAL PLAN per household -- `plan_menus` with
        the dishes ordered by the household's word under `mode`, as in `topk_group`; a household menu is ``days=1``.  `groups` as in
        `topk_group`.  Caps come per household or per member, not both: `caps` / `plan_caps` in the forms `plan_menus` accepts (a list
        of rows is aligned with `groups`); `member_caps` / `member_plan_caps` are dicts {user id: caps} (str or int keys, compared as
        ints; each value a dict {category index: cap} or a list of C ints) -- the household's cap for a category is the lowest any of
        its members has, a member without an entry is uncapped: "one of us may have fish at most twice this week" is
        ``member_plan_caps={her: {fish: 2}}``.  `exclude` in `topk_group`'s forms (a list aligned with `groups`, or a dict keyed by
        user: a household leaves out the union of its members' lists); `among` / `market` / `max_missing` as there, but `exclude`
        goes with either (an excluded dish outside the slate is ignored); `among` together with `market` raises.  1 <= k <= 64,
        days >= 1, days * k <= 1024.  A day's row ends in id -1 / NaN where it cannot take k dishes -- all of them when the slate is
        empty (the engine is not called).  Returns numpy (scores float32 [nG, days, k], dish ids int32 [nG, days, k]).
        (``torch.ops.m2d.plan_groups``.)"""
        what = "plan_group"
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 64:
            raise ValueError("%s: 1 <= k <= 64, got %r" % (what, k))
        if isinstance(days, bool) or not isinstance(days, (int, np.integer)) or int(days) < 1 or int(days) * int(k) > 1024:
            raise ValueError("%s: days >= 1 and days * k <= 1024, got days = %r, k = %r" % (what, days, k))
        k, days = int(k), int(days)
        if mode not in ("least", "mean", "most"):
            raise ValueError("%s: mode must be one of ['least', 'mean', 'most'], got %r" % (what, mode))
        if (caps is not None or plan_caps is not None) and (member_caps is not None or member_plan_caps is not None):
            raise ValueError("%s: caps / plan_caps (per household) together with member_caps / member_plan_caps (per member) is not "
                             "supported" % what)
        for name, table in (("member_caps", member_caps), ("member_plan_caps", member_plan_caps)):
            if table is not None and not isinstance(table, dict):
                raise ValueError("%s: %s must be a dict {user id: caps}" % (what, name))
        if among is not None and market is not None:
            raise ValueError("%s: among together with market is not supported" % what)
        groups = [list(g) for g in groups]
        nG = len(groups)
        members = []
        for g in groups:
            m = _ids(g, "user")
            members.append((m.cpu().numpy() if isinstance(m, torch.Tensor) else m).tolist())
        if any(len(m) < 1 or len(m) > 64 for m in members):
            raise ValueError("%s: a group has 1 to 64 members" % what)
        M = max([len(m) for m in members] + [1])
        per_member = member_caps is not None or member_plan_caps is not None
        if per_member:
            def expand(by_user, fill):
                rows = {int(_ids([u], "user")[0]): self._cap_row(spec, fill, what) for u, spec in by_user.items()}
                t = np.full((nG, M, self.engine.C), fill, dtype=np.int64)
                for g, m in enumerate(members):
                    for j, u in enumerate(m):
                        if u in rows:
                            t[g, j] = rows[u]
                if t.size and (t.min() < 0 or t.max() > np.iinfo(np.int32).max):
                    raise ValueError(what + ": caps must be >= 0")
                return torch.from_numpy(t.astype(np.int32)).to(self.device)
            table = expand(member_caps or {}, k)
            plan = None if member_plan_caps is None else expand(member_plan_caps, days * k)
        else:
            table = self._menu_caps(caps, k, nG, what)
            plan = None if plan_caps is None else self._menu_caps(plan_caps, days * k, nG, what)
        off = ids = None
        if exclude is not None:
            from .ops import exclusions_on_device
            if isinstance(exclude, dict):                    # keys and members are compared as ints: "7" and 7 are the same user
                by_user = {int(u): x for u, x in exclude.items()}
                had = [np.asarray(sorted({int(d) for u in m for d in by_user.get(u, ())}), dtype=np.int32) for m in members]
            elif len(exclude) != nG:
                raise ValueError("%s: %d exclusion lists for %d groups" % (what, len(exclude), nG))
            else:
                had = [(lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x)(_ids(x, "item")) for x in exclude]
            off, ids = exclusions_on_device(had, nG, self.device, what)      # sorted and de-duplicated per group
        slate = None
        if market is not None:
            slate = np.asarray(self.cookable(market, max_missing), dtype=np.int32)
        elif among is not None:
            d = _ids(among, "item")
            slate = np.unique(np.asarray(d.cpu().numpy() if isinstance(d, torch.Tensor) else d, dtype=np.int32).reshape(-1))
        if slate is not None and slate.size == 0:
            return np.full((nG, days, k), np.nan, dtype=np.float32), np.full((nG, days, k), -1, dtype=np.int32)
        padded = np.full((nG, M), -1, dtype=np.int32)
        for g, m in enumerate(members):
            padded[g, :len(m)] = m
        st = None if slate is None else torch.from_numpy(slate).to(self.device)
        s, i = torch.ops.m2d.plan_groups(self.engine.id, torch.from_numpy(padded).to(self.device), table, days, k, mode, plan, per_member,
                                         off, ids, st)
        self.engine.check()
        return s.cpu().numpy(), i.cpu().numpy()

    def set_ingredients(self, ingredient_table, offsets, ids, weights=None):
        """EXTENSION: multi-hot ingredient lists per dish (CSR) replacing the category sum of the high-level path."""
        self.engine.set_ingredients(ingredient_table, offsets, ids, weights)

    def set_mlp_head(self, W1, b1, W2, b2, w3, b3: float):
        """EXTENSION: 3-layer head added to the reference score (interaction vector -> 256 -> 64 -> 1)."""
        self.engine.set_mlp_head(W1, b1, W2, b2, w3, b3)

    def predict_extended(self, user_input, item_input, categories=None, head: bool = False) -> np.ndarray:
        """EXTENSION predict: ingredient high-level path (`head=False`; `categories=None` -> resident dish masks)
        or reference score + MLP head (`head=True`, resident dish masks)."""
        u, d = _ids(user_input, "user"), _ids(item_input, "item")
        dev = self.device
        ut = u.to(dev, torch.int32) if isinstance(u, torch.Tensor) else torch.from_numpy(u).to(dev)
        dt = d.to(dev, torch.int32) if isinstance(d, torch.Tensor) else torch.from_numpy(d).to(dev)
        if head:
            out = self.engine.score_pairs_mlp(ut, dt)
        else:
            m = None
            if categories is not None:
                m = _mask(categories, self.num_categories, len(u))
                m = m.to(dev) if isinstance(m, torch.Tensor) else torch.from_numpy(m).to(dev)
            out = self.engine.score_pairs_ingredients(ut, dt, m)
        self.engine.check()
        return out.cpu().numpy()


class Session:
    """Shim for ``tf.Session`` at the one place the scoring path uses it: ``sess.run(fetches, feed_dict)``
    with ``fetches`` = ``model.logits`` or ``[model.logits]`` (evaluate.py:58)."""

    def __init__(self, model: Model):
        self.model = model

    def run(self, fetches, feed_dict=None):
        """Fetches served: ``logits`` (evaluate.py:58); ``loss_value``, ``learning_rate``, ``train_op``, ``personal``,
        ``general`` (Train_recommender.py:180-199); ``epoch_increment`` / ``epoch_step`` (:155, :204).

        The reference fetches the memory write and ``train_op`` in one ``sess.run`` with no control dependency
        between them, so TF may order them either way; here the optimizer step runs first and ``Write_Memory``
        sees the updated tables.  ``general`` alone (the driver's ordinary batch, Train_recommender.py:195-199) writes
        General_Memory only; Personal_Memory is written only when ``personal`` is fetched (:180-184)."""
        as_list = isinstance(fetches, (list, tuple))
        fl: Sequence = fetches if as_list else [fetches]
        m = self.model
        known = (m.logits, m.loss_value, m.train_op, m.personal, m.general, m.epoch_increment, m.learning_rate)
        for f in fl:
            if not any(f is k for k in known) and f != "epoch_step":
                raise NotImplementedError("fetch %r is not served" % (f,))
        feed_dict = feed_dict or {}

        def feed(key, what):
            try:
                return feed_dict[key]
            except KeyError:
                raise ValueError("feed_dict is missing %r" % (what,)) from None

        has = lambda k: any(f is k for f in fl)
        res = {}
        if has(m.logits):
            res[id(m.logits)] = m.predict(feed(m.user_input, m.user_input), feed(m.item_input, m.item_input),
                                          feed(m.categories, m.categories))
        need_train = has(m.train_op) or has(m.loss_value)
        need_write = has(m.personal) or has(m.general)
        if need_train or need_write:
            # the batch crosses to the device once, whatever is fetched (Train_recommender.py:189-199 feeds six lists)
            floats = {}
            if need_train:
                floats["labels"] = (feed(m.labels, m.labels), 1)
            if need_write:
                floats["sign"] = (feed(m.write_sign, m.write_sign), 1)
                floats["onehot"] = (feed(m.user_one_hot_label, m.user_one_hot_label), None)
            ut, dt, mt, ex = m._device_batch(feed(m.user_input, m.user_input), feed(m.item_input, m.item_input),
                                             feed(m.categories, m.categories), floats)
        if need_train:
            loss, lr = m.train_step(ut, dt, mt, ex["labels"], apply=has(m.train_op))
            res[id(m.loss_value)] = np.float32(loss)
            res[id(m.train_op)] = None
            res["lr"] = np.float32(lr)
        if need_write:
            pmean, gmean = m.write_memory(ut, dt, mt, ex["sign"], ex["onehot"],
                                          personal=has(m.personal), general=has(m.general))
            res[id(m.personal)] = None if pmean is None else np.float32(pmean)
            res[id(m.general)] = None if gmean is None else np.float32(gmean)
        out = []
        for f in fl:
            if f is m.learning_rate:
                out.append(res.get("lr", np.float32(m.learning_rate)))
            elif f is m.epoch_increment:
                m.epoch_step += 1
                out.append(m.epoch_step)
            elif isinstance(f, str) and f == "epoch_step":
                out.append(m.epoch_step)
            else:
                out.append(res[id(f)])
        return out if as_list else out[0]
