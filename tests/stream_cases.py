"""Stream-order cases: what each entry point is asked on a side stream (the REAL request), what its device inputs hold until the
late copies land (the DECOY: another valid request of the same shapes), and the float64 restatement of both answers.

One table, ROWS, drives tests/test_gpu_stream_order.py; tests/test_stream_cases_cpu.py holds it to the conditions that keep a GPU
case from passing vacuously:

  * the decoy's answer differs from the real one in at least MIN_DIFFERENT of the lists (rank entries, table rows) or of the scores
    beyond helpers.TOL -- computed here from the float64 restatements alone (oracle/, the case modules' references, train_oracle);
  * every public method of ScoringEngine is either covered by a row (Row.covers) or listed in NOT_COVERED with its reason.

A row's inputs are numpy arrays by name; every one of them is a device tensor of the call and arrives late.  What a wrapper converts
on the host (a Python list, `.cpu()` in ops.exclusion_csr) cannot arrive late: such an argument is the same in both requests and
the row says so in `fixed`.

Sizes are those of test_gpu_readers_after_writers.py: U = 300, I = 3000, C = 4, k = 10, 4 000 pairs, head 256 x 64, one batch of
2^18 + 77 pairs for user_high_table; E = 64, and E = 200 for the padded / generic forms.  Calls under the MLP head and the profile
calls take 40 rows, not 300: their restatement is a matrix product per row.
"""
import functools
import types
import zlib

import numpy as np

import profile_cases as pc
import seen_dish_cases as sd
import slate_cases as sc
from helpers import TOL
from test_gpu_readers_after_writers import C, I, K, NBIG, NPAIRS, U, _head, _ingredients, _masks, _tables

MIN_DIFFERENT = 0.9
N_HEAD = 40                 # rows of the calls whose restatement runs the head or composes a profile
K_DEEP = 100
R_INGREDIENTS = 60          # the recipes' ingredient ids (markets)
L_LABELS = 12               # health labels of the profile calls
KINDS = ("plain", "mlp", "ing", "market")
WRITE_ARGS = (1.0, 1.0, 0.5)                       # beta_1, beta_2, alpha of the write_memory rows
TRAIN = ("adam", 0.05)                             # learner, lr of the train_step rows


def tables(E, tset=0):
    """Table set 0: what the engines are built from.  Table set 1: what the late-table cases copy in behind the blocker."""
    return _tables(E, seed=31 * tset)


@functools.lru_cache(maxsize=None)
def recipes():
    """Every dish's ingredient list (1 .. 4 ids of R_INGREDIENTS, none empty): (offsets int32[I + 1], ids int32)."""
    rng = np.random.default_rng(41)
    off = np.zeros(I + 1, np.int32)
    off[1:] = np.cumsum(rng.integers(1, 5, I))
    ids = rng.integers(0, R_INGREDIENTS, off[-1]).astype(np.int32)
    return off, ids


def cookable(market, max_missing, lists=None):
    """market_cases.restate's cookable ids for recipes() (no empty list), vectorised; the CPU test holds it to that restatement.
    `lists`: another (offsets, ids) pair in place of recipes() (writer_cases.py: set_recipes again)."""
    off, ids = recipes() if lists is None else lists
    present = np.zeros(R_INGREDIENTS, bool)
    present[np.asarray(market, np.int64)] = True
    missing = np.add.reduceat((~present[ids]).astype(np.int64), off[:-1])
    return np.flatnonzero(missing <= max_missing)


class Model:
    """The float64 restatement of one engine configuration on one set of tables."""

    def __init__(self, E, kind, tset=0, tabs=None, cats=None, head=None, recipes=None):
        """cats / head / recipes: what a writer of writer_cases.py left in place of the kind's own (None: the kind's own)"""
        assert kind in KINDS and (head is None or kind == "mlp") and (recipes is None or kind == "market")
        self.E, self.kind = E, kind
        self.PM, self.RE, self.CE = tables(E, tset) if tabs is None else tabs
        self.cats = _masks(3) if cats is None else cats
        self.head = (_head(E, 1) if head is None else head) if kind == "mlp" else None
        self.recipes = recipes                              # None: recipes()
        self.ing = _ingredients(E, 2) if kind == "ing" else None
        self.coef = 0.5 if kind == "mlp" else 0.99          # (a head at 0.99 hides its low-level blocks: readers-after-writers' _cfg)
        self._rows = {}

    def pairs(self, users, items, cats=None, PM=None, head=True):
        from oracle import m2d_oracle as oracle
        PM = self.PM if PM is None else PM
        users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
        cats = self.cats[items] if cats is None else cats
        with np.errstate(invalid="ignore", divide="ignore"):
            if self.head is not None and head:
                return oracle.inference_mlp(PM, self.RE, self.CE, self.cats, *self.head, users, items, coef=self.coef)
            if self.ing is not None:
                return oracle.inference_ingredients(PM, self.RE, *self.ing, users, items, cats, self.coef)
            return oracle.inference_f64(PM, self.RE, self.CE, users, items, cats, self.coef)

    def rows(self, users, PM=None, head=True):
        """[len(users), I]: every listed user's scores over the whole catalogue (cached per user on the model's own tables)."""
        assert self.ing is None              # (the ingredient restatement rebuilds H per call: pairs only)
        every = np.arange(I)
        out = np.empty((len(users), I))
        for j, u in enumerate(users):
            key = (int(u), head)
            if PM is not None or key not in self._rows:
                row = self.pairs(np.full(I, int(u)), every, PM=PM, head=head)
                if PM is not None:
                    out[j] = row
                    continue
                self._rows[key] = row
            out[j] = self._rows[key]
        return out


@functools.lru_cache(maxsize=None)
def model(E, kind, tset=0):
    return Model(E, kind, tset)


# ---- how far two answers are apart ------------------------------------------------------------------------------------------------
def different(what, a, b):
    """The share of `a` that differs from `b`: lists / rows that differ anywhere, ranks that differ, scores further apart than TOL."""
    a, b = np.asarray(a), np.asarray(b)
    if what == "lists":
        if a.shape != b.shape:               # (cookable_dishes: one list whose length is part of the answer)
            return 1.0
        return float(np.mean(np.any(a.reshape(a.shape[0], -1) != b.reshape(b.shape[0], -1), axis=1)))
    if what == "ranks":
        return float(np.mean(a != b))
    a, b = a.astype(np.float64), b.astype(np.float64)
    far = np.abs(a - b) > TOL * np.maximum(1.0, np.abs(b))
    if what == "rows":
        return float(np.mean(np.any(far.reshape(far.shape[0], -1), axis=1)))
    assert what == "scores"
    return float(np.mean(far))


Answer = types.SimpleNamespace


def lists_among(S, k, allowed=None, excluded=None):
    """The answer "lists": [n, k] ids, row j's first k of slate_cases.exact_lists' order over allowed[j] (default: every dish) less
    excluded[j] (-1 where fewer remain); with it the score rows S and the dishes each row was ranked over (what a check of a GPU list
    against the restatement needs)."""
    out = np.full((len(S), k), -1, np.int64)
    among = []
    for j, row in enumerate(S):
        ids = np.arange(I) if allowed is None else np.asarray(allowed[j], np.int64)
        if excluded is not None and len(excluded[j]):
            ids = np.setdiff1d(ids, np.asarray(excluded[j], np.int64))
        got = sc.exact_lists(row[ids][None, :], ids, k)[1][0]
        out[j, :len(got)] = got
        among.append(ids)
    return Answer(what="lists", value=out, S=S, among=among)


def scores(value):
    return Answer(what="scores", value=np.asarray(value, np.float64))


def csr_lists(off, ids):
    return [ids[off[j]:off[j + 1]] for j in range(len(off) - 1)]


# ---- requests: every generator returns (real, decoy), dicts of numpy arrays of equal shapes ---------------------------------------
def _other(rng, x, n):
    """ids of [0, n) that differ from x at every position"""
    return ((np.asarray(x, np.int64) + rng.integers(1, n, np.shape(x))) % n).astype(np.int32)


def _segments(rng, n, lo, hi, upper):
    """n ascending id segments of lo .. hi ids below `upper`, and the same number of ids in other segments of other lengths: the
    decoy's lengths are the real ones reversed, so both CSR pairs have the same shapes and every offset but the ends differs."""
    lens = rng.integers(lo, hi + 1, n)
    if (lens == lens[::-1]).all():
        lens[0] += 1
    out = []
    for ln in (lens, lens[::-1]):
        off = np.zeros(n + 1, np.int64)
        np.cumsum(ln, out=off[1:])
        ids = np.concatenate([np.sort(rng.choice(upper, int(x), replace=False)) for x in ln]).astype(np.int32)
        out.append((off, ids))
    return out


def req_pairs(B):
    def make(rng, m):
        users, items = rng.integers(0, U, B).astype(np.int32), rng.integers(0, I, B).astype(np.int32)
        real, decoy = dict(users=users, items=items), dict(users=_other(rng, users, U), items=_other(rng, items, I))
        for d in (real, decoy):
            d["cats"] = m.cats[d["items"]]
        return real, decoy
    return make


def req_users(n, excl=None, held=False):
    """n distinct users (the decoy's: the same ones rotated), with `excl` = (lo, hi) a CSR pair of excluded dishes per user"""
    def make(rng, m):
        users = rng.permutation(U)[:n].astype(np.int32)
        real, decoy = dict(users=users), dict(users=np.roll(users, 7))
        if excl is not None:
            (real["excl_off"], real["excl_ids"]), (decoy["excl_off"], decoy["excl_ids"]) = _segments(rng, n, excl[0], excl[1], I)
        if held:
            real["held"] = rng.integers(0, I, n).astype(np.int32)
            decoy["held"] = _other(rng, real["held"], I)
        return real, decoy
    return make


def req_candidates(nseg, L):
    def make(rng, m):
        out = []
        users = rng.permutation(U)[:nseg].astype(np.int32)
        for u in (users, np.roll(users, 5)):
            items = np.stack([rng.permutation(I)[:L] for _ in range(nseg)]).astype(np.int32)      # distinct within a segment
            out.append(dict(users=u, items=items, lens=rng.integers(K + 1, L + 1, nseg).astype(np.int32)))
        if (out[0]["lens"] == out[1]["lens"]).all():
            out[1]["lens"][0] = K + 1 + (out[1]["lens"][0] - K) % (L - K)
        return out
    return make


def req_slate(n, nD):
    def make(rng, m):
        users = rng.permutation(U)[:n].astype(np.int32)
        return tuple(dict(users=u, slate=np.sort(rng.choice(I, nD, replace=False)).astype(np.int32)) for u in (users, np.roll(users, 9)))
    return make


def req_groups(nG, M, excl=None, slate=0):
    def make(rng, m):
        out = []
        for _ in range(2):
            members = np.stack([rng.choice(U, M, replace=False) for _ in range(nG)]).astype(np.int32)
            short = rng.integers(1, M + 1, nG)
            members[np.arange(M)[None, :] >= short[:, None]] = -1                                   # -1 padding behind the members
            d = dict(members=members)
            if slate:
                d["slate"] = np.sort(rng.choice(I, slate, replace=False)).astype(np.int32)
            out.append(d)
        if excl is not None:
            (out[0]["excl_off"], out[0]["excl_ids"]), (out[1]["excl_off"], out[1]["excl_ids"]) = _segments(rng, nG, excl[0], excl[1], I)
        return out
    return make


def req_market(n):
    def make(rng, m):
        users = rng.permutation(U)[:n].astype(np.int32)
        return tuple(dict(users=u, market=rng.choice(R_INGREDIENTS, 30, replace=False).astype(np.int32)) for u in (users, np.roll(users, 3)))
    return make


def req_markets(nQ, excl=None, profiles=False):
    def make(rng, m):
        real, decoy = req_profiles(nQ, excl=excl)(rng, m) if profiles else req_users(nQ)(rng, m)
        excl_here = None if profiles else excl
        (real["market_off"], real["market_ids"]), (decoy["market_off"], decoy["market_ids"]) = _segments(rng, nQ, 20, 40, R_INGREDIENTS)
        if excl_here is not None:
            (real["excl_off"], real["excl_ids"]), (decoy["excl_off"], decoy["excl_ids"]) = _segments(rng, nQ, excl[0], excl[1], I)
        return real, decoy
    return make


def req_profiles(n, pairs=0, excl=None):
    """label rows (one to three labels of weight 1 or 2), General_Memory and the users (one in five a guest, -1): all three late"""
    def make(rng, m):
        out = []
        for _ in range(2):
            labels = np.zeros((n, L_LABELS), np.float32)
            for q in range(n):
                labels[q, rng.choice(L_LABELS, int(rng.integers(1, 4)), replace=False)] = rng.choice([1.0, 2.0])
            users = rng.permutation(U)[:n].astype(np.int32)
            users[rng.random(n) < 0.2] = -1
            d = dict(labels=labels, gm=(rng.standard_normal((L_LABELS, C + 1, m.E)) / 4).astype(np.float32), users=users)
            if pairs:
                d["rows"], d["items"] = rng.integers(0, n, pairs).astype(np.int32), rng.integers(0, I, pairs).astype(np.int32)
            out.append(d)
        if excl is not None:
            (out[0]["excl_off"], out[0]["excl_ids"]), (out[1]["excl_off"], out[1]["excl_ids"]) = _segments(rng, n, excl[0], excl[1], I)
        return out
    return make


def req_write(B=U, L=7):
    """Write_Memory of one pair per user (distinct users: a Personal_Memory row receives one add)"""
    def make(rng, m):
        out = []
        for _ in range(2):
            items = rng.integers(0, I, B).astype(np.int32)
            y = (rng.random((B, L)) < 0.3).astype(np.float32)
            y[:, 0] = 1
            out.append(dict(users=rng.permutation(U)[:B].astype(np.int32), items=items, cats=m.cats[items],
                            sign=np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32), labels=y,
                            gm=(rng.standard_normal((L, C + 1, m.E)) / 4).astype(np.float32)))
        while (out[0]["users"] == out[1]["users"]).any():
            out[1]["users"] = rng.permutation(U)[:B].astype(np.int32) if B < U else np.roll(out[0]["users"], int(rng.integers(1, U)))
        return out
    return make


def req_train(B):
    def make(rng, m):
        out = []
        for _ in range(2):
            items = rng.integers(0, I, B).astype(np.int32)
            out.append(dict(users=(rng.permutation(max(B, U))[:B] % U).astype(np.int32), items=items, cats=m.cats[items],
                            labels=rng.integers(0, 2, B).astype(np.float32)))
        return out
    return make


# ---- answers: float64 restatements, (kind of answer, array) ------------------------------------------------------------------------
def ans_pairs(head=True):
    return lambda m, d: scores(m.pairs(d["users"], d["items"], d["cats"], head=head))


def ans_topk(k=K, head=False):
    def ans(m, d):
        excluded = csr_lists(d["excl_off"], d["excl_ids"]) if "excl_off" in d else None
        return lists_among(m.rows(d["users"], head=head), k, excluded=excluded)
    return ans


def ans_candidates(head=False):
    def ans(m, d):
        S = m.rows(d["users"], head=head)
        return lists_among(S, K, allowed=[d["items"][s, :d["lens"][s]] for s in range(len(S))])
    return ans


def rank_exclusions(d, fixed_excl=None):
    """per query the excluded dishes of a catalogue_rank request: its late CSR pair, or the lists fixed on the host"""
    return csr_lists(d["excl_off"], d["excl_ids"]) if "excl_off" in d else fixed_excl


def ans_rank(fixed_excl=None, head=False):
    def ans(m, d):
        S = m.rows(d["users"], head=head)
        excl = rank_exclusions(d, fixed_excl)
        return Answer(what="ranks", value=np.array([sd.host_rank(S[q], int(d["held"][q]), excl[q]) for q in range(len(S))]), S=S)
    return ans


def ans_rerank(candidates):
    """topk_users_mlp(candidates = K1): the K1 best by the reference score, ranked again under the head"""
    def ans(m, d):
        first = lists_among(m.rows(d["users"], head=False), candidates).value
        return lists_among(m.rows(d["users"], head=True), K, allowed=list(first))
    return ans


def ans_slate(k=0):
    def ans(m, d):
        S = m.rows(d["users"])
        return lists_among(S, k, allowed=[d["slate"]] * len(S)) if k else scores(S[:, d["slate"]])
    return ans


def group_rows(m, members, mode):
    """[nG, I] float64: least misery / mean / most pleasure of the members' scores (no NaN here: every dish has a category)"""
    fn = {"least": np.min, "mean": np.mean, "most": np.max}[mode]
    return np.stack([fn(m.rows(g[g >= 0]), axis=0) for g in members])


def ans_groups(mode, k=K):
    def ans(m, d):
        S = group_rows(m, d["members"], mode)
        if not k:
            return scores(S[:, d["slate"]])
        return lists_among(S, k, allowed=[d["slate"]] * len(S) if "slate" in d else None,
                                    excluded=csr_lists(d["excl_off"], d["excl_ids"]) if "excl_off" in d else None)
    return ans


def composed(m, d):
    return pc.restate(m.PM, d["gm"], d["labels"], d["users"], 0.5).reshape(-1, C + 1, m.E)


def ans_profiles(what):
    def ans(m, d):
        PMc = composed(m, d)
        n = len(PMc)
        if what == "compose":
            return scores(PMc)
        if what == "score":
            return scores(m.pairs(d["rows"], d["items"], PM=PMc))
        S = m.rows(np.arange(n), PM=PMc)
        allowed = [cookable(x, 1, m.recipes) for x in csr_lists(d["market_off"], d["market_ids"])] if what == "markets" else None
        return lists_among(S, K, allowed=allowed, excluded=csr_lists(d["excl_off"], d["excl_ids"]) if "excl_off" in d else None)
    return ans


def ans_market(which):
    def ans(m, d):
        if which == "cookable":
            return Answer(what="lists", value=cookable(d["market"], 1, m.recipes)[None, :], S=None, among=None)
        S = m.rows(d["users"])
        if which == "one":
            return lists_among(S, K, allowed=[cookable(d["market"], 1, m.recipes)] * len(S))
        return lists_among(S, K, allowed=[cookable(x, 1, m.recipes) for x in csr_lists(d["market_off"], d["market_ids"])],
                                    excluded=csr_lists(d["excl_off"], d["excl_ids"]) if "excl_off" in d else None)
    return ans


def written_tables(m, d):
    from oracle import m2d_oracle as oracle
    return oracle.write_memory_scatter(m.PM, m.RE, m.CE, d["gm"], d["users"], d["items"], d["cats"], d["sign"], d["labels"], *WRITE_ARGS,
                                       general=False)[0]


def trained_tables(m, d):
    from oracle import train_oracle
    st = train_oracle.TrainState(m.PM, m.RE, m.CE, learner=TRAIN[0], lr=TRAIN[1], coef=m.coef)
    st.step(d["users"], d["items"], d["cats"], d["labels"])
    return st.PM, st.RE, st.CE


def ans_write(m, d):
    return Answer(what="rows", value=written_tables(m, d))


def ans_train(m, d):
    """[U_high ; Recipe_Embedding] after the step, a row per user and per dish"""
    PM, RE, CE = trained_tables(m, d)
    return Answer(what="rows", value=np.concatenate([PM[:, 0, :], RE]))


def touched_by_train(d):
    """The rows of ans_train's matrix that the request's step moves: its users' high-level rows, its dishes' rows.  A row no pair of
    the batch names gets no gradient and stays as it was under any request, so only these can tell two requests apart."""
    return np.unique(np.concatenate([d["users"].astype(np.int64), U + d["items"].astype(np.int64)]))


# ---- calls (eng: a ScoringEngine; t: the request as device tensors by name) -------------------------------------------------------
def _excl(t):
    return (t["excl_off"], t["excl_ids"]) if "excl_off" in t else None


def call_into(eng, t):
    import torch
    n = t["users"].numel()
    out_s = torch.empty((n, K), dtype=torch.float32, device=eng.device)
    out_i = torch.empty((n, K), dtype=torch.int32, device=eng.device)
    eng.topk_users_into(t["users"], K, out_s, out_i)
    return out_s, out_i


def call_write(eng, t):
    eng.write_memory(t["users"], t["items"], t["cats"], t["sign"], t["labels"], t["gm"], *WRITE_ARGS, write_pm=True, write_gm=False)
    return (eng.pm,)


def call_train(eng, t):
    out = eng.train_step(t["users"], t["items"], t["cats"], t["labels"])
    return out, eng.pm, eng.re, eng.ce


def call_market(eng, t):
    s, i, count = eng.topk_market(t["users"], t["market"], K, 1)
    return s, i


Row = types.SimpleNamespace


def _row(name, covers, kind, E, make, call, answer, options=None, fixed="", prepare=None, exact=True, select=None):
    """name; the ScoringEngine methods the row covers; engine kind and width; request generator; the call; the float64 answer;
    options set on both engines; the arguments that cannot arrive late; `prepare(eng)` run on both engines before the case (default
    stream, synchronised); exact: the outputs equal the twin's bit for bit (False: within TOL -- the writers add with float
    atomics, "order-dependent in the last bits", csrc/m2d_train.hip); select(real request): the rows of the answer that the
    decoy condition looks at (default: all)."""
    return Row(name=name, covers=tuple(covers), kind=kind, E=E, make=make, call=call, answer=answer, options=dict(options or {}),
               fixed=fixed, prepare=prepare, exact=exact, select=select)


def _fixed_excl():
    rng = np.random.default_rng(97)
    return [np.sort(rng.choice(I, 20, replace=False)).tolist() for _ in range(U)]


FIXED_EXCL = _fixed_excl()


def _train_begin(eng):
    eng.train_begin(*TRAIN)


def _rows():
    rows = []
    add = lambda *a, **kw: rows.append(_row(*a, **kw))
    pairs = lambda eng, t: (eng.score_pairs(t["users"], t["items"], t["cats"]),)
    for E in (64, 200):
        add("score_pairs-E%d" % E, ["score_pairs"], "plain", E, req_pairs(NPAIRS), pairs, ans_pairs())
        add("score_pairs_bydish-E%d" % E, ["score_pairs_bydish"], "plain", E, req_pairs(NPAIRS),
            lambda eng, t: (eng.score_pairs_bydish(t["users"], t["items"]),), ans_pairs())
        for form in (0, 1):
            add("score_pairs_mlp-form%d-E%d" % (form, E), ["score_pairs_mlp"], "mlp", E, req_pairs(NPAIRS),
                lambda eng, t: (eng.score_pairs_mlp(t["users"], t["items"]),), ans_pairs(), options={"mlp_bf16x3": 1, "mlp_form": form})
        add("topk_users-E%d" % E, ["topk_users"], "plain", E, req_users(U), lambda eng, t: eng.topk_users(t["users"], K), ans_topk())
        add("topk_users_excluding-E%d" % E, ["topk_users_excluding"], "plain", E, req_users(U, excl=(0, 40)),
            lambda eng, t: eng.topk_users_excluding(t["users"], K, _excl(t)), ans_topk())
    add("score_pairs-user_high_table", ["score_pairs"], "plain", 64, req_pairs(NBIG), pairs, ans_pairs(), options={"user_high_table": 1})
    add("score_pairs-pm_bf16", ["score_pairs"], "plain", 64, req_pairs(NPAIRS), pairs, ans_pairs(), options={"pm_bf16": 1})
    add("score_pairs_ingredients", ["score_pairs_ingredients"], "ing", 64, req_pairs(NPAIRS),
        lambda eng, t: (eng.score_pairs_ingredients(t["users"], t["items"]),), ans_pairs())
    add("score_pairs_mlp-bucketed", ["score_pairs_mlp"], "mlp", 64, req_pairs(16384 + 77),
        lambda eng, t: (eng.score_pairs_mlp(t["users"], t["items"]),), ans_pairs(), options={"mlp_bf16x3": 1, "mlp_form": 0})
    ranked = lambda head: (lambda eng, t: eng.rank_candidates(t["users"], t["items"], K, lens=t["lens"], head=head))
    add("rank_candidates", ["rank_candidates"], "plain", 64, req_candidates(64, 100), ranked(False), ans_candidates())
    add("rank_candidates-head", ["rank_candidates"], "mlp", 64, req_candidates(N_HEAD, 100), ranked(True), ans_candidates(head=True))
    topk = lambda eng, t: eng.topk_users(t["users"], K)
    add("topk_users-f32", ["topk_users"], "plain", 64, req_users(U), topk, ans_topk(), options={"topk_bf16x3": 0})
    add("topk_users-dense", ["topk_users"], "plain", 64, req_users(U), topk, ans_topk(), options={"variant": 7})
    add("topk_users-ranges103", ["topk_users"], "plain", 64, req_users(U), topk, ans_topk(), options={"variant": 103})
    add("topk_users-ranges228", ["topk_users"], "plain", 64, req_users(U), topk, ans_topk(), options={"variant": 228})
    add("topk_users_into", ["topk_users_into"], "plain", 64, req_users(U), call_into, ans_topk())
    add("topk_users_excluding-tier2", ["topk_users_excluding"], "plain", 64, req_users(U, excl=(0, 40)),
        lambda eng, t: eng.topk_users_excluding(t["users"], K, _excl(t)), ans_topk(), options={"topk_excl_tier": 2})
    add("catalogue_rank", ["catalogue_rank"], "plain", 64, req_users(U, held=True),
        lambda eng, t: eng.catalogue_rank(t["users"], t["held"], FIXED_EXCL), ans_rank(FIXED_EXCL),
        fixed="exclude: catalogue_rank(head=False) sorts its lists on the host (exclusions_on_device(as_is=False))")
    add("catalogue_rank-head", ["catalogue_rank"], "mlp", 64, req_users(N_HEAD, excl=(0, 40), held=True),
        lambda eng, t: eng.catalogue_rank(t["users"], t["held"], _excl(t), head=True), ans_rank(head=True))
    add("topk_users_deep", ["topk_users_deep"], "plain", 64, req_users(U, excl=(0, 40)),
        lambda eng, t: eng.topk_users_deep(t["users"], K_DEEP, _excl(t)), ans_topk(K_DEEP))
    add("topk_users_mlp", ["topk_users_mlp"], "mlp", 64, req_users(N_HEAD), lambda eng, t: eng.topk_users_mlp(t["users"], K),
        ans_topk(head=True))
    add("topk_users_mlp-candidates", ["topk_users_mlp"], "mlp", 64, req_users(N_HEAD),
        lambda eng, t: eng.topk_users_mlp(t["users"], K, candidates=64), ans_rerank(64))
    add("topk_users_mlp_excluding", ["topk_users_mlp_excluding"], "mlp", 64, req_users(N_HEAD, excl=(0, 40)),
        lambda eng, t: eng.topk_users_mlp_excluding(t["users"], K, _excl(t)), ans_topk(head=True))
    add("topk_users_mlp_deep", ["topk_users_mlp_deep"], "mlp", 64, req_users(N_HEAD, excl=(0, 40)),
        lambda eng, t: eng.topk_users_mlp_deep(t["users"], K_DEEP, _excl(t)), ans_topk(K_DEEP, head=True))
    add("score_slate", ["score_slate"], "plain", 64, req_slate(U, 150), lambda eng, t: (eng.score_slate(t["users"], t["slate"]),),
        ans_slate())
    add("topk_slate", ["topk_slate"], "plain", 64, req_slate(U, 150), lambda eng, t: eng.topk_slate(t["users"], t["slate"], K), ans_slate(K))
    for mode in ("least", "mean", "most"):
        add("topk_groups-" + mode, ["topk_groups"], "plain", 64, req_groups(40, 4),
            lambda eng, t, mode=mode: eng.topk_groups(t["members"], K, mode), ans_groups(mode))
        add("score_groups-" + mode, ["score_groups"], "plain", 64, req_groups(40, 4, slate=150),
            lambda eng, t, mode=mode: (eng.score_groups(t["members"], t["slate"], mode),), ans_groups(mode, k=0))
    add("topk_groups-excluding", ["topk_groups"], "plain", 64, req_groups(40, 4, excl=(0, 40)),
        lambda eng, t: eng.topk_groups(t["members"], K, "least", exclude=_excl(t)), ans_groups("least"))
    add("topk_groups-among", ["topk_groups"], "plain", 64, req_groups(40, 4, slate=150),
        lambda eng, t: eng.topk_groups(t["members"], K, "mean", among=t["slate"]), ans_groups("mean"))
    add("cookable_dishes", ["cookable_dishes"], "market", 64, req_market(N_HEAD), lambda eng, t: (eng.cookable_dishes(t["market"], 1),),
        ans_market("cookable"))
    add("topk_market", ["topk_market"], "market", 64, req_market(N_HEAD), call_market, ans_market("one"))
    add("topk_markets", ["topk_markets"], "market", 64, req_markets(60),
        lambda eng, t: eng.topk_markets(t["users"], (t["market_off"], t["market_ids"]), K, 1, return_counts=True), ans_market("each"))
    add("topk_markets_excluding", ["topk_markets_excluding"], "market", 64, req_markets(60, excl=(0, 40)),
        lambda eng, t: eng.topk_markets_excluding(t["users"], (t["market_off"], t["market_ids"]), _excl(t), K, 1, return_counts=True),
        ans_market("each"))
    add("compose_profiles", ["compose_profiles"], "plain", 64, req_profiles(N_HEAD),
        lambda eng, t: (eng.compose_profiles(t["labels"], t["gm"], t["users"], 0.5),), ans_profiles("compose"))
    add("topk_profiles", ["topk_profiles"], "plain", 64, req_profiles(N_HEAD),
        lambda eng, t: eng.topk_profiles(t["labels"], t["gm"], K, t["users"], 0.5), ans_profiles("topk"))
    add("topk_profiles-excluding", ["topk_profiles"], "plain", 64, req_profiles(N_HEAD, excl=(0, 40)),
        lambda eng, t: eng.topk_profiles(t["labels"], t["gm"], K, t["users"], 0.5, exclude=_excl(t)), ans_profiles("topk"))
    add("score_profiles", ["score_profiles"], "plain", 64, req_profiles(N_HEAD, pairs=2000),
        lambda eng, t: (eng.score_profiles(t["labels"], t["gm"], t["rows"], t["items"], t["users"], 0.5),), ans_profiles("score"))
    add("topk_markets_profiles", ["topk_markets_profiles"], "market", 64, req_markets(N_HEAD, profiles=True),
        lambda eng, t: eng.topk_markets_profiles(t["labels"], t["gm"], (t["market_off"], t["market_ids"]), K, t["users"], 0.5, max_missing=1),
        ans_profiles("markets"))
    add("topk_markets_profiles-excluding", ["topk_markets_profiles"], "market", 64, req_markets(N_HEAD, excl=(0, 40), profiles=True),
        lambda eng, t: eng.topk_markets_profiles(t["labels"], t["gm"], (t["market_off"], t["market_ids"]), K, t["users"], 0.5,
                                                 exclude=_excl(t), max_missing=1), ans_profiles("markets"))
    # (one pair per user: a Personal_Memory row receives ONE add, which no order of the atomics can change -- bit for bit)
    add("write_memory", ["write_memory"], "plain", 64, req_write(), call_write, ans_write,
        fixed="beta_1, beta_2, alpha: host scalars")
    for B in (128, 1100):                    # the fused step and the nine-launch form
        add("train_step-B%d" % B, ["train_step"], "plain", 64, req_train(B), call_train, ans_train, prepare=_train_begin, exact=False,
            select=touched_by_train)
    return rows


def req_users_tripled(rng, m):
    users = np.concatenate([rng.permutation(U) for _ in range(3)]).astype(np.int32)
    return dict(users=users), dict(users=np.roll(users, 11))


def _chain(kind):
    """The chain of calls behind one blocker, in order: topk_users, rank_candidates at L = 1024, score_pairs on the big batch,
    topk_users_excluding, topk_slate, topk_users with three times the users (the scratch grows in the middle of the chain),
    score_pairs_mlp.  topk_users_excluding and topk_slate refuse an engine with a head and score_pairs_mlp needs one: the chain
    without a head leaves out its last step, the chain with a head those two.  Rows like any other: a decoy, a float64 answer."""
    rows = []
    add = lambda name, *a, **kw: rows.append(_row("chain-%s-%s" % (kind, name), *a, **kw))
    topk = lambda eng, t: eng.topk_users(t["users"], K)
    add("topk_users", ["topk_users"], kind, 64, req_users(U), topk, ans_topk())
    add("rank_candidates", ["rank_candidates"], kind, 64, req_candidates(64, 1024),
        lambda eng, t: eng.rank_candidates(t["users"], t["items"], K, lens=t["lens"]), ans_candidates())
    add("score_pairs", ["score_pairs"], kind, 64, req_pairs(NBIG), lambda eng, t: (eng.score_pairs(t["users"], t["items"], t["cats"]),),
        ans_pairs(head=False))
    if kind == "plain":
        add("topk_users_excluding", ["topk_users_excluding"], kind, 64, req_users(U, excl=(0, 40)),
            lambda eng, t: eng.topk_users_excluding(t["users"], K, _excl(t)), ans_topk())
        add("topk_slate", ["topk_slate"], kind, 64, req_slate(U, 150), lambda eng, t: eng.topk_slate(t["users"], t["slate"], K), ans_slate(K))
    add("topk_users_tripled", ["topk_users"], kind, 64, req_users_tripled, topk, ans_topk())
    if kind == "mlp":
        add("score_pairs_mlp", ["score_pairs_mlp"], kind, 64, req_pairs(NPAIRS), lambda eng, t: (eng.score_pairs_mlp(t["users"], t["items"]),),
            ans_pairs())
    return rows


ROWS = _rows()
CHAINS = {kind: _chain(kind) for kind in ("plain", "mlp")}
BY_NAME = {r.name: r for r in ROWS + CHAINS["plain"] + CHAINS["mlp"]}
assert len(BY_NAME) == len(ROWS) + len(CHAINS["plain"]) + len(CHAINS["mlp"])

# Public methods of ScoringEngine without a late-input row, each with its reason.
NOT_COVERED = {
    "set_user_base": "setter: host value, no launch",
    "set_dish_categories": "setter: synchronous by design (null stream; out of scope per the stream contract's setter rule)",
    "set_ingredients": "setter: synchronous by design (builds H and validates the CSR, then waits)",
    "clear_ingredients": "setter: host state only",
    "set_mlp_head": "setter: synchronous by design",
    "clear_mlp_head": "setter: host state only",
    "set_recipes": "setter: validates once and synchronises",
    "clear_recipes": "setter: host state only",
    "train_begin": "setter: allocates the optimizer slots and waits",
    "train_slot": "checkpoint copy of a slot: a plain stream-ordered copy, no kernel reads a request",
    "train_steps": "host-only argument; synchronises the device by design",
    "train_end": "synchronises the device by design",
    "tables_updated": "host flags only; the late-table cases call it between the copies and the reader",
    "personal_memory_bf16": "no request: takes no device input; its build is the pm_bf16 row's",
    "set_option": "setter: a host value, no launch",
    "get_option": "host value (the diagnostics synchronise the device by design)",
    "last_kernel": "host value: the name the last launcher left",
    "score_pairs_host": "host-only arguments (numpy in, numpy out): the call waits for its own work",
    "stream_read_probe": "probe (calibration only)",
    "check": "the synchronising call every case ends with",
    "close": "destructor: frees the engine, no request",
}


@functools.lru_cache(maxsize=None)
def request(name):
    """(real, decoy) of a row: read-only numpy arrays by name"""
    r = BY_NAME[name]
    real, decoy = r.make(np.random.default_rng(zlib.crc32(name.encode())), model(r.E, r.kind))
    assert real.keys() == decoy.keys()
    for d in (real, decoy):
        for k, a in d.items():
            d[k] = np.ascontiguousarray(a)
            d[k].setflags(write=False)
    assert all(real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype for k in real), name
    return real, decoy


@functools.lru_cache(maxsize=None)
def answers(name):
    """(the real request's answer, the decoy's) from the float64 restatement"""
    r = BY_NAME[name]
    m = model(r.E, r.kind)
    real, decoy = request(name)
    return r.answer(m, real), r.answer(m, decoy)


def decoy_share(name):
    """The share of the real answer that the decoy's answer differs in (the rows the row's `select` names, where it has one)."""
    r = BY_NAME[name]
    a, b = answers(name)
    assert a.what == b.what
    va, vb = a.value, b.value
    if r.select is not None:
        rows = r.select(request(name)[0])
        va, vb = va[rows], vb[rows]
    return different(a.what, va, vb)


# ---- late errors: row -> (the input that carries the bad user id, the input that carries the bad item id or None) -----------------
# The entry points with an id check of their own.  First the decoy holds BAD_USER and the real request is clean; then the real
# request holds a bad id at another position -- BAD_ITEM where the call takes item ids, BAD_USER otherwise -- and the decoy is clean.
BAD_USER, BAD_ITEM = U + 5, I + 9
ERRORS = {
    "score_pairs-E64": ("users", "items"),
    "topk_users-E64": ("users", None),
    "topk_users_excluding-E64": ("users", "excl_ids"),
    "score_slate": ("users", "slate"),
    "topk_groups-least": ("members", None),
    "topk_markets": ("users", None),
    "compose_profiles": ("users", None),
    "write_memory": ("users", "items"),
    "train_step-B128": ("users", "items"),
}


def with_bad_id(d, key, position, value):
    """a copy of request d whose input `key` holds `value` at flat position `position`"""
    out = dict(d)
    a = d[key].copy()
    a.reshape(-1)[position] = value
    out[key] = a
    return out
