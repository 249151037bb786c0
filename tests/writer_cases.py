"""Readers after writers, the whole matrix: every reader call the engine has against every call that writes what the readers see
(tests/test_gpu_readers_after_writers_all.py on the GPU; tests/test_writer_cases_cpu.py holds the table to the conditions that keep
a GPU case from passing on stale state).  Nothing here needs a GPU.

ONE READER TABLE, READERS: every row of stream_cases.ROWS that is no writer, asked its REAL request, and four rows of the same shape
for the menu family's engine calls (_topk_menu, _topk_menu_filtered, _plan_menus, _plan_groups), which ScoringEngine keeps private and
stream_cases therefore cannot list (and one for score_pairs_host, whose arguments are host arrays).  The menu rows' answers are the features' own restatements over a matrix of float32 score words:
the float64 restatement's here (what decides `expected`), the engine's own score words on the GPU, as those features' tests do.

ONE WRITER TABLE, WRITERS: a name, the engine kinds it applies to, and steps.  A step has apply(eng, state) -- the call on the
engine -- and after(state) -- what the ORACLE's writer leaves: the float64 Write_Memory scatter, train_oracle's step, the edited
arrays, the new masks, head or recipes.  A writer of several steps is read after every step (writer, reader, writer, reader).

expected(kind, writer, step, reader) is decided by DATA: the row's answer restated on the state before the step and on the state
after it -- identical: "same" (the GPU answer must be bit-equal); a share of change at or above the thresholds of
test_gpu_readers_after_writers._assert_changed (more than 0.25 of the lists or ranks, more than 0.5 of the scores beyond
helpers.TOL): "changed"; in between: "weak", a badly chosen case that the CPU test fails on.  "refuses" comes from the one condition
under which a reader of a kind's own tables refuses: masks that are not 0/1 (refuses_weighted, with its source).

Sizes are those of test_gpu_readers_after_writers.py (stream_cases' docstring).
"""
import functools
import types
import zlib

import numpy as np

import group_cases as gc
import menu_cases as mc
import menu_filtered_cases as mf
import plan_cases as pc
import plan_group_cases as pg
import stream_cases as st
from test_gpu_readers_after_writers import C, I, K, U, _head, _ingredients, _masks

# engine kind of the GPU matrix -> (stream_cases kind, E).  "ing": the ingredient table is set (train_begin refuses such an engine)
ENGINE_KINDS = {"plain": ("plain", 64), "mlp": ("mlp", 64), "market": ("market", 64), "plain200": ("plain", 200), "mlp200": ("mlp", 200),
                "ing": ("ing", 64)}
WRITER_METHODS = ("write_memory", "train_step")
LISTS_OR_RANKS, SCORES = 0.25, 0.5           # _assert_changed's thresholds: the share must be ABOVE them
MARGIN = 0.05                                # ... and a case within this of its threshold is strengthened, not kept
N_SAMPLE = 40                                # result rows per reader that `expected` restates (all where the reader has fewer)
USER_BASE = 7000
MENU_K, PLAN_DAYS, PLAN_K, N_GROUPS, GROUP_M, SLATE_N = 10, 3, 5, 40, 4, 150


# ---- the menu family's rows ---------------------------------------------------------------------------------------------------------
def _req_menu(slate=0, excl=None, plan=False):
    def make(rng, m):
        out = []
        for _ in range(2):
            users = rng.permutation(U).astype(np.int32)
            d = dict(users=users, caps=mc.caps_all(U, C, 2))
            if plan:
                d["plan_caps"] = pc.plan_caps_of(U, C, PLAN_DAYS, PLAN_K, seed=int(rng.integers(0, 100)))
            if slate:
                d["slate"] = np.sort(rng.choice(I, slate, replace=False)).astype(np.int32)
            out.append(d)
        if excl is not None:                                 # the excluded dishes are the slate's own: each one changes a list
            segs = st._segments(rng, U, excl[0], excl[1], slate)
            for d, (off, at) in zip(out, segs):
                d["excl_off"], d["excl_ids"] = off, d["slate"][at]
        return out
    return make


def _req_plan_groups(rng, m):
    out = st.req_groups(N_GROUPS, GROUP_M)(rng, m)
    for d in out:
        d["caps"] = mc.caps_all(N_GROUPS, C, 2)
        d["plan_caps"] = pc.plan_caps_of(N_GROUPS, C, PLAN_DAYS, PLAN_K, seed=int(rng.integers(0, 100)))
    return out


def _menu_words(m, d):
    """the float64 restatement's score words of the request's rows: float32 [n, I] (for the groups: [U, I], the members' rows)"""
    if "members" not in d:
        return m.rows(d["users"], head=False).astype(np.float32)
    S = np.zeros((U, I), np.float32)
    ids = np.unique(d["members"][d["members"] >= 0])
    S[ids] = m.rows(ids, head=False)
    return S


def _restate_menu(W, cats, d):
    return mc.menu_lists(W, cats, d["caps"], MENU_K)


def _restate_filtered(W, cats, d):
    return mf.filtered_lists(W, cats, d["caps"], MENU_K, st.csr_lists(d["excl_off"], d["excl_ids"]), d["slate"])


def _restate_plan(W, cats, d):
    return pc.plan_lists(W, cats, d["caps"], d["plan_caps"], PLAN_DAYS, PLAN_K)


def _restate_groups(S, cats, d):
    return pg.group_plan(S, d["members"], gc.LEAST, cats, d["caps"], d["plan_caps"], PLAN_DAYS, PLAN_K)


def _ans_menu(restate):
    def ans(m, d):
        w, ids = restate(_menu_words(m, d), m.cats, d)
        return st.Answer(what="lists", value=ids.reshape(len(ids), -1), words=w)
    return ans


def _menu_rows():
    rows = []

    def add(name, make, call, restate):
        r = st._row(name, [name], "plain", 64, make, call, _ans_menu(restate))
        r.restate = restate                                  # (score words [n, I] or [U, I], masks, request) -> (words, ids)
        rows.append(r)
    excl = lambda t: (t["excl_off"], t["excl_ids"])
    add("_topk_menu", _req_menu(), lambda eng, t: eng._topk_menu(t["users"], MENU_K, t["caps"]), _restate_menu)
    add("_topk_menu_filtered", _req_menu(slate=SLATE_N, excl=(0, 40)),
        lambda eng, t: eng._topk_menu_filtered(t["users"], MENU_K, t["caps"], excl(t), t["slate"]), _restate_filtered)
    add("_plan_menus", _req_menu(plan=True), lambda eng, t: eng._plan_menus(t["users"], PLAN_DAYS, PLAN_K, t["caps"], t["plan_caps"]),
        _restate_plan)
    add("_plan_groups", _req_plan_groups,
        lambda eng, t: eng._plan_groups(t["members"], PLAN_DAYS, PLAN_K, t["caps"], t["plan_caps"], "least"), _restate_groups)
    # host arrays in, host array out: the snapshot hands every call its request as numpy arrays too, under "_host"
    rows.append(st._row("score_pairs_host", ["score_pairs_host"], "plain", 64, st.req_pairs(51),
                        lambda eng, t: (eng.score_pairs_host(t["_host"]["users"], t["_host"]["items"], t["_host"]["cats"]),), st.ans_pairs()))
    return rows


MENU_ROWS = _menu_rows()
MENU_CALLS = tuple(r.name for r in MENU_ROWS if r.name.startswith("_"))
READERS = [r for r in st.ROWS if not set(r.covers) & set(WRITER_METHODS)] + MENU_ROWS
BY_NAME = {r.name: r for r in READERS}
assert len(BY_NAME) == len(READERS)

# Public methods of ScoringEngine that are neither a reader nor a writer of the matrix, each with its reason.
NOT_IN_MATRIX = {
    "clear_mlp_head": "turns the engine into the kind without a head: the head's readers then refuse, nothing a kind's readers see is rewritten",
    "clear_recipes": "turns the engine into the kind without recipes: every market reader then refuses, no list is rewritten",
    "train_begin": "allocates the optimizer slots, writes no table: every train_step writer of the table starts with it",
    "train_end": "frees the optimizer slots, writes no table: every train_step writer of the table ends with it",
    "train_slot": "optimizer slots, not tables: the writer 'train_step-unapplied' reads every slot out and writes it back",
    "train_steps": "a host counter of the optimizer, no table",
    "personal_memory_bf16": "returns the mirror itself, no answer from the tables' readers: its build is the score_pairs-pm_bf16 row's",
    "set_option": "a host value: the snapshot sets and resets each reader's options around its call",
    "get_option": "a host value (the diagnostics synchronise the device by design)",
    "last_kernel": "a host value: the name the last launcher left",
    "stream_read_probe": "probe of the stream contract (calibration only)",
    "check": "the synchronising call every snapshot makes after every reader",
    "close": "destructor: frees the engine",
}


def readers_of(kind):
    skind, E = ENGINE_KINDS[kind]
    return [r for r in READERS if r.kind == skind and r.E == E]


@functools.lru_cache(maxsize=None)
def request(name):
    """a reader's REAL request: read-only numpy arrays by name (user ids before any user_base)"""
    if name in st.BY_NAME:
        return st.request(name)[0]
    r = BY_NAME[name]
    real = r.make(np.random.default_rng(zlib.crc32(name.encode())), st.model(r.E, r.kind))[0]
    for k, a in real.items():
        real[k] = np.ascontiguousarray(a)
        real[k].setflags(write=False)
    return real


# The pair calls that take no masks read the RESIDENT dish masks: the "cats" of their stream_cases request (drawn from the masks the
# engines start with) is not an argument of the call, and their restatement follows the masks of the state it is made on.
RESIDENT_MASKS = ("score_pairs_bydish", "score_pairs_ingredients")


def asked(r, d, cats):
    """the request as the restatement on a state with dish masks `cats` reads it"""
    return dict(d, cats=cats[d["items"]]) if r.covers[0] in RESIDENT_MASKS else d


def shifted(d, user_base):
    """the request under another user_base: every user id moved, fillers (-1) and guests (-1) as they are"""
    if not user_base:
        return d
    out = dict(d)
    for k in ("users", "members"):
        if k in d:
            out[k] = np.where(d[k] >= 0, d[k] + user_base, d[k]).astype(d[k].dtype)
    return out


# ---- a sample of a request's rows ---------------------------------------------------------------------------------------------------
SHARED = ("slate", "market", "gm")           # inputs every row of a request shares


def n_rows(d):
    return len(d["members"] if "members" in d else d["labels"] if "labels" in d else d["users"])


def sampled(r):
    """whether a sample of the request's rows can be asked alone: not where positions carry meaning (host lists fixed per position,
    pairs that name rows of the same request) and not where the answer is one list (cookable_dishes)"""
    return not r.fixed and r.name not in ("score_profiles", "cookable_dishes")


def subrequest(d, idx):
    """the request of rows `idx` alone"""
    idx = np.asarray(idx, np.int64)
    n = n_rows(d)
    out = {}
    for k, a in d.items():
        if k in SHARED:
            out[k] = a
        elif not k.endswith(("_off", "_ids")):
            assert len(a) == n, k
            out[k] = a[idx]
    for pre in ("excl", "market"):
        if pre + "_off" in d:
            lists = st.csr_lists(d[pre + "_off"], d[pre + "_ids"])
            out[pre + "_off"] = np.concatenate([[0], np.cumsum([len(lists[j]) for j in idx])]).astype(np.int64)
            out[pre + "_ids"] = np.concatenate([lists[j] for j in idx] + [np.zeros(0, np.int32)]).astype(np.int32)
    return out


def sample_rows(r, d, oracle=False):
    """The rows of a request that are restated (None: all).  For `expected`: the first N_SAMPLE rows, of the pairs the first 4 000.
    oracle=True, the GPU file's check of an engine's answers: every 37th row as test_gpu_readers_after_writers._assert_oracle takes
    them (every 7th of the readers of 40 rows), every pair of a batch but of the 2^18 + 77 every 64th."""
    n = n_rows(d)
    if not sampled(r):
        return None
    if "cats" in d:                                          # pairs
        limit, step = 4000, 64 if n > 20000 else 1
    else:
        limit, step = N_SAMPLE, 37 if n > 64 else 7
    if oracle:
        return np.arange(0, n, step) if step > 1 else None
    return np.arange(limit) if n > limit else None


# ---- states: what an engine holds besides its options -----------------------------------------------------------------------------
State = types.SimpleNamespace


@functools.lru_cache(maxsize=None)
def initial(kind):
    skind, E = ENGINE_KINDS[kind]
    m = st.model(E, skind)
    return State(kind=kind, skind=skind, E=E, tabs=(m.PM, m.RE, m.CE), cats=m.cats, head=m.head, ing=m.ing, coef=m.coef, user_base=0,
                 recipes=st.recipes() if skind == "market" else None, opt=None)


def _with(s, **kw):
    out = State(**vars(s))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def binary(cats):
    return bool(np.all((cats == 0) | (cats == 1)))


def model_of(s):
    """The float64 restatement of a state.  Its rows without the head are filled in at once from the oracle's factored form (score =
    <flatten(PM[u]), Dt[d]>, oracle.dish_vectors: the same float64 number by another order of the sums -- tests/test_oracle.py), one
    matrix product for all users in place of a call of the pair formula per user."""
    m = st.Model(s.E, s.skind, tabs=s.tabs, cats=s.cats, head=s.head if s.skind == "mlp" else None,
                 recipes=s.recipes if s.skind == "market" else None)
    if m.ing is None:
        from oracle import m2d_oracle as oracle
        with np.errstate(invalid="ignore", divide="ignore"):
            S = np.asarray(m.PM, np.float64).reshape(U, -1) @ oracle.dish_vectors(m.RE, m.CE, m.cats, m.coef).T
        m._rows.update({(u, False): S[u] for u in range(U)})
    return m


# m2d_rank_prepare (csrc/m2d_catalogue_rank.hip), the one place a reader refuses its own kind's tables: "needs 0/1 dish masks" -- the
# ranking scan's bound is stated for 0/1 masks.  Its callers: m2d_catalogue_rank, m2d_topk_users_excluding, and m2d_topk_profiles where
# it is given exclusion lists (m2d_profiles.hip runs m2d_topk_users_excluding's launcher on the composed rows).
def refuses_weighted(r):
    return r.name in ("catalogue_rank", "topk_profiles-excluding") or r.covers[0] == "topk_users_excluding"


# With the ingredient table set (m2d_deep_conditions, m2d_rank_prepare: "the ingredient table is set"): every call on the slate
# kernels and the ranking scans.  The methods that MUST refuse; any other reader either refuses by name too or answers as a fresh
# engine with the same ingredient table does.
REFUSE_INGREDIENTS = ("score_slate", "topk_slate", "topk_users_deep", "topk_groups", "score_groups", "catalogue_rank",
                      "topk_users_excluding") + MENU_CALLS


# ---- the writers' batches: the numpy twins of test_gpu_readers_after_writers._write_batch / _train_batch (the GPU file asserts that
# they are the same arrays, so the oracle's writer is given what the engine's is) -----------------------------------------------------
def write_batch(E, cats, B=600, L=7, seed=5):
    rng = np.random.default_rng(seed)
    users = (np.arange(B) % U).astype(np.int32)
    items = rng.integers(0, I, B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = (rng.standard_normal((L, C + 1, E)) / 4).astype(np.float32)
    return users, items, cats[items], sign, y, gm


def train_batch(cats, B, seed=11):
    rng = np.random.default_rng(seed)
    users = (rng.permutation(max(B, U))[:B] % U).astype(np.int32)
    items = rng.integers(0, I, B).astype(np.int32)
    return users, items, cats[items], rng.integers(0, 2, B).astype(np.float32)


def _cfg(s):
    """what _write_batch / _train_batch read of a configuration"""
    return types.SimpleNamespace(E=s.E, cats=s.cats, user_base=s.user_base)


def _f32(tabs):
    return tuple(np.asarray(x, np.float32) for x in tabs)


# ---- steps -------------------------------------------------------------------------------------------------------------------------
Step = types.SimpleNamespace


def step_write(write_pm, write_gm, seed=5):
    def apply(eng, s):
        from test_gpu_readers_after_writers import _write_batch
        eng.write_memory(*_write_batch(_cfg(s), seed=seed), write_pm=write_pm, write_gm=write_gm)

    def after(s):
        if not write_pm:
            return s
        from oracle import m2d_oracle as oracle
        users, items, cats, sign, y, gm = write_batch(s.E, s.cats, seed=seed)
        PM = oracle.write_memory_scatter(*s.tabs, gm, users, items, cats, sign, y, 1.0, 1.0, 0.5, general=False)[0]
        return _with(s, tabs=_f32((PM,) + tuple(s.tabs[1:])))
    return Step(name="write_memory(%s)" % "+".join(n for n, on in (("personal", write_pm), ("general", write_gm)) if on), apply=apply, after=after)


def step_train(learner, lr, B, variant=0, seed=11, kernel=None, do_apply=True):
    """one training step; the first one of a writer begins the training (train_begin) and carries the optimizer's slots along"""
    def apply(eng, s):
        from test_gpu_readers_after_writers import _train_batch
        if not getattr(eng, "_training", False):
            eng.train_begin(learner, lr)
        eng.set_option("variant", variant)
        out = eng.train_step(*_train_batch(_cfg(s), B, seed=seed), apply=do_apply)
        eng.check()
        eng.set_option("variant", 0)
        assert kernel is None or eng.last_kernel() == kernel, eng.last_kernel()
        assert np.isfinite(out.cpu().numpy()).all()
        if not do_apply:                                     # ... and an optimizer slot read out and written back is the same slot
            for tb in range(3):
                for sl in range(2):
                    eng.train_slot(tb, sl, restore=eng.train_slot(tb, sl).clone())

    def after(s):
        if not do_apply:
            return s
        import copy
        from oracle import train_oracle
        opt = copy.deepcopy(s.opt) if s.opt is not None else train_oracle.TrainState(*s.tabs, learner=learner, lr=lr, coef=s.coef)
        opt.PM, opt.RE, opt.CE = (np.array(x, np.float64) for x in s.tabs)     # (a Write_Memory may stand between two steps)
        opt.step(*train_batch(s.cats, B, seed=seed))
        return _with(s, tabs=_f32((opt.PM, opt.RE, opt.CE)), opt=opt)
    return Step(name="train_step(%s, B=%d%s%s)" % (learner, B, ", variant %d" % variant if variant else "", "" if do_apply else ", apply=False"),
                apply=apply, after=after)


def both(a, b):
    """two writers with no reader between them"""
    def apply(eng, s):
        a.apply(eng, s)
        b.apply(eng, a.after(s))
    return Step(name=a.name + " + " + b.name, apply=apply, after=lambda s: b.after(a.after(s)))


# the in-place edits: each strong enough alone (the CPU test prints the shares)
def _edit_pm(pm, lib):
    pm[:, 0] *= -1.5                                         # U_high: what the <U_high, CE_c> table and the mirror are built from
    pm[:, 1:] = lib.flip(pm[:, 1:], (2,)) * 4.0              # the low-level rows: the only ones a head's low blocks and E = 200 see


def _edit_re(re, lib):
    re[:] = lib.flip(re, (1,)) * -8.0                        # every row: the sorted dish rows and the dish vectors hold copies


def _edit_ce(ce, lib):
    ce[:] = lib.flip(ce, (0, 1)) * 1.5


def _edit_all(tabs, lib):
    """test_gpu_readers_after_writers.test_after_tables_updated's edit"""
    pm, re, ce = tabs
    re[7] *= 1000.0
    ce[:] = lib.flip(ce, (0, 1)) * 1.5
    pm[:, 0] *= -1.5


class _Numpy:
    flip = staticmethod(lambda x, dims: np.flip(x, dims).copy())


class _Torch:
    @staticmethod
    def flip(x, dims):
        import torch
        return torch.flip(x, dims=dims)


def step_edit(which):
    def edit(tabs, lib):
        if which == "all":
            _edit_all(tabs, lib)
        else:
            {"pm": _edit_pm, "re": _edit_re, "ce": _edit_ce}[which](tabs[("pm", "re", "ce").index(which)], lib)

    def apply(eng, s):
        edit((eng.pm, eng.re, eng.ce), _Torch)
        eng.tables_updated()

    def after(s):
        tabs = tuple(np.array(x, np.float32) for x in s.tabs)
        edit(tabs, _Numpy)
        return _with(s, tabs=tabs)
    return Step(name="tables_updated(%s)" % which, apply=apply, after=after)


def step_cats(seed, weighted=False):
    cats = _masks(seed, weighted)
    return Step(name="set_dish_categories(%s)" % ("weighted" if weighted else "0/1"), apply=lambda eng, s: eng.set_dish_categories(cats),
                after=lambda s: _with(s, cats=cats))


def step_head(seed):
    return Step(name="set_mlp_head", apply=lambda eng, s: eng.set_mlp_head(*_head(s.E, seed)), after=lambda s: _with(s, head=_head(s.E, seed)))


@functools.lru_cache(maxsize=None)
def other_recipes():
    """other lists for every dish: stream_cases.recipes()' shape from another seed"""
    rng = np.random.default_rng(43)
    off = np.zeros(I + 1, np.int32)
    off[1:] = np.cumsum(rng.integers(1, 5, I))
    return off, rng.integers(0, st.R_INGREDIENTS, off[-1]).astype(np.int32)


STEP_RECIPES = Step(name="set_recipes", apply=lambda eng, s: eng.set_recipes(*other_recipes(), st.R_INGREDIENTS),
                    after=lambda s: _with(s, recipes=other_recipes()))
STEP_USER_BASE = Step(name="set_user_base", apply=lambda eng, s: eng.set_user_base(USER_BASE), after=lambda s: _with(s, user_base=USER_BASE))


def _set_and_clear(eng, s):
    eng.set_ingredients(*_ingredients(s.E, 2))
    eng.clear_ingredients()


STEP_INGREDIENTS = Step(name="set_ingredients + clear_ingredients", apply=_set_and_clear, after=lambda s: s)

Writer = types.SimpleNamespace
EVERY = ("plain", "mlp", "market", "plain200", "mlp200", "ing")
TRAINABLE = ("plain", "mlp", "market", "plain200", "mlp200")


def _writers():
    w = []
    add = lambda name, kinds, *steps: w.append(Writer(name=name, kinds=tuple(kinds), steps=list(steps)))
    add("write_memory-personal", EVERY, step_write(True, False))
    add("write_memory-both", EVERY, step_write(True, True))
    add("write_memory-general", EVERY, step_write(False, True))
    add("train_step-fused-sgd", TRAINABLE, step_train("sgd", 200.0, 256, kernel="m2d_train_grad_fused"))
    add("train_step-fused-adam", TRAINABLE, step_train("adam", 0.05, 256, kernel="m2d_train_grad_fused"))
    add("train_step-nine-launch-1100", TRAINABLE, step_train("adam", 0.05, 1100, kernel="m2d_train_grad"))
    add("train_step-nine-launch-variant14", TRAINABLE, step_train("adam", 0.05, 256, variant=14, kernel="m2d_train_grad"))
    add("train_step-unapplied", TRAINABLE, step_train("adam", 0.05, 256),                 # (so that the slots hold something)
        step_train("adam", 0.05, 256, seed=12, do_apply=False))
    for which in ("pm", "re", "ce", "all"):
        add("tables_updated-" + which, EVERY, step_edit(which))
    add("set_dish_categories", TRAINABLE, step_cats(4), step_cats(5, weighted=True), step_cats(6))
    add("set_mlp_head", ("mlp", "mlp200"), step_head(8))
    add("set_recipes", ("market",), STEP_RECIPES)
    add("set_user_base", EVERY, STEP_USER_BASE)
    add("ingredients-set-and-cleared", ("plain",), STEP_INGREDIENTS)
    add("back-to-back", ("plain", "mlp", "market"), both(step_write(True, True), step_train("adam", 0.05, 256)),
        step_train("adam", 0.05, 1100, seed=13), step_write(True, False, seed=6))
    return w


WRITERS = _writers()
WRITER_BY_NAME = {w.name: w for w in WRITERS}
assert len(WRITER_BY_NAME) == len(WRITERS)
WRITER_COVERS = ("write_memory", "train_step", "tables_updated", "set_dish_categories", "set_mlp_head", "set_recipes", "set_user_base",
                 "set_ingredients", "clear_ingredients")
PAIRS = [(kind, w.name) for kind in ENGINE_KINDS for w in WRITERS if kind in w.kinds]


@functools.lru_cache(maxsize=None)
def states(kind, writer):
    """[the state before the writer, the state after its first step, ...]"""
    out = [initial(kind)]
    for step in WRITER_BY_NAME[writer].steps:
        out.append(step.after(out[-1]))
    return out


@functools.lru_cache(maxsize=None)
def _model(kind, writer, n):
    """the restatement of states(kind, writer)[n]; a state that is the one before it shares its model (and its cached rows)"""
    if n == 0:
        return model_of(initial(kind))
    chain = states(kind, writer)
    return _model(kind, writer, n - 1) if chain[n] is chain[n - 1] else model_of(chain[n])


@functools.lru_cache(maxsize=None)
def restated(kind, writer, n, reader):
    """the reader's answer to its sample on states(kind, writer)[n]"""
    r = BY_NAME[reader]
    d = request(reader)
    idx = sample_rows(r, d)
    m = _model(kind, writer, n)
    return r.answer(m, asked(r, d if idx is None else subrequest(d, idx), m.cats))


def measure(r, what):
    """How a reader's change is counted: as its answer says (stream_cases.different), but compose_profiles by profile ROW -- a row
    that differs anywhere beyond TOL, as stream_cases counts the writers' table rows.  Its answer is rows of Personal_Memory blended
    with General_Memory: an element no pair of a batch addresses (a category the paired dish is not in) gets no gradient at any
    step size, so the share of ELEMENTS a one-pair-per-user batch moves is bounded by the masks, below one half."""
    return "rows" if r.name == "compose_profiles" else what


def threshold(what):
    return SCORES if what in ("scores", "rows") else LISTS_OR_RANKS


def label(what, share):
    """`expected`'s word for a share of change"""
    return "same" if share == 0.0 else "changed" if share > threshold(what) else "weak"


def expected(kind, writer, step, reader):
    """("changed" | "same" | "refuses" | "weak", the restated share of change) of `reader` after step `step` of `writer`"""
    r = BY_NAME[reader]
    chain = states(kind, writer)
    if refuses_weighted(r) and not binary(chain[step + 1].cats):
        return "refuses", None
    if refuses_weighted(r) and not binary(chain[step].cats):
        return "changed", 1.0                                # it refused before the step: any answer is a change
    a, b = restated(kind, writer, step, reader), restated(kind, writer, step + 1, reader)
    if a.value.shape == b.value.shape and np.array_equal(a.value, b.value):
        return "same", 0.0
    what = measure(r, a.what)
    share = st.different(what, a.value, b.value)
    return label(what, share), share


def judge(what, before, after, want):
    """The comparison the GPU file makes between a reader's two answers, on host values: None if (before, after) is what `want`
    says, else what is wrong.  The CPU file runs stand-in readers through it."""
    if want == "same":
        same = before.shape == after.shape and before.dtype == after.dtype and before.tobytes() == after.tobytes()
        return None if same else "must be bit-equal and is not"
    assert want == "changed"
    share = st.different(what, before, after)
    return None if share > threshold(what) else "changed in a share %.3f of its results only: a stale answer could pass" % share
