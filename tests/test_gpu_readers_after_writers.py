"""Readers after writers: every function that reads the tables returns FRESH results after every function that writes them.

The engine keeps derived state behind hand-set flags and generation counters -- the factored dish vectors (dish_vec_valid,
dish_vec_gen -> the MLP head's pattern bytes), the pattern-sorted dish rows (grp_valid, grp_gen -> catalogue_rank's tile norms,
grp_ew = E or 2 E), the <U_high, CE_c> table (user_high_valid), the "a table value is inf / NaN" word (finite_scan_pending,
grp_nonfinite_known), the lazily built images of the MLP head's weights and the scratch of its pattern-grouped launch.  The
flags are reset by hand in m2d_write_memory, in the two forms of the training step, in m2d_tables_updated and in the setters.
A reset that goes missing serves yesterday's lists without any error, so each test here follows one pattern:

    snapshot (every reader; this also warms every cache) -> one writer -> snapshot -> the same snapshot on a FRESH engine built
    from the written engine's own tables

and asserts that the second snapshot equals the fresh engine's bit for bit (the kernels are reproducible: same tables, same
launch shapes, same bits), that it passes the oracle on the written tables, and that the writer CHANGED the answer -- more than
a quarter of the lists, more than half of the scores -- so that a stale answer cannot pass.  Writers that must change nothing
(a `general`-only Write_Memory, train_step(apply=False), an optimizer slot saved and restored) leave the snapshot bit-equal.

This file holds the ten readers the engine had when it was written, each with the kernel it is there for.  THE FULL MATRIX -- every
reader call the engine has since gained (rank_candidates, the deep, MLP, group, profile, slate, market and menu calls) against every
writer -- lives in tests/writer_cases.py (the tables) and tests/test_gpu_readers_after_writers_all.py (the same pattern, one test per
engine kind and writer).  A NEW READER MUST JOIN IT: tests/test_writer_cases_cpu.py fails until every public method of ScoringEngine
is a reader row, a writer, or excused by name with a reason.
"""
import functools
import types

import numpy as np
import pytest

from helpers import TOL, assert_mlp_scores, assert_scores_close, mlp_case

pytestmark = pytest.mark.gpu

U, I, C, K = 300, 3000, 4, 10
NPAIRS = 4000
NBIG = 2 ** 18 + 77                  # user_high_table serves batches of >= 2^18 pairs


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _tables(E, seed=0):
    rng = np.random.default_rng(1000 + E + seed)
    s = 1.0 / np.sqrt(E)
    return tuple((rng.standard_normal(shape) * s).astype(np.float32) for shape in ((U, C + 1, E), (I, E), (C, E)))


def _masks(seed, weighted=False):
    rng = np.random.default_rng(seed)
    cats = ((rng.integers(1, 2 ** C, I)[:, None] >> np.arange(C)[None, :]) & 1).astype(np.float32)
    if weighted:
        cats = (cats * rng.uniform(0.5, 2.0, (I, C))).astype(np.float32)
    return cats


def _head(E, seed, H1=256, H2=64, scale=4.0):
    rng = np.random.default_rng(seed)
    Kd = (C + 1) * E
    return ((rng.standard_normal((Kd, H1)) * scale / np.sqrt(Kd)).astype(np.float32), (rng.standard_normal(H1) * 0.1).astype(np.float32),
            (rng.standard_normal((H1, H2)) * scale / np.sqrt(H1)).astype(np.float32), (rng.standard_normal(H2) * 0.1).astype(np.float32),
            (rng.standard_normal(H2) * scale / np.sqrt(H2)).astype(np.float32), 0.25)


def _ingredients(E, seed, R=200):
    rng = np.random.default_rng(seed)
    ING = (rng.standard_normal((R, E)) / np.sqrt(E)).astype(np.float32)
    off = np.zeros(I + 1, np.int32)
    off[1:] = np.cumsum(rng.integers(1, 9, I))
    ids = rng.integers(0, R, off[-1]).astype(np.int32)
    return ING, off, ids, rng.uniform(0.5, 2.0, len(ids)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs():
    """What the readers are asked, the same in every snapshot (user ids before the engine's user_base is added)."""
    from foodrec_amd.ops import exclusion_csr
    rng = np.random.default_rng(7)
    csr = lambda lists: exclusion_csr(lists, U)              # (offsets, ids ascending within a user): sorted once, not per snapshot
    return types.SimpleNamespace(
        users=rng.integers(0, U, NPAIRS).astype(np.int32), items=rng.integers(0, I, NPAIRS).astype(np.int32),
        big_users=rng.integers(0, U, NBIG).astype(np.int32), big_items=rng.integers(0, I, NBIG).astype(np.int32),
        held=rng.integers(0, I, U).astype(np.int32),
        excl_some=csr([rng.choice(I, 20, replace=False).tolist() for _ in range(U)]),
        # nine dishes in ten excluded: no user's unfiltered top 16 holds k = 10 of the rest -- every user is "short"
        excl_most=csr([rng.choice(I, 2700, replace=False).tolist() for _ in range(U)]),
        excl_none=csr([[] for _ in range(U)]))                 # ... and with nothing excluded none is


def _cfg(E, cats=None, head=None, ing=None, user_base=0, mlp_x3=1):
    """A configuration with a head runs at blend 0.5: at the default 0.99 the low-level blocks of z carry weight 0.01 and the
    oracle check of the grouped MLP reader could not see a stale pattern byte (helpers.assert_mlp_scores refuses such inputs)."""
    return types.SimpleNamespace(E=E, cats=_masks(3) if cats is None else cats, head=head, ing=ing, user_base=user_base, mlp_x3=mlp_x3,
                                 coef=0.99 if head is None else 0.5)


def _engine(tabs, cfg):
    from foodrec_amd import ScoringEngine
    eng = ScoringEngine(*tabs, coef=cfg.coef, user_base=cfg.user_base)
    eng.set_dish_categories(cfg.cats)
    if cfg.head is not None:
        eng.set_mlp_head(*cfg.head)
    if cfg.ing is not None:
        eng.set_ingredients(*cfg.ing)
    return eng


def _binary(cats):
    return bool(np.all((cats == 0) | (cats == 1)))


# ---- the readers ----------------------------------------------------------------------------------------------------------
def _snapshot(eng, cfg):
    """Every reader this configuration has, by name -> tuple of host arrays (None: the reader refused, as it must for these
    masks).  Asserts the kernel each reader is there for."""
    import torch
    inp = _inputs()
    t = lambda a: torch.as_tensor(a, device="cuda")
    E, binary = cfg.E, _binary(cfg.cats)
    all_users = t(np.arange(U, dtype=np.int32) + cfg.user_base)
    users, items = t(inp.users + cfg.user_base), t(inp.items)
    cats_dev = t(cfg.cats)
    out = {}

    def run(name, fn, kernel=None, refuses=False):
        if refuses:
            with pytest.raises(ValueError):
                fn()
            out[name] = None
            return
        res = fn()
        eng.check()
        if kernel is not None:
            assert eng.last_kernel() in ((kernel,) if isinstance(kernel, str) else kernel), (name, eng.last_kernel())
        out[name] = tuple(x.cpu().numpy() for x in (res if isinstance(res, tuple) else (res,)))

    dense = "m2d_topk_mfma" if E in (32, 64, 128) else ("m2d_topk_mfma", "m2d_topk_generic")     # both read dish_vec
    grouped = "m2d_topk_grouped_bf16x3" if E in (64, 128) else "m2d_topk_grouped"
    topk = lambda: eng.topk_users(all_users, K)
    if cfg.ing is not None:
        run("ingredient_pairs", lambda: eng.score_pairs_ingredients(users, items))
        run("topk", topk, "m2d_topk_grouped_bf16x3" if binary else dense)                         # rows [H[d] | RE[d]]: grp_ew = 2 E
        eng.set_option("topk_grouped", 0)
        run("topk_dense", topk, dense)
        eng.set_option("topk_grouped", 1)
        return out
    run("topk", topk, grouped if binary else dense)
    run("pairs", lambda: eng.score_pairs(users, items, cats_dev[items.long()]))
    assert eng.last_kernel().startswith("m2d_score_pairs_c4")
    if cfg.head is not None:                                 # (catalogue_rank / topk_users_excluding refuse a model with a head)
        eng.set_option("mlp_bf16x3", cfg.mlp_x3)
        for form in (0, 1):
            eng.set_option("mlp_form", form)
            if not cfg.mlp_x3:
                want = "m2d_mlp_mfma"
            else:
                want = "m2d_mlp_pc_bf16x3" if form == 0 and E in (64, 128) else "m2d_mlp_mfma_bf16x3"
            run("mlp_form%d" % form, lambda: eng.score_pairs_mlp(users, items), want)
        eng.set_option("mlp_form", 0)
        if cfg.mlp_x3 and E in (64, 128):                    # NBIG >= 16 384 pairs: bucketed by mask pattern -- mlp_pat8, the mlp_pg scratch
            run("mlp_big", lambda: eng.score_pairs_mlp(t(inp.big_users + cfg.user_base), t(inp.big_items)), "m2d_mlp_pc_bf16x3")
        return out
    eng.set_option("topk_bf16x3", 0)
    run("topk_f32", topk, "m2d_topk_grouped" if binary else dense)
    eng.set_option("topk_bf16x3", 1)
    eng.set_option("variant", 7)
    run("topk_dense", topk, dense)                           # reads dish_vec
    eng.set_option("variant", 0)
    run("rank", lambda: eng.catalogue_rank(all_users, t(inp.held), inp.excl_some), "m2d_rank_count", refuses=not binary)
    for name, excl, short in (("excl_most", inp.excl_most, U), ("excl_none", inp.excl_none, 0)):
        run(name, lambda: eng.topk_users_excluding(all_users, K, (t(excl[0]), t(excl[1]))), "m2d_topk_excl_scan", refuses=not binary)
        if binary and E in (32, 64, 128):                    # (other sizes have no filtered tier: every user is scanned)
            assert eng.get_option("topk_excl_short") == short, (name, eng.get_option("topk_excl_short"))
    eng.set_option("topk_excl_tier", 2)
    run("excl_tier2", lambda: eng.topk_users_excluding(all_users, K, (t(inp.excl_some[0]), t(inp.excl_some[1]))), "m2d_topk_excl_scan",
        refuses=not binary)
    if binary:
        assert eng.get_option("topk_excl_short") == U
    eng.set_option("topk_excl_tier", 0)
    run("bydish", lambda: eng.score_pairs_bydish(users, items))
    eng.set_option("user_high_table", 1)
    big_items = t(inp.big_items)
    run("pairs_uh", lambda: eng.score_pairs(t(inp.big_users + cfg.user_base), big_items, cats_dev[big_items.long()]), "m2d_score_pairs_c4_uh")
    eng.set_option("user_high_table", 0)
    return out


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert (a[name] is None) == (b[name] is None), (what, name)
        for x, y in zip(a[name] or (), b[name] or ()):
            assert x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), \
                "%s: %s differs at %d of %d" % (what, name, int((_bits(x) != _bits(y)).sum()), x.size)


def _changed_fraction(name, a, b):
    if name == "rank":
        return float(np.mean(a[0] != b[0]))
    if name.startswith(("topk", "excl")):
        return float(np.mean(np.any(a[1] != b[1], axis=1)))
    x, y = a[0].astype(np.float64), b[0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.mean(np.abs(x - y) > TOL * np.maximum(1.0, np.abs(y))))


def _assert_changed(a, b, what, only=None):
    """The writer changed the answer: more than a quarter of the lists (ranks), more than half of the scores beyond the
    tolerance.  `only`: the readers this writer reaches; the others must be bit-equal."""
    for name in a:
        if a[name] is None or b[name] is None:
            continue
        if only is not None and not name.startswith(only):
            _assert_same({name: a[name]}, {name: b[name]}, what + " (untouched reader)")
            continue
        f = _changed_fraction(name, a[name], b[name])
        assert f > (0.5 if name.startswith(("pairs", "bydish", "mlp", "ingredient")) else 0.25), \
            "%s: %s changed in a fraction %.3f of its results only -- the test could pass on stale state" % (what, name, f)


def _host_tables(eng):
    return tuple(x.cpu().numpy().copy() for x in (eng.pm, eng.re, eng.ce))


def _assert_oracle(eng, snap, cfg):
    """The snapshot against the float64 restatement on the engine's tables as they stand: lists of a sample of users, pair scores."""
    from oracle import m2d_oracle as oracle
    from test_gpu_catalogue import _check
    inp = _inputs()
    PM, RE, CE = _host_tables(eng)
    if cfg.ing is not None:
        ref = oracle.inference_ingredients(PM, RE, *cfg.ing, inp.users, inp.items, cfg.cats[inp.items])
        assert_scores_close(snap["ingredient_pairs"][0], ref, what="ingredient pairs")
        return
    _check(eng, PM, RE, CE, cfg.cats, np.arange(0, U, 37), K, user_base=cfg.user_base)
    ref = oracle.inference_f64(PM, RE, CE, inp.users, inp.items, cfg.cats[inp.items], cfg.coef)
    assert_scores_close(snap["pairs"][0], ref, what="pairs")
    if "bydish" in snap:
        assert_scores_close(snap["bydish"][0], ref, what="bydish")
    if cfg.head is not None:
        ref = oracle.inference_mlp(PM, RE, CE, cfg.cats, *cfg.head, inp.users, inp.items, coef=cfg.coef)
        for form in (0, 1):
            assert_scores_close(snap["mlp_form%d" % form][0], ref, what="mlp form %d" % form)
        if "mlp_big" in snap:                                # a sample, and the condition that a lost k-period would show in it
            case = mlp_case(PM, RE, CE, cfg.cats, cfg.head, inp.big_users, inp.big_items, cfg.coef)
            assert_mlp_scores(snap["mlp_big"][0], case, np.arange(0, NBIG, 64), what="mlp, grouped launch")


def _after(eng, cfg, before, what, expect="changed", only=None):
    """The second snapshot, the fresh engine's, and the assertions every test makes.  Returns the second snapshot."""
    snap = _snapshot(eng, cfg)
    fresh = _engine(_host_tables(eng), cfg)
    _assert_same(snap, _snapshot(fresh, cfg), what + ": written engine vs fresh engine")
    fresh.close()
    if expect == "same":
        _assert_same(before, snap, what + ": must change nothing")
    else:
        _assert_changed(before, snap, what, only)
    _assert_oracle(eng, snap, cfg)
    return snap


# ---- writers ---------------------------------------------------------------------------------------------------------------
def _write_batch(cfg, B=600, L=7, seed=5):
    import torch
    rng = np.random.default_rng(seed)
    t = lambda a: torch.as_tensor(a, device="cuda")
    users = (np.arange(B) % U).astype(np.int32)             # every user is written to
    items = rng.integers(0, I, B).astype(np.int32)
    y = (rng.random((B, L)) < 0.3).astype(np.float32); y[:, 0] = 1
    sign = np.where(rng.random(B) < 0.5, 1.0, -1.0).astype(np.float32)
    gm = t((rng.standard_normal((L, C + 1, cfg.E)) / 4).astype(np.float32))
    return (t(users + cfg.user_base), t(items), t(cfg.cats[items]), t(sign), t(y), gm, 1.0, 1.0, 0.5)


def _train_batch(cfg, B, seed=11):
    import torch
    rng = np.random.default_rng(seed)
    t = lambda a: torch.as_tensor(a, device="cuda")
    users = (rng.permutation(max(B, U))[:B] % U).astype(np.int32)
    items = rng.integers(0, I, B).astype(np.int32)
    return t(users + cfg.user_base), t(items), t(cfg.cats[items]), t(rng.integers(0, 2, B).astype(np.float32))


def _kinds(E):
    """The three reader sets: the plain engine, the engine with an MLP head, the engine with an ingredient table."""
    return {"plain": _cfg(E), "mlp": _cfg(E, head=_head(E, 1)), "ingredients": _cfg(E, ing=_ingredients(E, 2))}


@pytest.mark.parametrize("kind", ["plain", "mlp", "ingredients"])
@pytest.mark.parametrize("write_pm,write_gm", [(True, False), (True, True), (False, True)], ids=["personal", "both", "general"])
def test_after_write_memory(kind, write_pm, write_gm):
    """m2d_write_memory resets user_high_valid and grp_nonfinite_known when it writes Personal_Memory; a `general`-only call
    writes no table the readers see."""
    cfg = _kinds(64)[kind]
    eng = _engine(_tables(64), cfg)
    before = _snapshot(eng, cfg)
    eng.write_memory(*_write_batch(cfg), write_pm=write_pm, write_gm=write_gm); eng.check()
    _after(eng, cfg, before, "write_memory", "changed" if write_pm else "same")


TRAIN = [pytest.param("sgd", 200.0, 256, 0, "m2d_train_grad_fused", id="fused-sgd"),
         pytest.param("adam", 0.05, 256, 0, "m2d_train_grad_fused", id="fused-adam"),
         pytest.param("adam", 0.05, 256, 14, "m2d_train_grad", id="nine-launch-variant14"),
         pytest.param("adam", 0.05, 1100, 0, "m2d_train_grad", id="nine-launch-1100")]


@pytest.mark.parametrize("kind,E", [("plain", 64), ("mlp", 64), ("plain", 128), ("plain", 200), ("mlp", 200)])
@pytest.mark.parametrize("learner,lr,B,variant,kernel", TRAIN)
def test_after_train_step(kind, E, learner, lr, B, variant, kernel):
    """Both forms of the step end by resetting dish_vec_valid, user_high_valid and grp_valid (all three tables moved)."""
    cfg = _kinds(E)[kind]
    eng = _engine(_tables(E), cfg)
    before = _snapshot(eng, cfg)
    eng.train_begin(learner, lr)
    eng.set_option("variant", variant)
    out = eng.train_step(*_train_batch(cfg, B)); eng.check()
    assert eng.last_kernel() == kernel and np.isfinite(out.cpu().numpy()).all()
    eng.set_option("variant", 0)
    _after(eng, cfg, before, "train_step %s" % learner)
    eng.train_end()


@pytest.mark.parametrize("kind", ["plain", "mlp"])
def test_after_writers_that_change_nothing(kind):
    """train_step(apply=False) computes the loss and the norm only; an optimizer slot read out and written back is the same slot."""
    cfg = _kinds(64)[kind]
    eng = _engine(_tables(64), cfg)
    eng.train_begin("adam", 0.05)
    eng.train_step(*_train_batch(cfg, 256)); eng.check()    # so that the slots hold something
    before = _snapshot(eng, cfg)
    tabs = _host_tables(eng)
    eng.train_step(*_train_batch(cfg, 256, seed=12), apply=False); eng.check()
    for tb in range(3):
        for sl in range(2):
            eng.train_slot(tb, sl, restore=eng.train_slot(tb, sl).clone())
    eng.check()
    assert all(np.array_equal(a, b) for a, b in zip(tabs, _host_tables(eng)))
    _after(eng, cfg, before, "apply=False / slot round trip", "same")
    eng.train_end()


@pytest.mark.parametrize("kind,E", [("plain", 64), ("mlp", 64), ("ingredients", 64), ("plain", 128), ("plain", 200), ("mlp", 200)])
def test_after_tables_updated(kind, E):
    """In-place edits of the borrowed tables, then tables_updated(): one Recipe_Embedding row (the sorted dish rows and the dish
    vectors hold a copy of it), the whole Category_Embedding and every user's high-level row."""
    import torch
    cfg = _kinds(E)[kind]
    eng = _engine(_tables(E), cfg)
    before = _snapshot(eng, cfg)
    eng.re[7] *= 1000.0                                      # dish 7 now leads the list of every user its low-level score favours
    eng.ce.copy_(torch.flip(eng.ce, dims=(0, 1)) * 1.5)
    eng.pm[:, 0].mul_(-1.5)                                  # U_high: what the <U_high, CE_c> table is built from
    eng.tables_updated()
    snap = _after(eng, cfg, before, "tables_updated")
    held = lambda s: float(np.mean(np.any(s["topk"][1] == 7, axis=1)))
    assert held(before) < 0.05 and held(snap) > 0.25         # the edited ROW is read, not only the edited Category_Embedding


def test_after_set_dish_categories():
    """Another 0/1 table, then a weighted one -- the pattern-grouped readers give way to the dense kernel, catalogue_rank and
    topk_users_excluding refuse -- then a 0/1 table again."""
    cfg = _cfg(64)
    eng = _engine(_tables(64), cfg)
    snap = _snapshot(eng, cfg)
    for step, cats in (("0/1", _masks(4)), ("weighted", _masks(5, weighted=True)), ("0/1 again", _masks(6))):
        cfg = _cfg(64, cats=cats)
        eng.set_dish_categories(cats)
        snap = _after(eng, cfg, snap, "set_dish_categories " + step)
        assert (snap["rank"] is None) == (step == "weighted") and (snap["excl_most"] is None) == (step == "weighted")


def test_after_set_dish_categories_with_an_mlp_head():
    """The head's pattern bytes (mlp_pat8) belong to one build of the dish vectors (dish_vec_gen)."""
    cfg = _cfg(64, head=_head(64, 1))
    eng = _engine(_tables(64), cfg)
    snap = _snapshot(eng, cfg)
    for step, cats in (("0/1", _masks(4)), ("weighted", _masks(5, weighted=True)), ("0/1 again", _masks(6))):
        cfg = _cfg(64, cats=cats, head=cfg.head)
        eng.set_dish_categories(cats)
        snap = _after(eng, cfg, snap, "set_dish_categories (mlp) " + step)


def test_after_set_and_clear_ingredients():
    """set -> clear -> set with another table: the sorted dish rows go from [H[d] | RE[d]] (grp_ew = 2 E) to RE[d] (E) and back."""
    ing_a, ing_b = _ingredients(64, 2), _ingredients(64, 9)
    cfg = _cfg(64, ing=ing_a)
    eng = _engine(_tables(64), cfg)
    with_a = _snapshot(eng, cfg)
    eng.clear_ingredients()
    plain = _cfg(64)
    cleared = _snapshot(eng, plain)
    fresh = _engine(_host_tables(eng), plain)
    _assert_same(cleared, _snapshot(fresh, plain), "clear_ingredients: written engine vs fresh engine")
    fresh.close()
    _assert_oracle(eng, cleared, plain)
    assert _changed_fraction("topk", with_a["topk"], cleared["topk"]) > 0.25
    cfg = _cfg(64, ing=ing_b)
    eng.set_ingredients(*ing_b)
    _after(eng, cfg, with_a, "set_ingredients (another table)")


@pytest.mark.parametrize("E,mlp_x3", [(64, 1), (64, 0), (200, 1), (200, 0)])
def test_after_set_mlp_head_again(E, mlp_x3):
    """The head's weight images (split-bf16 W1, zero-padded W1 for K = 1000, the producer / consumer image) are built lazily,
    once per head: a second head must not be served from the first one's."""
    cfg = _cfg(E, head=_head(E, 1), mlp_x3=mlp_x3)
    eng = _engine(_tables(E), cfg)
    before = _snapshot(eng, cfg)
    cfg = _cfg(E, head=_head(E, 8), mlp_x3=mlp_x3)
    eng.set_mlp_head(*cfg.head)
    _after(eng, cfg, before, "set_mlp_head", only="mlp")


def test_after_set_user_base():
    """The same rows under other ids: nothing a reader returns may change, ids outside the new range are refused."""
    import torch
    cfg = _cfg(64)
    eng = _engine(_tables(64), cfg)
    before = _snapshot(eng, cfg)
    cfg = _cfg(64, user_base=7000)
    eng.set_user_base(7000)
    _after(eng, cfg, before, "set_user_base", "same")
    eng.topk_users(torch.arange(3, dtype=torch.int32, device="cuda"), K)
    with pytest.raises(IndexError, match="user id [012] at position [012] "):
        eng.check()


def test_two_writers_back_to_back_then_writer_reader_writer_reader():
    """Write_Memory and a training step with no reader in between (the second writer must not mark as valid what the first one
    invalidated), then the alternation."""
    cfg = _cfg(64)
    eng = _engine(_tables(64), cfg)
    before = _snapshot(eng, cfg)
    eng.train_begin("adam", 0.05)
    eng.write_memory(*_write_batch(cfg), write_pm=True, write_gm=True)
    eng.train_step(*_train_batch(cfg, 256)); eng.check()
    snap = _after(eng, cfg, before, "write_memory + train_step")
    eng.train_step(*_train_batch(cfg, 1100, seed=13)); eng.check()
    snap = _after(eng, cfg, snap, "... + train_step (nine launches)")
    eng.write_memory(*_write_batch(cfg, seed=6), write_pm=True, write_gm=False); eng.check()
    _after(eng, cfg, snap, "... + write_memory")
    eng.train_end()


def test_model_serves_fresh_lists_after_the_training_fetches(tmp_path):
    """Session.run of the driver's training fetches, then Model.topk(exclude=...) and evaluate_model_full: the same answers as a
    fresh Model restored from this one's checkpoint, and the earlier checkpoint brings the earlier answers back."""
    from foodrec_amd import Model, Session
    from foodrec_amd.evaluator import evaluate_model_full
    E, L, B = 64, 7, 256
    PM, RE, CE = _tables(E)
    cats = _masks(3)
    rng = np.random.default_rng(17)
    GM = (rng.standard_normal((L, C + 1, E)) / 8).astype(np.float32)
    args = types.SimpleNamespace(learner="adam", num_categories=C, num_users=U, num_labels=L, embed_size=E, lr=0.05, decay_steps=1000,
                                 decay_rate=1.0, high_level_score_coefficient=0.99, beta_1=1.0, beta_2=1.0, alpha=0.5)
    d2c = {str(d): cats[d][:, None].tolist() for d in range(I)}
    users = list(range(U))
    train = {u: rng.choice(I, 30, replace=False).tolist() for u in users}
    test = {u: [int(rng.integers(0, I))] for u in users}

    def answers(model):
        model.set_dish_categories(d2c)
        s, i = model.topk(users, K, exclude=train)
        hits, ndcgs = evaluate_model_full(None, model, test, train, K, d2c)
        return s, i, np.asarray(hits), np.asarray(ndcgs)

    def same(a, b):
        return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))

    model = Model(args, PM.copy(), RE.copy(), CE.copy(), GM.copy())
    sess = Session(model)
    first = answers(model)
    model.save(str(tmp_path / "before.npz"))
    bu = rng.permutation(U)[:B]
    bi = rng.integers(0, I, B)
    labels = rng.integers(0, 2, B).astype(np.float32)
    onehot = (rng.random((B, L)) < 0.3).astype(np.float32); onehot[:, 0] = 1
    feed = {model.user_input: [str(u) for u in bu], model.item_input: list(bi), model.labels: list(labels),
            model.categories: cats[bi][:, :, None].tolist(), model.user_one_hot_label: onehot.tolist(),
            model.write_sign: np.where(labels > 0, 1.0, -1.0)[:, None].tolist(), model.dropout_keep_prob: 0.8,
            model.is_training_flag: True}
    sess.run([model.loss_value, model.learning_rate, model.general, model.train_op], feed)
    sess.run([model.loss_value, model.learning_rate, model.personal, model.general, model.train_op], feed)
    second = answers(model)
    assert np.mean(np.any(first[1] != second[1], axis=1)) > 0.25             # training changed the lists
    model.save(str(tmp_path / "after.npz"))
    fresh = Model(args, np.zeros_like(PM), np.zeros_like(RE), np.zeros_like(CE), GM.copy())
    fresh.restore(str(tmp_path / "after.npz"))
    assert same(second, answers(fresh))
    model.restore(str(tmp_path / "before.npz"))
    assert same(first, answers(model))
