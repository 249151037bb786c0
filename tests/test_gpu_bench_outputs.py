"""bench.py's plain run on hardware: it times exactly --steps steps, runs none of the --full legs, and --dump-outputs writes
what the last timed step computed -- the same files from run to run, and scores the CPU restatement agrees with."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_scores_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I, B = 20000, 5000, 65536
FULL_ONLY = ("cpu_baseline", "scaling_path", "catalogue_topk", "evaluator", "config2_mlp", "config4_topk",
             "with_ingredient_table", "with_user_high_table", "cfg1_ingredients_pairs_per_s", "stream_probe_GBps")


def _run(tmp_path, tag, *extra):
    out, dump = str(tmp_path / (tag + ".json")), str(tmp_path / tag)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--users", str(U),
           "--dishes", str(I), "--settle-ms", "0", "--dump-outputs", dump, "--out", out] + list(extra)
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.load(open(out)), dump


def test_plain_run_dumps_the_timed_scores(tmp_path):
    import torch
    from benchlib.common import make_inputs
    from oracle import m2d_oracle as oracle
    line, d1 = _run(tmp_path, "a", "--pairs", str(B))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert not [k for k in FULL_ONLY if k in line] and "survey_8d_frac" not in line["roofline"]
    got = np.load(os.path.join(d1, "scores.npy"))
    assert got.dtype == np.float32 and got.shape == (B,)
    # the inputs are seeded: the same command writes the same scores
    _, d2 = _run(tmp_path, "b", "--pairs", str(B))
    assert np.array_equal(np.load(os.path.join(d2, "scores.npy")), got)
    # ... and they are the scores of bench.py's inputs (the seed make_inputs is given at rank 0)
    PM, RE, CE, users, items, cats = (t.cpu().numpy() for t in make_inputs(torch, torch.device("cuda", 0), U, I, 4, 64, B,
                                                                          20260101 + 2, 0))
    assert_scores_close(got, oracle.inference_f64(PM, RE, CE, users, items, cats), what="bench --dump-outputs")


def test_plain_topk_run_dumps_the_lists(tmp_path):
    line, d = _run(tmp_path, "t", "--workload", "topk", "--topk-users", "512")
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    s, ids = np.load(os.path.join(d, "topk_scores.npy")), np.load(os.path.join(d, "topk_dish_ids.npy"))
    assert s.dtype == np.float32 and ids.dtype == np.float64 and s.shape == ids.shape == (512, 10)
    assert np.all((ids >= 0) & (ids < I)) and np.all(np.diff(s, axis=1) <= 0)
