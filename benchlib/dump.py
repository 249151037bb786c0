"""--dump-outputs DIR: what the timed path computed in its last step, as .npy files, so that two builds can be compared
output for output on the same seeded inputs."""
from __future__ import annotations

import os

import numpy as np

BUDGET_BYTES = 64 << 20
SAMPLE_SEED = 20260101


def write_outputs(out_dir, arrays, budget=BUDGET_BYTES):
    """`arrays`: name -> tensor, rows along dim 0.  Floating tensors are written as float32, integer ones (dish ids) as
    float64, which holds them exactly.  Arrays with the same number of rows form a group, and the groups share `budget`
    bytes: a group within its share is written whole, and a larger one keeps a fixed, seeded, sorted sample of rows --
    the same rows for each of its arrays -- with `<name>_rows.npy` (float64) naming them.
    Returns {name: rows written}."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    conv = {k: (v.detach(), 4 if v.is_floating_point() else 8) for k, v in arrays.items()}
    groups = {}
    for k, (t, eb) in conv.items():
        groups.setdefault(t.shape[0], []).append((k, (t[0].numel() if t.dim() > 1 else 1) * eb))
    left, written = budget, {}
    order = sorted(groups, key=lambda n: n * sum(rb for _, rb in groups[n]))
    for i, n in enumerate(order):
        share = left / (len(order) - i)
        rows = None
        if n * sum(rb for _, rb in groups[n]) > share:   # every kept row costs its data and one float64 index per array
            m = max(1, int(share // sum(rb + 8 for _, rb in groups[n])))
            rows = np.sort(np.random.default_rng(SAMPLE_SEED).choice(n, m, replace=False))
        for k, _ in groups[n]:
            t, eb = conv[k]
            if rows is not None:
                t = t.index_select(0, torch.as_tensor(rows, device=t.device))
                np.save(os.path.join(out_dir, k + "_rows.npy"), rows.astype(np.float64))
            a = t.cpu().numpy().astype(np.float32 if eb == 4 else np.float64)
            np.save(os.path.join(out_dir, k + ".npy"), a)
            left -= a.nbytes + (rows.nbytes if rows is not None else 0)
            written[k] = int(a.shape[0])
    return written
