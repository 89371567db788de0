"""Seeded (prediction, truth) table pairs for the WTW cell metric's tests and tools/cell_metric_bench.py: ruled grids of 40 x 20 pixel cells with logical
axes [col, col, row, row], the prediction a jittered, thinned, partly mislabelled and reshuffled copy of the truth.  Data only; nothing here is the
metric."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

Table = Tuple[np.ndarray, np.ndarray]


def grid_cells(n: int) -> Table:
    """n cells of a grid about 1.3 times as wide as high, row-major: (boxes float64 [n, 8], axes int64 [n, 4])"""
    cols = max(1, int(math.ceil(math.sqrt(n * 1.3))))
    k = np.arange(n)
    r, c = k // cols, k % cols
    x1, y1 = c * 40.0 + 3.0, r * 20.0 + 5.0
    x3, y3 = x1 + 40.0, y1 + 20.0
    boxes = np.stack([x1, y1, x3, y1, x3, y3, x1, y3], 1).astype(np.float64).reshape(n, 8)
    axes = np.stack([c, c, r, r], 1).astype(np.int64).reshape(n, 4)
    return boxes, axes


def sized_pair(seed: int, n_pred: int, n_gt: int, jitter: float = 4.0, wrong: float = 0.1) -> Tuple[Table, Table]:
    """a pair with exactly n_pred and n_gt cells, both drawn (in shuffled order) from one grid of max(n_pred, n_gt) cells; the prediction's corners
    are moved by up to `jitter` pixels and a share `wrong` of its cells has one axis off by one"""
    rng = np.random.default_rng(seed)
    boxes, axes = grid_cells(max(n_pred, n_gt, 1))
    gi, pi = rng.permutation(len(boxes))[:n_gt], rng.permutation(len(boxes))[:n_pred]
    pb = boxes[pi] + rng.uniform(-jitter, jitter, (n_pred, 8))
    pa = axes[pi].copy()
    bad = np.nonzero(rng.random(n_pred) < wrong)[0]
    pa[bad, rng.integers(0, 4, len(bad))] += 1
    return (pb, pa), (boxes[gi].copy(), axes[gi].copy())


def table_pair(seed: int, n: int, jitter: float = 4.0, drop: float = 0.1, wrong: float = 0.05) -> Tuple[Table, Table]:
    """a truth table of n cells and its prediction: about a share `drop` of the cells missing, the rest as in sized_pair"""
    rng = np.random.default_rng(seed)
    keep = max(1, int(round(n * (1.0 - drop * rng.uniform(0.5, 1.5)))))
    return sized_pair(seed + 1000003, min(keep, n), n, jitter, wrong)
