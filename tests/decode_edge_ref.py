"""CPU references of the decode edge cases (tests/decode_edge_synth.py), computed once per process and shared by
tests/test_decode_edges_host.py and tests/test_gpu_decode_edges.py.

``oracle.lore_decode.topk_1class`` is ``torch.topk``, whose order among equal scores is arbitrary; the kernels' contract is (score desc,
pixel index asc).  ``lexsort_topk_1class`` states that contract with the oracle's signature and replaces ``topk_1class`` in the tie cases
only; the re-sort after the snap (``torch.sort``, as arbitrary among equal scores) is made stable there, which is the kernels' (new score
desc, previous rank asc).  test_decode_edges_host.py proves that neither replacement changes anything on tie-free maps."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import centernet_ref as R  # noqa: E402
import decode_edge_synth as S  # noqa: E402
from oracle import lore_decode as od  # noqa: E402


def lexsort_topk_1class(scores: torch.Tensor, K: int):
    """topk_1class with ties broken by ascending pixel index: (score [1,K], ind [1,K] int64, ys [1,K], xs [1,K])"""
    b, c, H, W = scores.shape
    assert b == 1 and c == 1 and H * W >= K
    s = scores.reshape(-1).numpy()
    order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))[:K]
    ind = torch.from_numpy(order.astype(np.int64)).view(1, 1, -1)
    ys = (ind / torch.tensor([float(W)])).int().float()
    xs = (ind % W).int().float()
    return torch.from_numpy(s[order].copy()).view(1, -1), ind.view(1, -1), ys.view(1, -1), xs.view(1, -1)


_torch_sort = torch.sort


def _stable_sort(*a, **k):
    """the oracle re-sorts the cells by their scores after the snap with torch.sort, which keeps no order among equal scores either;
    the kernels' contract there is (new score desc, previous rank asc), i.e. the stable sort"""
    k["stable"] = True
    return _torch_sort(*a, **k)


def lore_reference(heads, rev, ties=False):
    """-> dict(n, raw [K,10], logi [n,256], snap: the arguments of the oracle's snap_vertices call or None)"""
    t = {k: torch.from_numpy(v.copy()) for k, v in heads.items()}
    H, W = heads["hm"].shape[2:]
    _, meta = od.lore_preprocess_geometry(4 * H, 4 * W, 4 * H, 4 * W)
    seen = {}
    real_snap = od.snap_vertices

    def spy(*a):
        seen["snap"] = a
        return real_snap(*a)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(od, "snap_vertices", spy)
        if ties:
            mp.setattr(od, "topk_1class", lexsort_topk_1class)
            mp.setattr(torch, "sort", _stable_sort)
        logi, ps, polys, results, raw = od.process_detect_output(t, meta, wiz_rev=rev, vis_thresh=0.2, return_raw=True)
    return {"n": int(logi.shape[1]), "raw": raw, "logi": logi[0].numpy(), "snap": seen.get("snap")}


def cn_reference(case):
    heads, (cw, ch) = case
    return R.centernet_cells(heads, cw, ch)


# name -> (generator call, wiz_rev, ties)
LORE_CASES = {
    "ties": (lambda: S.lore_ties(), False, True),
    "ties_rev": (lambda: S.lore_ties(), True, True),
    "cap_cells": (lambda: S.lore_cap_cells(), False, False),
    "cap_cells_rev": (lambda: S.lore_cap_cells(), True, False),
    "cap_corners": (lambda: S.lore_cap_corners(), True, False),
    "overflow_cells": (lambda: S.lore_overflow(corner_class=False), False, True),
    "overflow_corners": (lambda: S.lore_overflow(corner_class=True), True, True),
    "rim": (lambda: S.lore_rim(), False, False),
    "rim_rev": (lambda: S.lore_rim(), True, False),
    "outside": (lambda: S.lore_outside(), False, False),
    "outside_rev": (lambda: S.lore_outside(), True, False),
    "rounds": (lambda: S.lore_rounds(), True, False),
}
CN_CASES = {
    "ties": lambda: S.cn_ties(),
    "cap_verts": lambda: S.cn_cap_verts(),
    "overflow": lambda: S.cn_overflow(),
    "rim": lambda: S.cn_rim(),
    "rounds": lambda: S.cn_rounds(exact_two=cn_identity()),
}


def cn_identity() -> bool:
    """does a crop of the map's own size make centernet_decode_affine the exact identity?"""
    from pdf_table_amd.centernet_stage import centernet_decode_affine
    n = S.CN_ROUNDS_SIZE
    return bool(np.array_equal(centernet_decode_affine(n, n, n, n), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])))


@functools.lru_cache(maxsize=None)
def lore_case(name):
    """-> (heads, facts, wiz_rev, reference); treat as read-only"""
    gen, rev, ties = LORE_CASES[name]
    heads, facts = gen()
    return heads, facts, rev, lore_reference(heads, rev, ties)


@functools.lru_cache(maxsize=None)
def cn_case(name):
    """-> ((heads, (crop w, crop h)), facts, reference cells [n, 9]); treat as read-only"""
    case, facts = CN_CASES[name]()
    return case, facts, cn_reference(case)


@functools.lru_cache(maxsize=None)
def lore_seam_case():
    tables, facts = S.lore_seams()
    return tables, facts, [lore_reference(h, True) for h in tables]


@functools.lru_cache(maxsize=None)
def cn_seam_case():
    cases, facts = S.cn_seams()
    return cases, facts, [cn_reference(c) for c in cases]
