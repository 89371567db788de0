"""The WTW cell metric: cell detection precision / recall / F1 at an IoU threshold and the accuracy of the logical locations, as the reference grades
its Lore structure model -- ``TableWtwComputeMetric`` (eval/table_metric.py) over ``EvalUtils.load_table_pred_and_label`` / ``eval_table`` /
``PairTable`` (utils/eval/eval_utils.py) and ``TableEval`` (entity/table_entity.py:569-656), reading the ``center/<name>.txt`` + ``logi/<name>.txt`` files
``LoreProcessor.save_result`` writes (lore/processer_lore.py:190-228).

The rule, per (prediction, truth) table pair:
  * each table's cells are sorted by ``TableEval.bubble_sort``.  Its comparison ``is_priori`` is strict on (axis[2], axis[0], axis[3], axis[1]) and
    falsy on equality, so the bubble sort is a STABLE sort on that key (``sort_order``);
  * every truth cell takes the FIRST prediction cell, in sorted order, with ``compute_iou >= iou_threshold`` (``PairTable.matching``): the first, not the
    best, and nothing is removed, so one prediction cell may serve several truth cells;
  * ``compute_iou`` reads points 1 and 3 of the quads only: rec = (x1, y1, x3, y3); 0 where ``max(x1) >= min(x3) or min(y3) <= max(y1)``, else
    ``S_cross / (S1 + S2 - S_cross)`` with S = (x3 - x1) * (y3 - y1), S_cross = (d - u) * (r - l);
  * tp = matched truth cells, truep = those whose four axes equal the prediction cell's; precision = tp / n_pred, recall = tp / n_truth,
    acc = truep / tp, each ``None`` where the reference returns ``'null'`` (an empty side, tp == 0).
The truth's own sort changes only the order of the reference's ``match_list``; ``match`` here lists the truth cells in their INPUT order.

Arithmetic: float64 on inputs of any dtype (converted first).  That is what the reference computes on its evaluation path, where every coordinate is
``float()`` of a text file.  ``TableEval(bboxes=..., axis=...)`` on in-memory float32 arrays would compute in float32; that arithmetic is deliberately
not restated.  Ours, not the reference's: a non-finite coordinate, an axis outside int32 or ``iou_threshold <= 0`` is a ``ValueError`` (the reference
computes on with NaN), ``evaluate_dirs`` walks the truth's files in sorted order (the reference in ``os.listdir`` order, which moves the last bits of
the means), writes no files, and answers ``nan`` instead of ``ZeroDivisionError`` when no pair could be loaded.

Two routes with equal results: ``WtwMetric()`` is numpy on the host; ``WtwMetric(engine=HipEngine(0))`` packs a chunk of pairs, makes one pinned
upload, one launch of ``pt_op_cell_metric`` (csrc/cell_metric.hip, one workgroup per pair) and one copy back.  A pair with a table above 4096 cells is
scored by the host route and listed in ``last_fallback``."""
from __future__ import annotations

import os
import re
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .lib import PT_CELL_METRIC_MAX

Table = Tuple[np.ndarray, np.ndarray]

METRIC_KEYS = ("total", "error_total", "acs_null", "recall_null", "precision_null", "acc", "axis_ture_total", "axis_ture_radio", "det_precision",
               "det_recall", "f1", "bbox_acc", "bbox_true_total", "len_acc", "len_det_precision", "len_det_recall")
_SPLIT = re.compile(";|,")
_GT_TILE = 256          # host route: [256, 4096] float64 blocks, about ten of them alive: under 100 MB for a 4096 x 4096 pair


# ---- files ----------------------------------------------------------------------------------------------------------------------------------------
def load_table(center_file: str, logi_file: str) -> Table:
    """``TableEval.load_tabu``: the two files' lines zipped pairwise, a quad split on ';' or ',', the axes on ','; a line pair on which ``float`` / ``int``
    fails, or that holds fewer than 8 coordinates or 4 axes, is skipped.  -> (boxes float64 [n, 8], axes int64 [n, 4])"""
    with open(center_file) as fb, open(logi_file) as fa:
        lines_b, lines_a = fb.readlines(), fa.readlines()
    boxes, axes = [], []
    for lb, la in zip(lines_b, lines_a):
        try:
            b = [float(v) for v in _SPLIT.split(lb.strip())]
            a = [int(v) for v in la.strip().split(",")]
        except ValueError:
            continue
        if len(b) < 8 or len(a) < 4:
            continue
        boxes.append(b[:8])
        axes.append(a[:4])
    try:
        ax = np.asarray(axes, dtype=np.int64).reshape(-1, 4)
    except OverflowError as e:
        raise ValueError(f"{logi_file}: an axis outside int64") from e
    return np.asarray(boxes, dtype=np.float64).reshape(-1, 8), ax


def save_table(polygons, logi, center_file: str, logi_file: str) -> None:
    """what ``LoreProcessor.save_result`` writes, byte for byte: per cell ``x,y;x,y;x,y;x,y`` with ``f"{v:.5f}"`` and ``str(int(v))`` axes joined by
    ',', lines joined by a newline, one trailing newline (an empty table is a single newline)."""
    for f in (center_file, logi_file):
        os.makedirs(os.path.dirname(os.path.abspath(f)), exist_ok=True)
    rows = [";".join(f"{b[2 * i]:.5f},{b[2 * i + 1]:.5f}" for i in range(4)) for b in polygons]
    with open(center_file, "w") as f:
        f.write("\n".join(rows) + "\n")
    rows = [",".join(str(int(v)) for v in a) for a in logi]
    with open(logi_file, "w") as f:
        f.write("\n".join(rows) + "\n")


def table_from_result(table_dict: Dict, model: Optional[str] = None) -> Table:
    """(boxes, axes) of a pipeline or stage result carrying ``polygons`` [n, 8] and ``logi`` [n, 4]; the axes are ``int()`` of the stored values, as
    ``save_table`` writes them.  Only Lore's results carry logical locations."""
    if table_dict.get("logi") is None or table_dict.get("polygons") is None:
        who = model or table_dict.get("model") or ("a token model (SLANet, MtlTabNet, TableMaster)" if "structure_str_list" in table_dict
                                                    else "CenterNet")
        raise ValueError(f"the WTW cell metric needs 'polygons' and 'logi'; this result of {who} carries {sorted(table_dict.keys())}: only the Lore "
                         f"structure model predicts logical locations")
    boxes = np.asarray(table_dict["polygons"], dtype=np.float64).reshape(-1, 8)
    axes = np.asarray([[int(v) for v in a] for a in np.asarray(table_dict["logi"]).reshape(-1, 4)], dtype=np.int64).reshape(-1, 4)
    return boxes, axes


# ---- one pair, host route ---------------------------------------------------------------------------------------------------------------------------
def _table(t) -> Table:
    boxes = np.ascontiguousarray(np.asarray(t[0], dtype=np.float64).reshape(-1, 8))
    raw = np.asarray(t[1]).reshape(-1, 4)
    axes = np.ascontiguousarray(raw.astype(np.int64))
    if len(boxes) != len(axes):
        raise ValueError(f"{len(boxes)} boxes and {len(axes)} axes")
    if not np.isfinite(boxes).all():
        raise ValueError("a non-finite coordinate")
    if raw.dtype.kind == "f" and not np.array_equal(axes, raw):
        raise ValueError("an axis that is not an integer")
    if axes.size and (axes.min() < -2 ** 31 or axes.max() > 2 ** 31 - 1):
        raise ValueError("an axis outside int32")
    return boxes, axes


def _threshold(iou_threshold) -> float:
    thr = float(iou_threshold)
    if not thr > 0.0:
        raise ValueError(f"iou_threshold must be positive, not {iou_threshold!r}")
    return thr


def sort_order(axes) -> np.ndarray:
    """int64 [n]: the input indices in the order ``TableEval.bubble_sort`` leaves: a stable sort on (axis[2], axis[0], axis[3], axis[1])"""
    a = np.asarray(axes, dtype=np.int64).reshape(-1, 4)
    return np.lexsort((np.arange(len(a)), a[:, 1], a[:, 3], a[:, 0], a[:, 2])).astype(np.int64)


def _first_hits(pb: np.ndarray, gb: np.ndarray, thr: float) -> np.ndarray:
    """pb [n_pred, 8] in sorted order, gb [n_gt, 8] -> int64 [n_gt]: the first position in pb with iou >= thr, or -1"""
    out = np.full(len(gb), -1, dtype=np.int64)
    if len(pb) == 0:
        return out
    p0, p1, p2, p3 = (pb[None, :, k] for k in (0, 1, 4, 5))
    s2 = (p2 - p0) * (p3 - p1)
    with np.errstate(all="ignore"):
        for g in range(0, len(gb), _GT_TILE):
            t = gb[g:g + _GT_TILE]
            g0, g1, g2, g3 = (t[:, None, k] for k in (0, 1, 4, 5))
            left, right = np.maximum(g0, p0), np.minimum(g2, p2)
            up, down = np.maximum(g1, p1), np.minimum(g3, p3)
            s1 = (g2 - g0) * (g3 - g1)
            cross = (down - up) * (right - left)
            hit = (cross / (s1 + s2 - cross) >= thr) & ~((left >= right) | (down <= up))
            first = hit.argmax(axis=1)
            out[g:g + _GT_TILE] = np.where(hit[np.arange(len(t)), first], first, -1)
    return out


def _match_host(pred: Table, gt: Table, thr: float) -> Tuple[np.ndarray, int, int]:
    order = sort_order(pred[1])
    pos = _first_hits(pred[0][order], gt[0], thr)
    found = pos >= 0
    match = np.full(len(pos), -1, dtype=np.int64)
    match[found] = order[pos[found]]
    tp = int(found.sum())
    truep = int((pred[1][match[found]] == gt[1][found]).all(axis=1).sum()) if tp else 0
    return match, tp, truep


def match_pair(pred, gt, iou_threshold: float = 0.5) -> Tuple[np.ndarray, int, int]:
    """pred, gt: (boxes [n, 8], axes [n, 4]).  -> (match int64 [n_gt], tp, truep): per truth cell, in the truth's input order, the input index of the
    first prediction cell in the prediction's sorted order with iou >= iou_threshold, or -1; the matches; the matches with four equal axes."""
    return _match_host(_table(pred), _table(gt), _threshold(iou_threshold))


def _result(match: np.ndarray, tp: int, truep: int, n_pred: int, n_gt: int) -> Dict:
    """``PairTable.eval_bbox`` + ``eval_axis`` from the counts; None is the reference's 'null'"""
    return {"precision": tp / n_pred if n_pred > 0 else None, "recall": tp / n_gt if n_gt > 0 else None, "fp": n_pred - tp, "fn": n_gt - tp,
            "acc": None if n_gt == 0 or tp == 0 else truep / tp, "tp": tp, "truep": truep, "match": match}


def wtw_result(summary: Dict) -> Dict:
    """the nine keys ``TableWtwComputeMetric.__call__`` returns"""
    return {"acc": summary["acc"], "axis_ture_radio": summary["axis_ture_radio"], "axis_ture_total": summary["axis_ture_total"],
            "det_precision": summary["det_precision"], "det_recall": summary["det_recall"], "det_f1": summary["f1"], "det_bbox_acc": summary["bbox_acc"],
            "bbox_true_total": summary["bbox_true_total"], "total": summary["total"]}


# ---- the device route -------------------------------------------------------------------------------------------------------------------------------
def _pair_bytes(n_pred: int, n_gt: int) -> int:
    """device bytes of one pair in a chunk: 32 + 16 per cell, 4 per match, its record, offset and counts"""
    return 48 * (n_pred + n_gt) + 4 * n_gt + 32 + 8 + 8


def pack_chunk(tables: Sequence[Tuple[Table, Table]]):
    """-> (boxes float64 [N, 4] = (x1, y1, x3, y3), axes int32 [N, 4], pairs int64 [P, 4], moff int64 [P]) of a chunk of (pred, gt) pairs"""
    bs, as_, pairs, moff, at, m = [], [], [], [], 0, 0
    for (pb, pa), (gb, ga) in tables:
        pairs.append((at, len(pb), at + len(pb), len(gb)))
        moff.append(m)
        at += len(pb) + len(gb)
        m += len(gb)
        bs += [pb[:, (0, 1, 4, 5)], gb[:, (0, 1, 4, 5)]]
        as_ += [pa, ga]
    boxes = np.ascontiguousarray(np.concatenate(bs), dtype=np.float64) if bs else np.zeros((0, 4))
    axes = np.ascontiguousarray(np.concatenate(as_), dtype=np.int32) if as_ else np.zeros((0, 4), np.int32)
    return boxes, axes, np.asarray(pairs, dtype=np.int64).reshape(-1, 4), np.asarray(moff, dtype=np.int64)


def device_matches(engine, tables: Sequence[Tuple[Table, Table]], thr: float, events: Optional[list] = None):
    """one pinned upload, one pt_op_cell_metric launch, one copy back.  -> (match int32 [sum n_gt], counts int32 [P, 2], moff).  events: a list that
    receives the two device events around the launch (tools/cell_metric_bench.py times the kernel alone with them)."""
    import torch
    boxes, axes, pairs, moff = pack_chunk(tables)
    parts = [a.view(np.uint8).ravel() for a in (boxes, axes, pairs, moff)]
    offs, total = [], 0
    for a in parts:
        offs.append(total)
        total += (a.size + 15) // 16 * 16
    host = torch.empty((max(total, 16),), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    for o, a in zip(offs, parts):
        hv[o:o + a.size] = a
    dev = host.to(engine._tdev, non_blocking=True)
    view = lambda k, dtype, shape: dev[offs[k]:offs[k] + parts[k].size].view(dtype).reshape(shape)
    P, M = len(pairs), int(pairs[:, 3].sum())
    out = torch.empty((M + 2 * P,), dtype=torch.int32, device=engine._tdev)      # [matches | counts]: one copy back
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if events is not None else None
    if ev:
        ev[0].record()
    engine.op_cell_metric(view(0, torch.float64, (-1, 4)), view(1, torch.int32, (-1, 4)), view(2, torch.int64, (-1, 4)), pairs, thr,
                          moff=view(3, torch.int64, (-1,)), h_moff=moff, match=out, counts=out[M:], match_elems=M)
    if ev:
        ev[1].record()
        events.append(ev)
    got = out.cpu().numpy()
    return got[:M], got[M:].reshape(P, 2), moff


# ---- the public interface ---------------------------------------------------------------------------------------------------------------------------
class WtwMetric:
    """The WTW cell metric (see the module docstring).  engine: a HipEngine for the device route, None for numpy on the host.  scratch_budget: bytes of
    device memory one chunk of the device route may take for its cells, records and matches."""

    def __init__(self, engine=None, iou_threshold: float = 0.5, scratch_budget: int = 1 << 28):
        self.engine = engine
        self.iou_threshold = _threshold(iou_threshold)
        self.scratch_budget = int(scratch_budget)
        self.max_pairs = 65535
        self.last_fallback: List[int] = []
        self.events = None          # a list: receives the device events of every chunk (device_matches)

    def evaluate(self, pred, gt) -> Dict:
        return self.batch_evaluate([(pred, gt)])[0]

    def batch_evaluate(self, pairs) -> List[Dict]:
        """pairs: (pred, gt) with pred, gt = (boxes [n, 8], axes [n, 4]) -> per pair dict(precision, recall, fp, fn, acc, tp, truep, match)"""
        tables = [(_table(p), _table(g)) for p, g in pairs]
        thr = self.iou_threshold
        self.last_fallback = []
        out: List[Optional[Dict]] = [None] * len(tables)
        todo = []
        for k, (p, g) in enumerate(tables):
            n_pred, n_gt = len(p[0]), len(g[0])
            if n_pred == 0 or n_gt == 0:                                 # an empty side: nothing can match, no launch
                out[k] = _result(np.full(n_gt, -1, dtype=np.int64), 0, 0, n_pred, n_gt)
            elif self.engine is None or max(n_pred, n_gt) > PT_CELL_METRIC_MAX:
                if self.engine is not None:
                    self.last_fallback.append(k)
                out[k] = _result(*_match_host(p, g, thr), n_pred, n_gt)
            else:
                todo.append(k)
        for chunk in self._chunks(tables, todo):
            match, counts, moff = device_matches(self.engine, [tables[q] for q in chunk], thr, self.events)
            for j, q in enumerate(chunk):
                n_pred, n_gt = len(tables[q][0][0]), len(tables[q][1][0])
                out[q] = _result(match[moff[j]:moff[j] + n_gt].astype(np.int64), int(counts[j, 0]), int(counts[j, 1]), n_pred, n_gt)
        return out

    def _chunks(self, tables, todo):
        """the device route's calls: indices of `todo` in order, cut where the budget or max_pairs is reached"""
        chunk, used = [], 0
        for k in todo:
            need = _pair_bytes(len(tables[k][0][0]), len(tables[k][1][0]))
            if chunk and (used + need > self.scratch_budget or len(chunk) >= self.max_pairs):
                yield chunk
                chunk, used = [], 0
            chunk.append(k)
            used += need
        if chunk:
            yield chunk

    @staticmethod
    def summarize(per_pair: Sequence[Dict], error_total: int = 0) -> Dict:
        """``EvalUtils.eval_table``'s ``metric`` without its three time keys.  An empty mean and 0 / 0 are nan, as numpy gives there."""
        total = len(per_pair)
        acs = [r["acc"] for r in per_pair if r["acc"] is not None]
        precisions = [r["precision"] for r in per_pair if r["precision"] is not None]
        recalls = [r["recall"] for r in per_pair if r["recall"] is not None]
        axis_true = sum(1 for r in per_pair if r["acc"] == 1)
        bbox_true = sum(1 for r in per_pair if r["precision"] == 1 and r["recall"] == 1)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)               # numpy: "Mean of empty slice"
            acc, det_p, det_r = np.array(acs).mean(), np.array(precisions).mean(), np.array(recalls).mean()
            f1 = 2 * det_p * det_r / (det_p + det_r)
        ratio = lambda n: n / total if total else float("nan")
        return {"total": total, "error_total": int(error_total), "acs_null": total - len(acs), "recall_null": total - len(recalls),
                "precision_null": total - len(precisions), "acc": float(acc), "axis_ture_total": axis_true, "axis_ture_radio": ratio(axis_true),
                "det_precision": float(det_p), "det_recall": float(det_r), "f1": float(f1), "bbox_acc": ratio(bbox_true), "bbox_true_total": bbox_true,
                "len_acc": len(acs), "len_det_precision": len(precisions), "len_det_recall": len(recalls)}

    def evaluate_dirs(self, predict_path: str, label_path: str) -> Dict:
        """``load_table_pred_and_label`` + ``eval_table`` over <label_path>/gt_center, gt_logi and <predict_path>/center, logi.  A truth file whose
        prediction (or own logi file) is missing, or that is empty on either side after loading, goes to ``error_list``; names not ending in .txt are
        passed over.  -> dict(summary, error_list, file_names, per_pair, result = wtw_result(summary)); no file is written."""
        gt_center, gt_logi = os.path.join(label_path, "gt_center"), os.path.join(label_path, "gt_logi")
        center, logi = os.path.join(predict_path, "center"), os.path.join(predict_path, "logi")
        names, pairs, error_list = [], [], []
        for name in sorted(os.listdir(gt_center)):
            if not (os.path.exists(os.path.join(center, name)) and os.path.exists(os.path.join(logi, name)) and os.path.exists(os.path.join(gt_logi, name))):
                error_list.append(name)
                continue
            if not name.endswith(".txt"):
                continue
            pred, gt = load_table(os.path.join(center, name), os.path.join(logi, name)), load_table(os.path.join(gt_center, name), os.path.join(gt_logi, name))
            if len(pred[0]) > 0 and len(gt[0]) > 0:
                names.append(name)
                pairs.append((pred, gt))
            else:
                error_list.append(name)
        per_pair = self.batch_evaluate(pairs)
        summary = self.summarize(per_pair, len(error_list))
        return {"summary": summary, "error_list": error_list, "file_names": names, "per_pair": per_pair, "result": wtw_result(summary)}
