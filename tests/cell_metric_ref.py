"""The WTW cell metric restated loop for loop -- bubble sort, matching, eval_bbox, eval_axis and eval_table's sums -- as the reference's TableEval /
PairTable / EvalUtils.eval_table run them (entity/table_entity.py:569-656, utils/eval/eval_utils.py:23-113,196-284), for the tests on machines
without the reference tree.  Shares no code with pdf_table_amd/cell_metric.py.  Coordinates are numpy float64 scalars, as TableBBox's points are, so
a zero denominator is inf / nan with a warning, not an exception."""
import re
import warnings

import numpy as np

EMPTY = "empty"
NULL = "null"


class Unit:
    def __init__(self, bbox, axis, index):
        self.point1 = np.array([[bbox[0], bbox[1]]])
        self.point3 = np.array([[bbox[4], bbox[5]]])
        self.axis = axis
        self.index = index          # the input position: what the tests compare


def load_lines(center_lines, logi_lines):
    units = []
    for bbox, axis in zip(center_lines, logi_lines):
        try:
            bbox = list(map(float, re.split(";|,", bbox.strip())))
            axis = list(map(int, axis.strip().split(",")))
            axis[3], bbox[7]
            units.append(Unit(bbox, axis, len(units)))
        except Exception:
            pass
    return units


def units_of(boxes, axes):
    return [Unit([float(v) for v in b], [int(v) for v in a], k) for k, (b, a) in enumerate(zip(boxes, axes))]


def is_priori(a, b):
    ka, kb = a.axis, b.axis
    if ka[2] < kb[2]:
        return True
    elif ka[2] > kb[2]:
        return False
    if ka[0] < kb[0]:
        return True
    elif ka[0] > kb[0]:
        return False
    if ka[3] < kb[3]:
        return True
    elif ka[3] > kb[3]:
        return False
    if ka[1] < kb[1]:
        return True
    elif ka[1] > kb[1]:
        return False


def bubble_sort(units):
    units = list(units)
    length = len(units)
    for index in range(length):
        for j in range(1, length - index):
            if is_priori(units[j], units[j - 1]):
                units[j - 1], units[j] = units[j], units[j - 1]
    return units


def compute_iou(b1, b2):
    rec1 = (b1.point1[0][0], b1.point1[0][1], b1.point3[0][0], b1.point3[0][1])
    rec2 = (b2.point1[0][0], b2.point1[0][1], b2.point3[0][0], b2.point3[0][1])
    left_column_max = max(rec1[0], rec2[0])
    right_column_min = min(rec1[2], rec2[2])
    up_row_max = max(rec1[1], rec2[1])
    down_row_min = min(rec1[3], rec2[3])
    if left_column_max >= right_column_min or down_row_min <= up_row_max:
        return 0
    S1 = (rec1[2] - rec1[0]) * (rec1[3] - rec1[1])
    S2 = (rec2[2] - rec2[0]) * (rec2[3] - rec2[1])
    S_cross = (down_row_min - up_row_max) * (right_column_min - left_column_max)
    return S_cross / (S1 + S2 - S_cross)


def matching(pred_sorted, gt_sorted, iou_threshold=0.5):
    match_list = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for tunit in gt_sorted:
            if_find = 0
            for sunit in pred_sorted:
                if compute_iou(tunit, sunit) >= iou_threshold:
                    match_list.append(sunit)
                    if_find = 1
                    break
            if if_find == 0:
                match_list.append(EMPTY)
    return match_list


def eval_bbox(match_list, n_pred, n_gt):
    tp = sum(1 for u in match_list if u is not EMPTY)
    recall = tp / n_gt if n_gt > 0 else NULL
    precision = tp / n_pred if n_pred > 0 else NULL
    return precision, recall, n_pred - tp, n_gt - tp


def eval_axis(match_list, gt_sorted):
    tp = sum(1 for u in match_list if u is not EMPTY)
    truep = 0
    for i in range(len(gt_sorted)):
        pred_unit = match_list[i]
        if pred_unit is not EMPTY:
            flag = True
            for j in range(4):
                if pred_unit.axis[j] != gt_sorted[i].axis[j]:
                    flag = False
                    break
            if flag:
                truep += 1
    if len(gt_sorted) == 0:
        return NULL, truep
    return (NULL if tp == 0 else truep / tp), truep


def pair(pred_units, gt_units, iou_threshold=0.5):
    """-> dict in the package's terms: match int list in the truth's INPUT order (pred input index or -1), the sorted orders, the reference's figures with
    None for 'null'"""
    ps, gs = bubble_sort(pred_units), bubble_sort(gt_units)
    ml = matching(ps, gs, iou_threshold)
    match = [-1] * len(gt_units)
    for g, u in zip(gs, ml):
        match[g.index] = -1 if u is EMPTY else u.index
    precision, recall, fp, fn = eval_bbox(ml, len(ps), len(gs))
    acc, truep = eval_axis(ml, gs)
    none = lambda v: None if v is NULL else v
    return {"pred_order": [u.index for u in ps], "gt_order": [u.index for u in gs], "match_sorted": [-1 if u is EMPTY else u.index for u in ml],
            "match": match, "precision": none(precision), "recall": none(recall), "fp": fp, "fn": fn, "acc": none(acc),
            "tp": sum(1 for u in ml if u is not EMPTY), "truep": truep}


def eval_table(results, error_total=0):
    """eval_table's metric (without the time keys) from pair() results"""
    total = len(results)
    acs, precisions, recalls = [], [], []
    axis_ture, bbox_accs, acs_null, recall_null, precision_null = 0, [], 0, 0, 0
    for i, r in enumerate(results):
        if r["acc"] is not None:
            acs.append(r["acc"])
        else:
            acs_null += 1
        if r["acc"] == 1:
            axis_ture += 1
        if r["precision"] is not None:
            precisions.append(r["precision"])
        else:
            precision_null += 1
        if r["recall"] is not None:
            recalls.append(r["recall"])
        else:
            recall_null += 1
        if r["precision"] == 1 and r["recall"] == 1:
            bbox_accs.append(i)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        result_acc = np.array(acs).mean()
        det_precision = np.array(precisions).mean()
        det_recall = np.array(recalls).mean()
        f = 2 * det_precision * det_recall / (det_precision + det_recall)
    return {"total": total, "error_total": error_total, "acs_null": acs_null, "recall_null": recall_null, "precision_null": precision_null,
            "acc": float(result_acc), "axis_ture_total": axis_ture, "axis_ture_radio": axis_ture / total, "det_precision": float(det_precision),
            "det_recall": float(det_recall), "f1": float(f), "bbox_acc": len(bbox_accs) / total, "bbox_true_total": len(bbox_accs), "len_acc": len(acs),
            "len_det_precision": len(precisions), "len_det_recall": len(recalls)}
