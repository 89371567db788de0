#!/usr/bin/env python
"""tests/golden/cell_metric.json from the REFERENCE's own classes: TableEval (entity/table_entity.py) read from files, PairTable and
EvalUtils.load_table_pred_and_label / eval_table (utils/eval/eval_utils.py).  Run where the reference tree exists:

    python tests/golden/make_golden_cell_metric.py

Only DATA is written: per case the text lines of the four files, the reference's sorted orders (input indices, recovered through id() of the units
before the bubble sort), its match_list as prediction input indices (-1 for EMPTY, in the truth's SORTED order, as the reference keeps it), eval_bbox()
and eval_axis(); and for one set of files the whole metric dict of eval_table minus its time keys, with the error_list.  os.listdir is held to sorted
order while load_table_pred_and_label runs: the reference sums its means in directory order, which is not a property of the metric."""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF_SRC, _pkg, _Stub, ref_import, stub_env  # noqa: E402,F401


def quad(x1, y1, x3, y3):
    return f"{x1:.5f},{y1:.5f};{x3:.5f},{y1:.5f};{x3:.5f},{y3:.5f};{x1:.5f},{y3:.5f}"


def grid(seed, rows, cols, jitter=0.0, drop=0.0, wrong=0.0, spans=True, shuffle=True):
    """a seeded ruled table: (truth center lines, truth logi lines, prediction center lines, prediction logi lines).  Cells of 40 x 20 pixels, some
    merged with the right neighbour; the prediction is the truth with corners moved by up to `jitter` pixels, a share `drop` of the cells missing, a
    share `wrong` with one axis off by one, in shuffled order."""
    rng = np.random.default_rng(seed)
    cells = []
    for r in range(rows):
        c = 0
        while c < cols:
            w = 2 if spans and c + 1 < cols and rng.random() < 0.15 else 1
            cells.append((c * 40.0 + 3, r * 20.0 + 5, (c + w) * 40.0 + 3, (r + 1) * 20.0 + 5, [c, c + w - 1, r, r]))
            c += w
    gt_order = rng.permutation(len(cells)) if shuffle else np.arange(len(cells))
    gc = [quad(*cells[k][:4]) for k in gt_order]
    gl = [",".join(str(v) for v in cells[k][4]) for k in gt_order]
    pc, pl = [], []
    for k in (rng.permutation(len(cells)) if shuffle else np.arange(len(cells))):
        if rng.random() < drop:
            continue
        x1, y1, x3, y3, ax = cells[k]
        d = rng.uniform(-jitter, jitter, 4) if jitter else np.zeros(4)
        ax = list(ax)
        if rng.random() < wrong:
            ax[int(rng.integers(0, 4))] += 1
        pc.append(quad(x1 + d[0], y1 + d[1], x3 + d[2], y3 + d[3]))
        pl.append(",".join(str(v) for v in ax))
    return gc, gl, pc, pl


def cases():
    """name -> (prediction center lines, prediction logi lines, truth center lines, truth logi lines)"""
    out = {}
    for name, args in {"grid_6x5_exact": (1, 6, 5, 0.0, 0.0, 0.0), "grid_8x7_jitter": (2, 8, 7, 3.0, 0.1, 0.05),
                       "grid_12x10_jitter": (3, 12, 10, 6.0, 0.1, 0.1), "grid_15x20_heavy": (4, 15, 20, 12.0, 0.2, 0.1),
                       "grid_5x4_axes_only": (5, 5, 4, 0.0, 0.0, 0.5)}.items():
        gc, gl, pc, pl = grid(*args)
        out[name] = (pc, pl, gc, gl)
    one = ["0,0;10,0;10,10;0,10"]
    # two prediction cells with EQUAL axes, both above 0.5 on the truth cell: the stable sort keeps the input order, so the first listed wins
    a, b = "0,0;10,0;10,9;0,9", "0,0;9,0;9,10;0,10"
    out["dup_keys_ab"] = ([a, b], ["1,1,2,2", "1,1,2,2"], one, ["1,1,2,2"])
    out["dup_keys_ba"] = ([b, a], ["1,1,2,2", "1,1,2,2"], one, ["1,1,2,2"])
    # both above 0.5; the one ranked later (top index 1) is the exact box: the earlier, worse one is taken
    out["later_has_higher_iou"] = (["0,0;10,0;10,10;0,10", "0,0;10,0;10,6;0,6"], ["0,0,1,1", "0,0,0,0"], one, ["0,0,1,1"])
    out["iou_exactly_half"] = (["0,0;1,0;1,1;0,1"], ["0,0,0,0"], ["0,0;2,0;2,1;0,1"], ["0,0,0,0"])
    out["iou_just_below_half"] = (["0,0;0.99999,0;0.99999,1;0,1"], ["0,0,0,0"], ["0,0;2,0;2,1;0,1"], ["0,0,0,0"])
    out["iou_just_above_half"] = (["0,0;1.00001,0;1.00001,1;0,1"], ["0,0,0,0"], ["0,0;2,0;2,1;0,1"], ["0,0,0,0"])
    out["touching"] = (["1,0;2,0;2,1;1,1", "0,1;1,1;1,2;0,2"], ["1,1,0,0", "0,0,1,1"], ["0,0;1,0;1,1;0,1"], ["0,0,0,0"])
    out["x3_below_x1"] = (["10,0;0,0;0,10;10,10", "0,0;10,0;10,10;0,10"], ["0,0,0,0", "0,0,0,0"],
                          ["0,0;10,0;10,10;0,10", "10,0;0,0;0,10;10,10", "12,0;2,0;2,-10;12,-10"], ["0,0,0,0", "1,1,0,0", "2,2,0,0"])
    out["zero_area_against_itself"] = (["5,5;5,5;5,5;5,5", "0,0;4,0;4,0;0,0"], ["0,0,0,0", "1,1,0,0"],
                                       ["5,5;5,5;5,5;5,5", "0,0;4,0;4,0;0,0"], ["0,0,0,0", "1,1,0,0"])
    out["one_pred_serves_three"] = (["0,0;10,0;10,10;0,10", "50,50;60,50;60,60;50,60"], ["0,0,0,0", "1,1,1,1"],
                                    ["0,0;10,0;10,10;0,10", "1,0;10,0;10,10;1,10", "0,0;10,0;10,8;0,8", "100,100;110,100;110,110;100,110"],
                                    ["0,0,0,0", "0,0,0,0", "5,5,5,5", "1,1,1,1"])
    # keys equal except the fourth axis (the third word of the sort key): the cell listed second sorts first and is taken
    out["fourth_axis_decides"] = (["0,0;10,0;10,9;0,9", "0,0;9,0;9,10;0,10"], ["0,0,0,1", "0,0,0,0"], one, ["0,0,0,0"])
    out["second_axis_decides"] = (["0,0;10,0;10,9;0,9", "0,0;9,0;9,10;0,10"], ["0,1,0,0", "0,0,0,0"], one, ["0,1,0,0"])
    out["negative_axis"] = (["0,0;10,0;10,9;0,9", "0,0;9,0;9,10;0,10", "20,0;30,0;30,10;20,10"], ["0,0,0,0", "0,0,-1,0", "-3,-3,-1,-1"],
                            ["0,0;10,0;10,10;0,10", "20,0;30,0;30,10;20,10"], ["0,0,-1,0", "-3,-3,-1,-1"])
    gc, gl, pc, pl = grid(7, 4, 4, 1.0, 0.0, 0.0)
    pc2, pl2 = list(pc), list(pl)
    pc2[5:5] = ["12,13;14,x;1,1;2,2", ""]                             # a malformed and an empty line: their logi lines go with them
    pl2[5:5] = ["9,9,9,9", "8,8,8,8"]
    pl2[9] = "1,2,3"                                                   # too few axes: the line pair is dropped
    gl2 = list(gl)
    gl2[2] = "1,1,a,1"
    out["malformed_lines"] = (pc2, pl2, gc, gl2)
    out["empty_pred"] = ([], [], one, ["0,0,0,0"])
    out["empty_gt"] = (one, ["0,0,0,0"], [], [])
    out["both_empty"] = ([], [], [], [])
    return out


SET = ["grid_6x5_exact", "grid_8x7_jitter", "grid_12x10_jitter", "grid_5x4_axes_only", "dup_keys_ab", "later_has_higher_iou", "touching",
       "malformed_lines", "one_pred_serves_three", "empty_pred"]      # the last is empty on one side; SET_MISSING has no prediction file at all
SET_MISSING = "iou_exactly_half"


def text(lines):
    return "\n".join(lines) + "\n"


def write_tree(root, cs, names, missing):
    for d in ("pred/center", "pred/logi", "label/gt_center", "label/gt_logi"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for n in list(names) + [missing]:
        pc, pl, gc, gl = cs[n]
        for d, lines in (("label/gt_center", gc), ("label/gt_logi", gl)) + ((("pred/center", pc), ("pred/logi", pl)) if n != missing else ()):
            with open(os.path.join(root, d, n + ".txt"), "w") as f:
                f.write(text(lines))


def main():
    stub_env()
    for m in ("pycocotools", "pycocotools.coco"):
        sys.modules.setdefault(m, _Stub(m))
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = _Stub("tqdm")
        sys.modules["tqdm"].tqdm = lambda it, **kw: it
    te = ref_import("pdftable.entity.table_entity")
    sys.modules["pdftable.entity"].TableEval = te.TableEval
    eu = ref_import("pdftable.utils.eval.eval_utils")
    TableEval, PairTable, EvalUtils = te.TableEval, eu.PairTable, eu.EvalUtils
    # _Stub swallows FileUtils.dump_json / TimeUtils.now_str_short (calls return None); sorted_dict likewise
    before = []
    orig_sort = TableEval.bubble_sort

    def spy(units):
        before.append([id(u) for u in units])
        return orig_sort(units)
    TableEval.bubble_sort = staticmethod(spy)

    cs = cases()
    out = {"cases": {}, "set": {}}
    null = lambda v: None if isinstance(v, str) and v == eu.NULL else (float(v) if isinstance(v, (float, np.floating)) else v)
    with tempfile.TemporaryDirectory() as tmp:
        for d in ("c", "l", "gc", "gl"):
            os.makedirs(os.path.join(tmp, d))
        for name, (pc, pl, gc, gl) in cs.items():
            for d, lines in (("c", pc), ("l", pl), ("gc", gc), ("gl", gl)):
                with open(os.path.join(tmp, d, name + ".txt"), "w") as f:
                    f.write(text(lines))
            del before[:]
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):      # load_tabu prints a traceback per bad line
                pred = TableEval(os.path.join(tmp, "c"), os.path.join(tmp, "l"), name + ".txt")
                gt = TableEval(os.path.join(tmp, "gc"), os.path.join(tmp, "gl"), name + ".txt")
            pidx = {u: k for k, u in enumerate(before[0])}
            gidx = {u: k for k, u in enumerate(before[1])}
            pair = PairTable(pred, gt)
            precision, recall, fp, fn = pair.eval_bbox()
            out["cases"][name] = {
                "center": pc, "logi": pl, "gt_center": gc, "gt_logi": gl,
                "pred_order": [pidx[id(u)] for u in pred.ulist], "gt_order": [gidx[id(u)] for u in gt.ulist],
                "match_sorted": [-1 if isinstance(u, str) else pidx[id(u)] for u in pair.match_list],
                "precision": null(precision), "recall": null(recall), "fp": int(fp), "fn": int(fn), "acc": null(pair.eval_axis()),
            }
        root = os.path.join(tmp, "tree")
        write_tree(root, cs, SET, SET_MISSING)
        real_listdir = os.listdir
        os.listdir = lambda p: sorted(real_listdir(p))
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                table_dict, error_list = EvalUtils.load_table_pred_and_label(os.path.join(root, "pred"), os.path.join(root, "label"))
                metric = EvalUtils.eval_table(table_dict, error_list, root)
        finally:
            os.listdir = real_listdir
        for k in ("start_time", "end_time", "use_time"):
            metric.pop(k)
        out["set"] = {"names": SET, "missing_pred": SET_MISSING, "error_list": list(error_list), "file_names": [t["file_name"] for t in table_dict],
                      "metric": {k: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for k, v in metric.items()}}
    path = os.path.join(HERE, "cell_metric.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(out["cases"]), "cases; set:", out["set"]["metric"], out["set"]["error_list"])


if __name__ == "__main__":
    main()
