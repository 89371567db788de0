"""pdf_table_amd/cell_metric.py, host route (no GPU), and tests/cell_metric_ref.py against tests/golden/cell_metric.json -- what the reference's own
TableEval, PairTable and EvalUtils.eval_table gave for the same files (tests/golden/make_golden_cell_metric.py).  Every integer, order, None and summary
value is compared exactly: floats with ==, nan matching nan."""
import json
import math
import os

import numpy as np
import pytest

import cell_metric_ref as R
from pdf_table_amd import cell_metric as M
from pdf_table_amd import lib as L
from pdf_table_amd.cell_metric import WtwMetric

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

with open(os.path.join(HERE, "golden", "cell_metric.json")) as _f:
    GOLD = json.load(_f)
CASES = GOLD["cases"]


def same(a, b):
    """== with nan matching nan and None matching None only"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def text(lines):
    return "\n".join(lines) + "\n"


def write_case(d, case, name, pred=True):
    for sub, key in (("label/gt_center", "gt_center"), ("label/gt_logi", "gt_logi")) + ((("pred/center", "center"), ("pred/logi", "logi")) if pred else ()):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
        with open(os.path.join(d, sub, name + ".txt"), "w") as f:
            f.write(text(case[key]))


def load_case(tmp_path, name):
    write_case(str(tmp_path), CASES[name], name)
    p = lambda sub: os.path.join(str(tmp_path), sub, name + ".txt")
    return M.load_table(p("pred/center"), p("pred/logi")), M.load_table(p("label/gt_center"), p("label/gt_logi"))


def test_fixture_has_the_cases_it_should():
    assert len(CASES) >= 20 and max(len(c["gt_center"]) for c in CASES.values()) <= 300
    assert CASES["dup_keys_ab"]["match_sorted"] == [0] and CASES["dup_keys_ba"]["match_sorted"] == [0]      # stability decides
    assert CASES["later_has_higher_iou"]["match_sorted"] == [1] and CASES["later_has_higher_iou"]["pred_order"] == [1, 0]
    assert CASES["iou_exactly_half"]["match_sorted"] == [0] and CASES["iou_just_below_half"]["match_sorted"] == [-1]
    assert CASES["touching"]["match_sorted"] == [-1] and CASES["zero_area_against_itself"]["match_sorted"] == [-1, -1]
    assert CASES["one_pred_serves_three"]["match_sorted"].count(0) == 3
    assert CASES["fourth_axis_decides"]["pred_order"] == [1, 0] and CASES["fourth_axis_decides"]["match_sorted"] == [1]
    assert CASES["empty_pred"]["precision"] is None and CASES["empty_gt"]["recall"] is None and CASES["empty_gt"]["acc"] is None
    assert len(CASES["malformed_lines"]["pred_order"]) == len(CASES["malformed_lines"]["center"]) - 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_package_and_restatement_reproduce_the_reference(tmp_path, name):
    want = CASES[name]
    pred, gt = load_case(tmp_path, name)
    assert pred[0].dtype == np.float64 and pred[1].dtype == np.int64 and pred[0].shape[1:] == (8,) and pred[1].shape[1:] == (4,)
    # the package
    assert M.sort_order(pred[1]).tolist() == want["pred_order"] and M.sort_order(gt[1]).tolist() == want["gt_order"]
    got = WtwMetric().evaluate(pred, gt)
    assert got["match"].dtype == np.int64
    assert [int(got["match"][g]) for g in want["gt_order"]] == want["match_sorted"]
    tp = sum(1 for m in want["match_sorted"] if m >= 0)
    assert (got["tp"], got["fp"], got["fn"]) == (tp, want["fp"], want["fn"])
    for k in ("precision", "recall", "acc"):
        assert same(got[k], want[k]), (k, got[k], want[k])
    m, tp2, truep = M.match_pair(pred, gt)
    assert m.tolist() == got["match"].tolist() and (tp2, truep) == (got["tp"], got["truep"])
    assert got["acc"] is None or got["acc"] == truep / tp
    # the loop-for-loop restatement the GPU tests use
    ref = R.pair(R.load_lines(want["center"], want["logi"]), R.load_lines(want["gt_center"], want["gt_logi"]))
    for k in ("pred_order", "gt_order", "match_sorted", "fp", "fn"):
        assert ref[k] == want[k], k
    for k in ("precision", "recall", "acc"):
        assert same(ref[k], want[k]), k
    assert ref["match"] == got["match"].tolist() and (ref["tp"], ref["truep"]) == (got["tp"], got["truep"])


def test_evaluate_dirs_equals_the_reference_summary(tmp_path):
    s = GOLD["set"]
    for n in s["names"]:
        write_case(str(tmp_path), CASES[n], n)
    write_case(str(tmp_path), CASES[s["missing_pred"]], s["missing_pred"], pred=False)
    with open(os.path.join(str(tmp_path), "label", "gt_center", "notes.md"), "w") as f:      # exists on the truth side only: an error, as in the reference
        f.write("x\n")
    got = WtwMetric().evaluate_dirs(os.path.join(str(tmp_path), "pred"), os.path.join(str(tmp_path), "label"))
    assert got["error_list"] == sorted(s["error_list"] + ["notes.md"]) and got["file_names"] == s["file_names"]
    want = dict(s["metric"], error_total=s["metric"]["error_total"] + 1)
    assert set(got["summary"]) == set(want) == set(M.METRIC_KEYS)
    for k, v in want.items():
        assert same(got["summary"][k], v), (k, got["summary"][k], v)
    assert got["result"] == {"acc": want["acc"], "axis_ture_radio": want["axis_ture_radio"], "axis_ture_total": want["axis_ture_total"],
                             "det_precision": want["det_precision"], "det_recall": want["det_recall"], "det_f1": want["f1"],
                             "det_bbox_acc": want["bbox_acc"], "bbox_true_total": want["bbox_true_total"], "total": want["total"]}
    assert sorted(os.listdir(str(tmp_path))) == ["label", "pred"]            # nothing written
    # the restatement's eval_table gives the same summary from its own pairs
    ref = [R.pair(R.load_lines(CASES[n[:-4]]["center"], CASES[n[:-4]]["logi"]), R.load_lines(CASES[n[:-4]]["gt_center"], CASES[n[:-4]]["gt_logi"]))
           for n in s["file_names"]]
    rs = R.eval_table(ref, len(s["error_list"]))
    for k, v in s["metric"].items():
        assert same(rs[k], v), (k, rs[k], v)
    # summarize() on the package's own per-pair results, and on nothing at all
    assert all(same(WtwMetric.summarize(got["per_pair"], 3)[k], v) for k, v in dict(want, error_total=3).items())
    empty = WtwMetric.summarize([])
    assert empty["total"] == 0 and all(math.isnan(empty[k]) for k in ("acc", "det_precision", "det_recall", "f1", "axis_ture_radio", "bbox_acc"))


def test_nan_f1_when_nothing_matches():
    far = (np.asarray([[100, 100, 110, 100, 110, 110, 100, 110]]), np.asarray([[0, 0, 0, 0]]))
    near = (np.asarray([[0, 0, 10, 0, 10, 10, 0, 10]]), np.asarray([[0, 0, 0, 0]]))
    r = WtwMetric().evaluate(far, near)
    assert (r["precision"], r["recall"], r["acc"], r["tp"], r["fp"], r["fn"]) == (0.0, 0.0, None, 0, 1, 1)
    s = WtwMetric.summarize([r])
    assert s["det_precision"] == 0.0 and math.isnan(s["f1"]) and math.isnan(s["acc"]) and s["acs_null"] == 1 and s["len_acc"] == 0


def test_save_table_bytes_and_round_trip(tmp_path):
    polys = np.asarray([[0.5, 1.25, 10, 1.25, 10, 7.123456, 0.5, 7.123456], [-3, 0, 1e3, 0, 1e3, 2, -3, 2]], dtype=np.float32)
    logi = np.asarray([[0, 1, 2, 3], [4.0, 4.0, -1.0, 7.9]], dtype=np.float32)
    c, l = str(tmp_path / "center" / "a.txt"), str(tmp_path / "logi" / "a.txt")
    M.save_table(polys, logi, c, l)
    assert open(c, "rb").read() == (b"0.50000,1.25000;10.00000,1.25000;10.00000,7.12346;0.50000,7.12346\n"
                                    b"-3.00000,0.00000;1000.00000,0.00000;1000.00000,2.00000;-3.00000,2.00000\n")
    assert open(l, "rb").read() == b"0,1,2,3\n4,4,-1,7\n"
    boxes, axes = M.load_table(c, l)
    assert axes.tolist() == [[0, 1, 2, 3], [4, 4, -1, 7]]
    assert np.array_equal(boxes, np.asarray([[float(f"{v:.5f}") for v in p] for p in polys]))
    M.save_table(boxes, axes, c, l)                                      # a second trip changes nothing
    b2, a2 = M.load_table(c, l)
    assert np.array_equal(b2, boxes) and np.array_equal(a2, axes)
    M.save_table(np.zeros((0, 8)), np.zeros((0, 4)), c, l)              # an empty table is one newline, as "\n".join([]) + "\n" is
    assert open(c, "rb").read() == b"\n" and M.load_table(c, l)[0].shape == (0, 8)
    t = M.table_from_result({"polygons": polys, "logi": logi})
    assert t[0].dtype == np.float64 and t[1].tolist() == [[0, 1, 2, 3], [4, 4, -1, 7]]


def test_refusals():
    ok = (np.asarray([[0, 0, 10, 0, 10, 10, 0, 10.0]]), np.asarray([[0, 0, 0, 0]]))
    bad = (np.asarray([[0, 0, 10, 0, np.nan, 10, 0, 10.0]]), np.asarray([[0, 0, 0, 0]]))
    inf = (np.asarray([[0, 0, 10, 0, 10, 10, 0, np.inf]]), np.asarray([[0, 0, 0, 0]]))
    for t in (bad, inf):
        with pytest.raises(ValueError, match="non-finite"):
            M.match_pair(t, ok)
        with pytest.raises(ValueError, match="non-finite"):
            WtwMetric().evaluate(ok, t)
    for thr in (0, 0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="iou_threshold"):
            M.match_pair(ok, ok, iou_threshold=thr)
        with pytest.raises(ValueError, match="iou_threshold"):
            WtwMetric(iou_threshold=thr)
    with pytest.raises(ValueError, match="int32"):
        M.match_pair((ok[0], np.asarray([[0, 0, 2 ** 31, 0]])), ok)
    with pytest.raises(ValueError, match="CenterNet"):
        M.table_from_result({"polygons": ok[0]})
    with pytest.raises(ValueError, match="token model"):
        M.table_from_result({"structure_str_list": ["<td>"], "polygons": ok[0]})
    with pytest.raises(ValueError, match="MyNet"):
        M.table_from_result({"polygons": ok[0]}, model="MyNet")
    assert M.match_pair(ok, ok, iou_threshold=1.0)[0].tolist() == [0]     # IoU 1 reaches a threshold of 1


def test_inputs_of_any_dtype_are_float64_first():
    """float32 corners whose float32 IoU arithmetic would differ: the metric converts, then computes in float64"""
    rng = np.random.default_rng(3)
    b = rng.uniform(0, 50, (40, 8)).astype(np.float32)
    b[:, 4:6] = b[:, 0:2] + rng.uniform(1, 30, (40, 2)).astype(np.float32)
    a = rng.integers(0, 6, (40, 4)).astype(np.int16)
    r32 = M.match_pair((b, a), (b[::-1], a[::-1]))
    r64 = M.match_pair((b.astype(np.float64), a.astype(np.int64)), (b[::-1].astype(np.float64), a[::-1].astype(np.int64)))
    assert r32[0].tolist() == r64[0].tolist() and r32[1:] == r64[1:]
    ref = R.pair(R.units_of(b, a), R.units_of(b[::-1], a[::-1]))
    assert ref["match"] == r64[0].tolist() and (ref["tp"], ref["truep"]) == r64[1:]


def test_host_tiles_agree_with_one_block():
    """more truth cells than one host tile (256): the tiled scan equals the restatement"""
    rng = np.random.default_rng(9)
    n = 300
    x, y = rng.uniform(0, 400, n), rng.uniform(0, 400, n)
    w, h = rng.uniform(5, 60, n), rng.uniform(5, 60, n)
    gb = np.stack([x, y, x + w, y, x + w, y + h, x, y + h], 1)
    pb = gb + rng.uniform(-4, 4, gb.shape)
    ga = rng.integers(0, 4, (n, 4))
    pa = ga.copy()
    pa[::7, 1] += 1
    m, tp, truep = M.match_pair((pb, pa), (gb, ga))
    ref = R.pair(R.units_of(pb, pa), R.units_of(gb, ga))
    assert m.tolist() == ref["match"] and (tp, truep) == (ref["tp"], ref["truep"]) and 0 < truep < tp


def test_entry_point_is_declared_bound_and_dispatched():
    assert L.EXPECTED_ABI == 21
    L.load()
    assert "pt_op_cell_metric" in L.EXPORTS and L.PT_CELL_METRIC_MAX == 4096
    from pdf_table_amd import build as B
    protos = {name: params for _, name, params in B._prototypes()}
    assert "pt_op_cell_metric" in protos
    assert len(protos["pt_op_cell_metric"].split(",")) == len(L.EXPORTS["pt_op_cell_metric"][1]) == 13
    assert "cell_metric.hip" in B.ONCE_HIP_SOURCES
    assert "pt_bf16::api::pt_op_cell_metric(" in B.dispatch_source()
    hdr = open(os.path.join(REPO, "include", "pdftable_hip.h")).read()
    assert "#define PT_CELL_METRIC_MAX 4096" in hdr
    from pdf_table_amd.engine import HipEngine
    assert callable(HipEngine.op_cell_metric)
