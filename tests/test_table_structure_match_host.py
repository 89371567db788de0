"""pdf_table_amd/table_structure_match.py against what the reference's own TableMatch recorded (tests/golden/table_match.json, written by
tests/golden/make_table_match_golden.py): kept lines, match maps and HTML strings in both modes, exactly; and the OcrTablePipeline constructor
behaviours of the token route that need no engine."""
import json
import os

import numpy as np
import pytest

from pdf_table_amd import table_structure_match as M

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "table_match.json")) as _f:
    GOLD = json.load(_f)["cases"]


def arrays(case):
    cells = np.array(case["cells"], dtype=case["cell_dtype"])
    lines = np.array(case["lines"], dtype=np.int64).reshape(-1, 4)
    return cells, lines


def chain(html):
    """the tags match_table_structure_and_text_cell strips from TableMatch's string"""
    for a, b in (("<html><body>", ""), ("</body></html>", ""), ("<tbody>", ""), ("</tbody>", ""), ("</tr>", "</tr>\n"),
                 ("<table>", "<table class='pdf-table' border='1'>")):
        html = html.replace(a, b)
    return html


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_reproduces_the_reference(case):
    cells, lines = arrays(case)
    kept = M.filter_lines(cells, lines)
    assert kept.tolist() == case["kept"]
    matched = M.match_result(lines[kept], cells)
    assert [[k, v] for k, v in matched.items()] == case["matched"]
    rec = [(case["texts"][i], 1) for i in kept.tolist()]
    assert M.pred_html(case["tokens"], matched, rec) == case["html"]
    assert M.pred_html_master(case["tokens"], matched, rec) == case["html_master"]
    for master, key in ((False, "html"), (True, "html_master")):
        got = M.structure_table_html(case["tokens"], cells, lines, case["texts"], master)
        assert got == [chain(case[key])]
        # a match map handed in (the device's: line indices into the texts given) is used as it is
        by_page = {k: [int(kept[i]) for i in v] for k, v in matched.items()}
        assert M.structure_table_html(case["tokens"], cells, None, case["texts"], master, matched=by_page) == got


def test_float_text_boxes_are_the_integer_ones():
    case = next(c for c in GOLD if c["name"] == "random_f32_dense")
    cells, lines = arrays(case)
    for dt in (np.float32, np.float64):
        assert [[k, v] for k, v in M.match_result(lines.astype(dt), cells).items()] == case["matched"]


def test_float32_area_decides_the_golden_case():
    """the recorded case exists for one reason: with the cell's own area in float64 the other cell wins"""
    case = next(c for c in GOLD if c["name"] == "f32_area_decides")
    cells, lines = arrays(case)
    assert cells.dtype == np.float32
    w32 = list(M.match_result(lines, cells))[0]
    w64 = list(M.match_result(lines, cells.astype(np.float64)))[0]
    assert w32 == case["matched"][0][0] and w64 == case["float64_winner"] and w32 != w64


def test_goldens_cover_what_they_claim():
    by = {c["name"]: c for c in GOLD}
    assert by["y_filter"]["kept"] == [0, 3, 4]                                        # ymax == smallest y kept, one pixel above dropped
    assert by["iou0_equal_distance"]["matched"] == [[1, [0]]] and by["identical_cells"]["matched"][0] == [1, [0]]
    assert "<b>" in by["html_lines"]["texts"] and "" in by["html_lines"]["texts"]
    assert any("<eb" in t for t in by["html_master_tokens"]["tokens"]) and "<thead>" in by["html_master_tokens"]["tokens"]
    assert {c["cell_dtype"] for c in GOLD} == {"float32", "int32"} and {len(c["cells"][0]) for c in GOLD} == {4, 8}


def test_four_value_cells_are_not_reordered():
    """match_result takes a 4-value box as it is (no min / max): a box given upside down keeps its negative extent"""
    cells = np.array([[10, 30, 50, 10], [10, 10, 50, 30]], np.float32)
    k1, _ = M.match_keys(np.array([[12, 12, 48, 28]]), cells)
    assert k1[0, 0] == 1.0 and k1[0, 1] < 1.0


def test_table_without_cells_gets_no_html():
    assert M.structure_table_html(["<html>"], np.array([]), np.zeros((0, 4)), [], False) == []
    assert M.structure_table_html(["<html>"], np.zeros((0, 8), np.float32), np.array([[1, 2, 3, 4]]), ["x"], True) == []


def test_use_master_follows_the_model():
    assert [M.use_master_for(m) for m in ("SLANet", "MtlTabNet", "TableMaster", "Lgpma", "Lore")] == [False, True, True, True, False]


def test_shared_master_helpers_are_the_mtl_ones():
    from pdf_table_amd import mtl_stage
    assert M.deal_bb is mtl_stage.deal_bb and M.deal_eb_token is mtl_stage.deal_eb_token


# ---- OcrTablePipeline: what the constructor decides before any engine exists ----------------------------------------------------------
def test_pipeline_slanet_without_a_model_directory_is_refused_before_an_engine_exists(monkeypatch):
    from pdf_table_amd import pipeline as P

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(P, "HipEngine", no_engine)
    with pytest.raises(ValueError, match="out of scope"):
        P.OcrTablePipeline(table_structure=True, table_structure_model="SLANet", synthetic_seed=0)
    with pytest.raises(ValueError, match="tsr_task_path"):
        P.OcrTablePipeline(table_structure=True, table_structure_model="SLANet", table_html=True)


def test_pipeline_slanet_with_a_model_directory_reaches_the_engine(monkeypatch, tmp_path):
    """with tsr_task_path the constructor no longer refuses: the first thing it does is create the engine"""
    from pdf_table_amd import pipeline as P

    class Reached(Exception):
        pass

    def engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "HipEngine", engine)
    with pytest.raises(Reached):
        P.OcrTablePipeline(table_structure=True, table_structure_model="SLANet", tsr_task_path=str(tmp_path), table_html=True)


def test_attach_html_dispatches_on_the_table_dict():
    """no engine: _attach_html only reads the stage results.  Token route for dicts with structure_str_list and no logi (the stage's match map for
    SLANet, the host match with use_master for MtlTabNet), [] for a table without cells"""
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.table_text_match import text_boxes, texts_in_table
    case = next(c for c in GOLD if c["name"] == "html_master_tokens")
    cells, lines = arrays(case)
    quads = lines[:, [0, 1, 2, 1, 2, 3, 0, 3]].astype(np.float64)
    far = np.array([[900, 900, 950, 900, 950, 920, 900, 920]], np.float64)              # a line outside the table box: never a candidate
    boxes = [np.concatenate([far, quads])]
    texts = [["far away"] + case["texts"]]
    pipe = OcrTablePipeline.__new__(OcrTablePipeline)
    pipe.table_structure_model = "MtlTabNet"
    tsr = [[{"polygons": cells[:, [0, 1, 2, 1, 2, 3, 0, 3]], "structure_str_list": case["tokens"]},
            {"polygons": np.array([]), "structure_str_list": ["<html>"]}]]
    tb = [np.array([[5, 5, 305, 65], [5, 5, 305, 65]])]
    pipe._attach_html(tsr, tb, boxes, texts)
    inside = texts_in_table([5, 5, 305, 65], text_boxes(boxes[0]), diff=2)
    assert inside.tolist() == list(range(1, 14))
    assert tsr[0][0]["table_html"] == [chain(case["html_master"])] and tsr[0][0]["db_table_html"] == tsr[0][0]["table_html"]
    assert tsr[0][1]["table_html"] == [] and tsr[0][1]["db_table_html"] == []
    # SLANet: the stage's map (cell ordinal -> page line indices) and use_master False
    pipe.table_structure_model = "SLANet"
    matched = {k: [i + 1 for i in v] for k, v in case["matched"]}
    one = [[{"polygons": tsr[0][0]["polygons"], "structure_str_list": case["tokens"], "matched": matched}]]
    pipe._attach_html(one, [tb[0][:1]], boxes, texts)
    assert one[0][0]["table_html"] == [chain(case["html"])]
    del one[0][0]["matched"], one[0][0]["table_html"]
    with pytest.raises(RuntimeError, match="matched"):
        pipe._attach_html(one, [tb[0][:1]], boxes, texts)
