"""Table HTML through the product API for the structure models that give tokens + one box per cell: ``OcrTablePipeline(table_structure_model=
"SLANet", tsr_task_path=..., table_html=True)`` -- SlaNetStage matches every table's lines to its cells on the device (pt_op_table_match) -- and
``"MtlTabNet"`` (the host match with use_master).  The SLANet graph is the stand-in of tools/onnx_export_slanet.py at the reduced sizes of
tests/test_gpu_slanet_door.py (network input 128 x 128, T = 24); detector, recogniser and MtlTabNet are seeded.  Every expectation is computed by hand
from the result's own polygons, tokens and lines with pdf_table_amd/table_structure_match.py, which tests/test_table_structure_match_host.py pins to
the reference's recorded results."""
import os
import shutil
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from pdf_table_amd import table_structure_match as M  # noqa: E402
from pdf_table_amd.synth_pages import make_page  # noqa: E402
from pdf_table_amd.table_text_match import text_boxes, texts_in_table  # noqa: E402

pytestmark = pytest.mark.gpu

DICTS = os.path.join(REPO, "tests", "golden", "slanet")
SIZE, STEPS = 128, 24
TABLE_BOXES = [np.array([[30, 40, 600, 400]]), np.array([[20, 30, 330, 250], [300, 200, 630, 470]])]


def pages():
    return [make_page(i)[0][:480, :640].copy() for i in (0, 1)]


@pytest.fixture(scope="module")
def sla(tmp_path_factory):
    from onnx_export_slanet import SlaNetLike, export_slanet, seeded_slanet
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.rec_postprocess import TableLabelDecode
    d = str(tmp_path_factory.mktemp("slanet_pipeline"))
    for name in ("table_structure_dict.txt", "table_structure_dict_ch.txt"):
        shutil.copy(os.path.join(DICTS, name), d)
    dec = TableLabelDecode(os.path.join(DICTS, "table_structure_dict.txt"), merge_no_span_structure=True)
    net = seeded_slanet(SlaNetLike(n_cls=30, n_loc=4, steps=STEPS), 2, cell_ids=(dec.dict["<td"], dec.dict["<td></td>"]), cell_bias=9.0)
    with open(os.path.join(d, "model.onnx"), "wb") as f:
        f.write(export_slanet(net, SIZE))
    pipe = OcrTablePipeline(synthetic_seed=0, table_structure=True, table_structure_model="SLANet", tsr_task_path=d, table_html=True, lang="en",
                            table_max_len=SIZE)
    return pipe, pipe.predict(pages(), table_boxes=TABLE_BOXES)


def by_hand(page_result, box, table, use_master):
    """-> (table_html, match map in page line indices) from the result's own polygons, tokens and lines"""
    quads = np.array([e["bbox"] for e in page_result.ocr_result], np.float64).reshape(-1, 8)
    texts = [e["text"] for e in page_result.ocr_result]
    tbx = text_boxes(quads) if len(quads) else np.zeros((0, 4))
    cand = texts_in_table([float(v) for v in box], tbx, diff=2) if len(tbx) else np.zeros(0, np.int64)
    cells = np.asarray(table["polygons"])
    html = M.structure_table_html(table["structure_str_list"], cells, tbx[cand], [texts[i] for i in cand], use_master)
    matched = {}
    if cells.ndim == 2 and len(cells) and len(cand):
        kept = M.filter_lines(cells, tbx[cand])
        matched = {c: [int(cand[kept[i]]) for i in ls] for c, ls in M.match_result(tbx[cand][kept], cells).items()}
    return html, matched, cand


def test_predict_attaches_the_token_route_html(sla):
    pipe, res = sla
    assert [len(r.table_structure_result) for r in res] == [1, 2]
    n_lines = n_matched = n_cells = 0
    for r, boxes in zip(res, TABLE_BOXES):
        assert np.array_equal(text_boxes(np.array([e["bbox"] for e in r.ocr_result], np.float64).reshape(-1, 8)) if len(r.ocr_result) else np.zeros((0, 4)),
                              text_boxes(r.det_result) if len(r.det_result) else np.zeros((0, 4)))
        for box, table in zip(boxes, r.table_structure_result):
            html, matched, cand = by_hand(r, box, table, use_master=False)
            print(f"table {box.tolist()}: {len(table['polygons'])} cells, {len(cand)} candidate lines, matched {table['matched']}")
            assert table["matched"] == matched                       # the kernel's map = the host match_result on the same boxes
            assert table["table_html"] == html and table["db_table_html"] == html
            assert all(0 <= c < len(table["polygons"]) for c in matched)
            if len(table["polygons"]):
                assert len(html) == 1 and html[0].startswith("<table class='pdf-table' border='1'>") and "<html>" not in html[0]
            else:
                assert html == []
            n_lines, n_matched, n_cells = n_lines + len(cand), n_matched + sum(len(v) for v in matched.values()), n_cells + len(table["polygons"])
    assert n_cells > 0 and n_lines > 0 and n_matched > 0             # the seeded stages do give cells and lines: nothing above was vacuous


def test_predict_stream_returns_what_predict_returns(sla):
    pipe, res = sla
    out = list(pipe.predict_stream([pages()], table_boxes=[TABLE_BOXES]))
    assert len(out) == 1 and len(out[0]) == 2
    for a, b in zip(out[0], res):
        assert np.array_equal(a.det_result, b.det_result) and [e["text"] for e in a.ocr_result] == [e["text"] for e in b.ocr_result]
        assert len(a.table_structure_result) == len(b.table_structure_result)
        for ta, tb in zip(a.table_structure_result, b.table_structure_result):
            assert ta["structure_str_list"] == tb["structure_str_list"] and np.array_equal(ta["polygons"], tb["polygons"])
            assert ta["matched"] == tb["matched"] and ta["table_html"] == tb["table_html"] and ta["db_table_html"] == tb["db_table_html"]


def test_stage_without_text_boxes_is_unchanged(sla):
    """no text_boxes: the dict the stage gave before (no 'matched'), the same polygons and tokens"""
    import torch
    pipe, res = sla
    batch = torch.from_numpy(np.stack(pages())).to(pipe.engine._tdev)
    plain = pipe.table_structure_task.recognize_tables(batch, TABLE_BOXES)
    for page, r in zip(plain, res):
        for t, want in zip(page, r.table_structure_result):
            assert set(t) == {"polygons", "structure_str_list", "score"}
            assert t["structure_str_list"] == want["structure_str_list"] and np.array_equal(t["polygons"], want["polygons"])
    with pytest.raises(ValueError, match="page_frame"):
        pipe.table_structure_task.recognize_tables(batch, TABLE_BOXES, page_frame=False, text_boxes=[np.zeros((0, 4)), np.zeros((0, 4))])


def test_stage_matches_many_lines_over_two_micro_batches(sla):
    """the seeded detector finds few lines; 60 seeded integer line boxes per page (dozens per table) through the stage, three tables as micro-batches
    of 2 + 1: 'matched' must be the host match_result on the stage's own polygons"""
    import torch
    pipe, _ = sla
    stage = pipe.table_structure_task._stage
    g = np.random.default_rng(3)
    lines = []
    for _ in range(2):
        xy = np.stack([g.integers(0, 560, 60), g.integers(0, 450, 60)], 1)
        lines.append(np.concatenate([xy, xy + np.stack([g.integers(10, 80, 60), g.integers(8, 30, 60)], 1)], 1).astype(np.float64))
    batch = torch.from_numpy(np.stack(pages())).to(pipe.engine._tdev)
    keep, stage.micro_batch = stage.micro_batch, 2
    try:
        got = stage(batch, TABLE_BOXES, page_frame=True, text_boxes=lines)
    finally:
        stage.micro_batch = keep
    total = 0
    for page, boxes, tbx in zip(got, TABLE_BOXES, lines):
        for box, table in zip(boxes, page):
            cand = texts_in_table([float(v) for v in box], tbx, diff=2)
            cells = np.asarray(table["polygons"])
            kept = M.filter_lines(cells, tbx[cand])
            want = {c: [int(cand[kept[i]]) for i in ls] for c, ls in M.match_result(tbx[cand][kept], cells).items()}
            print(f"table {box.tolist()}: {len(cells)} cells, {len(cand)} candidates, {len(kept)} kept, {len(want)} cells with lines")
            assert table["matched"] == want
            total += len(kept)
    assert total >= 20


def test_mtl_tabnet_gets_master_html():
    """MtlTabNet (int32 polygons made on the host): the numpy match and get_pred_html_master; before the token route existed this was []"""
    from pdf_table_amd.pipeline import OcrTablePipeline
    pipe = OcrTablePipeline(synthetic_seed=59, table_structure=True, table_structure_model="MtlTabNet", table_html=True, max_seq_len=20,
                            max_seq_len_cell=6)
    page = pages()[:1]
    box = TABLE_BOXES[0]
    res = pipe.predict(page, table_boxes=[box])
    table = res[0].table_structure_result[0]
    html, matched, cand = by_hand(res[0], box[0], table, use_master=True)
    print(f"MtlTabNet: {len(table['polygons'])} cells, {len(cand)} candidate lines, matched {matched}")
    assert len(table["polygons"]) > 0 and len(cand) > 0
    assert len(table["table_html"]) == 1 and table["table_html"][0] and table["table_html"] == html and table["db_table_html"] == html
    out = list(pipe.predict_stream([page], table_boxes=[[box]]))[0]
    assert out[0].table_structure_result[0]["table_html"] == html
