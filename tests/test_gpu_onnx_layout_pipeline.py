"""A PicoDet ONNX export through the product API: ``OcrTablePipeline(layout=True, layout_task_path=<dir with model.onnx>)`` and the stage behind it,
``OnnxLayoutStage`` (pdf_table_amd/layout_stage.py): the engine's pre-processing kernel, the executor's captured layer walk, ONE
pt_op_pico_candidates launch on the graph's outputs, one pinned copy of the candidate records, LayoutStage's host decode.

Stand-in (the real ``*_layout_infer`` files are not available offline): ``tools/onnx_export.py:PicoLike(ncls=5, levels=4)`` seeded as in
tests/test_gpu_onnx_seq.py::test_layout_task_onnx_door -- seed 21, head bias -2 on the class rows, class weights x 3 -- exported at 800 x 608 with a
dynamic batch: a few dozen regions per page, every one of them "text".  For the table tests a second file whose stride-8 head has its "table" bias
raised by 0.25: on the fp32 module that adds 38 to 61 small "table" regions per generator page (checked on the CPU with oracle/picodet.py), far
enough from none that the engine's 16-bit arithmetic cannot lose them all.

The comparison is the synchronous route ``OcrLayoutTask._detect_pages_host`` (every anchor copied to the host, numpy filters) and, for the stream,
``predict()`` of the same pipeline: the kernel converts and copies only, so every comparison is EXACT -- label, category id, score and bbox bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu


def _export(path, table_bias=0.0):
    import onnx_export as X
    m = X.seeded(X.PicoLike(ncls=5, levels=4), 21)
    with torch.no_grad():
        for h in m.heads:
            h.bias[:5] -= 2.0
            h.weight[:5] *= 3.0
        m.heads[0].bias[3] += table_bias
    (path / "model.onnx").write_bytes(X.torch_export(m, torch.zeros(1, 3, 800, 608), dynamic_batch=True))
    return path


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return _export(tmp_path_factory.mktemp("pico_text"))


@pytest.fixture(scope="module")
def standin_tables(tmp_path_factory):
    return _export(tmp_path_factory.mktemp("pico_tables"), table_bias=0.25)


@pytest.fixture(scope="module")
def pages():
    from pdf_table_amd.synth_pages import make_page
    return [make_page(i, 1024)[0] for i in range(3)]


def _text_detector(p):
    """bench.py's detector on the pipeline's engine: the seeded DB-ResNet18 with the text channel, so that the boxes are the pages' lines"""
    from pdf_table_amd import lib as L
    from pdf_table_amd.det_stage import DetConfig
    from pdf_table_amd.synth_weights import db_resnet18_state_dict
    from pdf_table_amd.weights import pack_db_resnet18
    p.engine.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=p.engine.weight_fmt))
    p.text_detector._stage.cfg = DetConfig(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5).resolved()
    return p


@pytest.fixture(scope="module")
def pipe(standin):
    from pdf_table_amd.pipeline import OcrTablePipeline
    p = _text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_task_path=str(standin)))
    yield p
    p.engine.close()


def _same_layout(a, b):
    """two per-page result lists, element for element, bit for bit"""
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert len(pa) == len(pb)
        for ra, rb in zip(pa, pb):
            assert ra["label"] == rb["label"] and ra["category_id"] == rb["category_id"]
            assert np.asarray(ra["score"]).tobytes() == np.asarray(rb["score"]).tobytes()
            assert ra["bbox"].dtype == rb["bbox"].dtype and ra["bbox"].tobytes() == rb["bbox"].tobytes()


def _same(ra, rb, tables=False):
    assert len(ra) == len(rb)
    for a, b in zip(ra, rb):
        _same_layout([a.layout_result], [b.layout_result])
        assert np.array_equal(a.det_result, b.det_result)
        assert [e["text"] for e in a.ocr_result] == [e["text"] for e in b.ocr_result]
        assert all(np.array_equal(x["bbox"], y["bbox"]) for x, y in zip(a.ocr_result, b.ocr_result))
        assert a.rotated_180 == b.rotated_180
        if tables:
            assert len(a.table_structure_result) == len(b.table_structure_result)
            for ta, tb in zip(a.table_structure_result, b.table_structure_result):
                if ta is None or tb is None:
                    assert ta is None and tb is None
                    continue
                assert np.array_equal(ta["polygons"], tb["polygons"]) and np.array_equal(ta["logi"], tb["logi"])
                assert ta.get("table_html") == tb.get("table_html")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_stage_equals_host_route(standin, pages, precision):
    from pdf_table_amd.layout_stage import OnnxLayoutStage
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    task = OcrLayoutTask(model="picodet", task_type="en", task_path=str(standin), precision=precision)
    try:
        assert type(task._stage) is OnnxLayoutStage and task._exec.precision == {"bf16": "bf16", "fp32": "bf16x3"}[precision]
        pages_t = torch.from_numpy(np.stack(pages)).to(task._engine._tdev)
        want = task._detect_pages_host(pages_t)
        assert min(len(w) for w in want) >= 3, [len(w) for w in want]
        got = task._stage(pages_t)
        assert task._stage._tail_ok and all(task._stage._tail_ok.values())      # the device tail served it, not the fallback
        _same_layout(got, want)
        _same_layout(task.detect_pages(pages_t), want)
        _same_layout([task(pages[1])[0]], [want[1]])                            # the reference's per-image door
        print(f"ONNX layout stage {precision}: regions per page {[len(w) for w in want]}")
    finally:
        task._engine.close()


def test_eager_captured_and_replayed_walks(pipe, pages):
    task, stage = pipe.layout_task, pipe.layout_task._stage
    dev = pipe.engine._tdev
    a = torch.from_numpy(np.stack(pages[:2])).to(dev)
    b = torch.from_numpy(np.stack(pages[1:3])).to(dev)
    org = tuple(a.shape[1:3])
    runs = []
    for _ in range(4):                                                           # eager (remembered), capture + replay, replay, replay
        n, ticket = stage.forward(a)
        runs.append(stage.finish(n, ticket, org))
    assert n == 2 and min(len(r) for r in runs[0]) >= 3
    for r in runs[1:]:
        _same_layout(r, runs[0])
    assert any(k[0][0] == 2 for k in stage.exec._graphs) or os.environ.get("PT_ONNX_GRAPH", "1") == "0"      # this batch shape has its captured graph
    want_b = task._detect_pages_host(b)
    _same_layout(runs[0], task._detect_pages_host(a))
    # a forward() queued before the previous finish(): two landing buffers, and the graph's buffers replayed over in between
    na, ta = stage.forward(a)
    nb, tb = stage.forward(b)
    assert ta[1][1].data_ptr() != tb[1][1].data_ptr()
    _same_layout(stage.finish(na, ta, org), runs[0])
    _same_layout(stage.finish(nb, tb, org), want_b)
    assert any(len(x) != len(y) or any(p["bbox"].tobytes() != q["bbox"].tobytes() for p, q in zip(x, y)) for x, y in zip(runs[0], want_b))


def test_predict_equals_the_task(pipe, pages):
    from pdf_table_amd.layout_stage import OnnxLayoutStage
    assert type(pipe.layout_task._stage) is OnnxLayoutStage and pipe.layout_task.synthetic_seed is None
    assert pipe.text_detector.synthetic_seed == 0                               # the file is served beside seeded stages
    res = pipe.predict(pages)
    pages_t = torch.from_numpy(np.stack(pages)).to(pipe.engine._tdev)
    want = pipe.layout_task._detect_pages_host(pages_t)
    assert min(len(w) for w in want) >= 3
    _same_layout([r.layout_result for r in res], want)
    _same_layout(pipe.layout_task.detect_pages(pages_t), want)
    assert sum(len(r.det_result) for r in res) >= 20 and all(len(r.ocr_result) == len(r.det_result) for r in res)


def test_stream_equals_predict(pipe, pages, standin):
    """fails without OnnxLayoutStage: predict_stream() took the task's stage, the in-tree net -- seeded, or without weights when no seed is given --
    instead of the file"""
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    from pdf_table_amd.pipeline import OcrTablePipeline
    batches = [[pages[0], pages[1]], [pages[1], pages[2]], [pages[2], pages[0]], [pages[0], pages[1]]]
    want = [pipe.predict(b) for b in batches]
    assert all(len(r.layout_result) >= 3 and len(r.det_result) >= 10 for w in want for r in w)
    got = list(pipe.predict_stream(batches))
    assert len(got) == 4
    for g, w in zip(got, want):
        _same(g, w)
    # what the stream returns is the FILE's result: the task door on the same file, built on its own (no seed)
    door = OcrLayoutTask(model="picodet", task_type="en", task_path=str(standin), engine=pipe.engine)
    _same_layout([r.layout_result for r in got[1]], door.detect_pages(torch.from_numpy(np.stack(batches[1])).to(pipe.engine._tdev)))
    pipe.aux_layout = True
    try:
        got = list(pipe.predict_stream(batches))
    finally:
        pipe.aux_layout = False
    for g, w in zip(got, want):
        _same(g, w)
    # the stage handed to from_engine
    q = OcrTablePipeline.from_engine(pipe.engine, pipe.text_detector._stage, pipe.text_recognizer._stage, layout_stage=pipe.layout_task._stage)
    _same(q.predict(batches[1]), want[1])
    for g, w in zip(q.predict_stream(batches[:2]), want[:2]):
        _same(g, w)


def test_tables_and_html_from_this_layout(standin_tables, pages):
    from pdf_table_amd.pipeline import OcrTablePipeline
    p = _text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_task_path=str(standin_tables), table_structure=True, table_html=True))
    try:
        batch = pages[:2]
        pages_t = torch.from_numpy(np.stack(batch)).to(p.engine._tdev)
        host = p.layout_task._detect_pages_host(pages_t)
        n_tables = [sum(r["label"] == "table" for r in lay) for lay in host]
        assert min(n_tables) >= 1, n_tables                                     # the host route alone yields table regions on these pages
        want = p.predict(batch)
        _same_layout([r.layout_result for r in want], host)
        # every table's crop box is one of this layout's "table" regions: as many results as regions that leave a crop, and the same results
        # when those regions are handed in as table_boxes
        tb = p._layout_table_boxes(host)
        kept = p._drop_empty_crops(tb, tuple(pages_t.shape[1:3]))
        assert [len(k) for k in kept] == [len(t) for t in tb]                   # no region of these pages lies outside its page
        assert [len(r.table_structure_result) for r in want] == [len(t) for t in tb] and sum(len(t) for t in tb) >= 1
        given = p.predict(batch, table_boxes=tb)
        _same(given, want, tables=True)
        assert any("table_html" in t for r in want for t in r.table_structure_result if t is not None)
        got = list(p.predict_stream([batch, batch]))
        assert len(got) == 2
        _same(got[0], want, tables=True)
        _same(got[1], want, tables=True)
        print(f"tables from the ONNX layout: table regions per page {n_tables}, crops {[len(k) for k in kept]}")
    finally:
        p.engine.close()


def test_orientation_vote_second_layout_pass(standin, pages):
    from pdf_table_amd import lib as L
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    p = _text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_task_path=str(standin), text_orientation=True))
    try:
        p.engine.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True), fmt=p.engine.weight_fmt))
        flipped = np.ascontiguousarray(pages[1][::-1, ::-1])
        batches = [[pages[0], flipped], [flipped, pages[2]]]
        want = [p.predict(b) for b in batches]
        assert [r.rotated_180 for w in want for r in w] == [False, True, True, False]
        assert all(len(r.layout_result) >= 3 for w in want for r in w)
        for attrs in ({}, {"aux_layout": True}):
            for k, v in attrs.items():
                setattr(p, k, v)
            got = list(p.predict_stream(batches, orientation_vote=True))
            assert len(got) == 2
            for g, w in zip(got, want):
                _same(g, w)
                assert [r.text_upright for r in g] == [r.text_upright for r in w]
    finally:
        p.engine.close()


def test_in_tree_pipeline_is_unchanged(pages):
    """without layout_task_path the stage is LayoutStage on the seeded in-tree net, and two constructions give the same results"""
    from pdf_table_amd.layout_stage import LayoutStage
    from pdf_table_amd.pipeline import OcrTablePipeline
    res = []
    for _ in range(2):
        p = _text_detector(OcrTablePipeline(synthetic_seed=0, layout=True))
        try:
            assert type(p.layout_task._stage) is LayoutStage and p.layout_task.synthetic_seed == 4 and p.layout_task._exec is None
            res.append((p.predict(pages[:2]), list(p.predict_stream([pages[:2]]))[0]))
        finally:
            p.engine.close()
    _same(res[0][0], res[1][0])
    _same(res[0][1], res[1][1])
    _same(res[0][0], res[0][1])
