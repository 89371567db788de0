"""device_decode=True through the stages and the pipeline: LayoutStage / OnnxLayoutStage queue pt_op_layout_decode behind their candidate kernels and
land (counts, detection counts, detections) instead of the records; OcrTablePipeline(layout_device_decode=True) hands the knob on.

Stage tests: the same stage object family runs the same pages with the knob off, then on.  The off run's LANDED records feed the margin checker
(tests/layout_decode_ref.py) page by page; a page where a decision could flip within 4 x its own host-vs-float64 difference is left out -- at most a
quarter of the pages, never all, and with these pages and seeds none (the counts are printed).  The other pages must give the same labels in the
same order, boxes and scores within that bound.  Pipeline tests: predict(), predict_stream() and the stage agree bit for bit among themselves."""
import warnings

import numpy as np
import pytest
import torch

import layout_decode_ref as R
import test_gpu_onnx_layout_pipeline as P

pytestmark = pytest.mark.gpu


def export_sparse(path):
    """The stand-in for the on-against-off comparison.  P._export's head answers the white background of the generator pages with the SAME score on
    hundreds of anchors (474 candidates a page, about 200 exactly equal pairs even in the pair mode, whose outputs carry 16 mantissa bits): ties, for
    which no reference order exists.  Here only the stride-8 head can pass, and its class bias is set between the background's logit (1.50 with
    the class weights x 3) and those of the anchors that see print (the 20th best of a page is near 1.79), which leaves a few dozen distinct
    candidates a page; the other levels' class biases are far below zero.  Measured on the GPU before the values were fixed."""
    import onnx_export as X
    m = X.seeded(X.PicoLike(ncls=5, levels=4), 21)
    with torch.no_grad():
        m.heads[0].weight[:5] *= 3.0
        m.heads[0].bias[:5] -= 1.79
        for h in m.heads[1:]:
            h.bias[:5] -= 30.0
    (path / "model.onnx").write_bytes(X.torch_export(m, torch.zeros(1, 3, 800, 608), dynamic_batch=True))
    return path


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return P._export(tmp_path_factory.mktemp("pico_text_dd"))


@pytest.fixture(scope="module")
def standin_sparse(tmp_path_factory):
    return export_sparse(tmp_path_factory.mktemp("pico_sparse_dd"))


@pytest.fixture(scope="module")
def standin_tables(tmp_path_factory):
    return P._export(tmp_path_factory.mktemp("pico_tables_dd"), table_bias=0.25)


@pytest.fixture(scope="module")
def pages():
    from pdf_table_amd.synth_pages import make_page
    return [make_page(i, 1024)[0] for i in range(4)]


def _landed_cases(stage, ticket, n, org, probs):
    """the records an off-run landed -> one margin-checker case per page"""
    ticket[0].synchronize()
    counts = ticket[1][0][:n].numpy().copy()
    assert (counts <= stage.max_cands).all()
    rec = ticket[1][1][:n].numpy()
    return [{"name": f"page{i}", "rec": rec[i, :counts[i]].copy(), "cfg": stage.config, "org": tuple(org), "probs": probs} for i in range(n)]


def _compare_pages(cases, off, on, what, min_regions):
    left_out, n_regions = [], []
    for i, (case, a, b) in enumerate(zip(cases, off, on)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d_box, d_score, same = R.host_vs_64(case)
        if not (same and R.margins_ok(case, 4 * d_box, 4 * d_score)):
            left_out.append(i)
            continue
        n_regions.append(len(a))
        assert [r["label"] for r in a] == [r["label"] for r in b] and [r["category_id"] for r in a] == [r["category_id"] for r in b]
        e_box = max((float(np.abs(x["bbox"] - y["bbox"]).max()) for x, y in zip(a, b)), default=0.0)
        e_score = max((abs(float(x["score"]) - float(y["score"])) for x, y in zip(a, b)), default=0.0)
        print(f"{what} page {i}: {len(case['rec'])} records, {len(a)} regions, host vs float64 {d_box:.3g} / {d_score:.3g}, device vs host {e_box:.3g} / {e_score:.3g}")
        assert e_box <= 4 * d_box and e_score <= 4 * d_score
        assert all(y["bbox"].dtype == np.float64 and y["bbox"].shape == (4,) for y in b)
    print(f"{what}: {len(left_out)} of {len(cases)} pages left out {left_out}, regions per compared page {n_regions}")
    assert len(left_out) * 4 <= len(cases) and len(left_out) < len(cases)
    assert sum(n_regions) >= min_regions


def test_in_tree_stage_on_against_off(pages):
    from pdf_table_amd.layout_stage import LayoutStage
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    task = OcrLayoutTask(model="picodet", task_type="en", synthetic_seed=4)
    try:
        off = task._stage
        assert type(off) is LayoutStage and not off.device_decode
        on = LayoutStage(task._engine, task._config, device_decode=True)
        pages_t = torch.from_numpy(np.stack(pages)).to(task._engine._tdev)
        org = tuple(pages_t.shape[1:3])
        n, ticket = off.forward(pages_t)
        cases = _landed_cases(off, ticket, n, org, probs=False)
        want = off.finish(n, ticket, org)
        m, t_on = on.forward(pages_t)
        assert m == n and len(t_on[1]) == 3 and t_on[1][2].shape[1:] == (5 * 100, 6)      # counts, detection counts, detections: 24 KB a page
        got = on.finish(m, t_on, org)
        _compare_pages(cases, want, got, "in-tree stage", min_regions=1)
        P._same_layout(on(pages_t), got)                                                      # the second landing buffer, the same result
    finally:
        task._engine.close()


def test_onnx_stage_on_against_off(standin_sparse, pages):
    from pdf_table_amd.layout_stage import OnnxLayoutStage
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    task = OcrLayoutTask(model="picodet", task_type="en", task_path=str(standin_sparse), precision="fp32")
    try:
        off = task._stage
        on = OnnxLayoutStage(task._engine, task._exec, task._config, device_decode=True)
        dev = task._engine._tdev
        a = torch.from_numpy(np.stack(pages[:2])).to(dev)
        b = torch.from_numpy(np.stack(pages[2:4])).to(dev)
        org = tuple(a.shape[1:3])
        cases, want = [], []
        for x in (a, b):
            n, ticket = off.forward(x)
            cases += _landed_cases(off, ticket, n, org, probs=True)
            want += off.finish(n, ticket, org)
        runs = []
        for _ in range(4):                                   # eager (remembered), capture + replay, replay, replay
            n, ticket = on.forward(a)
            runs.append(on.finish(n, ticket, org))
        for r in runs[1:]:
            P._same_layout(r, runs[0])
        na, ta = on.forward(a)                               # two forwards in flight: two landing buffers
        nb, tb = on.forward(b)
        assert ta[1][2].data_ptr() != tb[1][2].data_ptr()
        got_a, got_b = on.finish(na, ta, org), on.finish(nb, tb, org)
        P._same_layout(got_a, runs[0])
        assert on._tail_ok and all(on._tail_ok.values())
        _compare_pages(cases, want, got_a + got_b, "ONNX stage fp32", min_regions=6)
    finally:
        task._engine.close()


def test_pipeline_predict_stream_and_stage_agree(standin, pages):
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    from pdf_table_amd.pipeline import OcrTablePipeline
    with pytest.raises(ValueError, match="layout_device_decode"):
        OcrTablePipeline(synthetic_seed=0, layout=False, layout_device_decode=True)
    p = P._text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_task_path=str(standin), layout_device_decode=True))
    try:
        stage = p.layout_task._stage
        assert stage.device_decode
        batches = [[pages[0], pages[1]], [pages[1], pages[2]], [pages[2], pages[0]]]
        want = [p.predict(b) for b in batches]
        assert all(len(r.layout_result) >= 3 for w in want for r in w)
        for k, b in enumerate(batches):
            P._same_layout([r.layout_result for r in want[k]], stage(torch.from_numpy(np.stack(b)).to(p.engine._tdev)))
        for attrs in ({}, {"aux_layout": True}):
            for key, v in attrs.items():
                setattr(p, key, v)
            got = list(p.predict_stream(batches))
            assert len(got) == 3
            for g, w in zip(got, want):
                P._same(g, w)
        p.aux_layout = False
        q = OcrTablePipeline.from_engine(p.engine, p.text_detector._stage, p.text_recognizer._stage, layout_stage=stage)
        P._same(q.predict(batches[1]), want[1])
        # the knob is per task: a door built without it on the same engine and file lands records
        door = OcrLayoutTask(model="picodet", task_type="en", task_path=str(standin), engine=p.engine)
        assert not door._stage.device_decode
    finally:
        p.engine.close()


def test_pipeline_with_tables_and_html(standin_tables, pages):
    from pdf_table_amd.pipeline import OcrTablePipeline
    p = P._text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_task_path=str(standin_tables), table_structure=True, table_html=True,
                                          layout_device_decode=True))
    try:
        batch = pages[:2]
        want = p.predict(batch)
        assert sum(r["label"] == "table" for w in want for r in w.layout_result) >= 1
        assert any("table_html" in t for r in want for t in r.table_structure_result if t is not None)
        got = list(p.predict_stream([batch, batch]))
        assert len(got) == 2
        P._same(got[0], want, tables=True)
        P._same(got[1], want, tables=True)
    finally:
        p.engine.close()


def test_pipeline_with_orientation_vote(standin, pages):
    from pdf_table_amd import lib as L
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    p = P._text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_task_path=str(standin), text_orientation=True, layout_device_decode=True))
    try:
        p.engine.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True), fmt=p.engine.weight_fmt))
        flipped = np.ascontiguousarray(pages[1][::-1, ::-1])
        batches = [[pages[0], flipped], [flipped, pages[2]]]
        want = [p.predict(b) for b in batches]
        assert [r.rotated_180 for w in want for r in w] == [False, True, True, False]
        assert all(len(r.layout_result) >= 3 for w in want for r in w)
        got = list(p.predict_stream(batches, orientation_vote=True))
        assert len(got) == 2
        for g, w in zip(got, want):
            P._same(g, w)
    finally:
        p.engine.close()
