"""DocXLayout through the product API: ``DocXLayoutStage`` against the CPU restatement chain, the task's doors, and
``OcrTablePipeline(layout=True, layout_model="DocXLayout", layout_task_path=<checkpoint>)`` in predict() and predict_stream().  The model has
no in-tree weights: every test writes a seeded checkpoint to a temporary directory and passes its path."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docxlayout_ref as R  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.docxlayout_stage import DOCX_MEAN, DOCX_STD, DocXLayoutConfig, DocXLayoutStage  # noqa: E402
from pdf_table_amd.synth_weights import docxlayout_dla34_state_dict  # noqa: E402
from pdf_table_amd.weights import pack_docxlayout_dla34  # noqa: E402

pytestmark = pytest.mark.gpu

# the small chain.  The seed is chosen on the CPU: of the seeds 0 .. 99 whose three pages all give regions, the one on which the restatement's
# decisions are settled by the widest margin (tests/docxlayout_ref.py: chain_headroom), so that no page is left out
CHAIN_SEED, CHAIN_KW = 78, {}
CHAIN_RES = (128, 160)


def _chain_pages():
    from pdf_table_amd.synth_pages import make_page
    return [np.ascontiguousarray(make_page(i, 1024)[0][100:356, 60:380]) for i in range(3)]


def _restated_input(page, inp_h, inp_w):
    from oracle import lore_pre
    trans, _ = lore_pre.lore_preprocess_geometry(page.shape[0], page.shape[1], inp_h, inp_w, False)
    warped = lore_pre.warp_affine_u8(np.ascontiguousarray(page[:, :, ::-1]), trans, inp_w, inp_h)
    x = ((warped / 255. - np.array(DOCX_MEAN, np.float32).reshape(1, 1, 3)) / np.array(DOCX_STD, np.float32).reshape(1, 1, 3)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]


def _same_layout(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert len(pa) == len(pb), (len(pa), len(pb))
        for ra, rb in zip(pa, pb):
            assert ra["label"] == rb["label"] and ra["category_id"] == rb["category_id"] and ra["score"] == rb["score"], (ra, rb)
            assert ra["bbox"].dtype == rb["bbox"].dtype and ra["bbox"].tobytes() == rb["bbox"].tobytes(), (ra, rb)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """the default seeded checkpoint in the reference's layout: a directory holding pytorch_model.bin with a ``state_dict`` entry"""
    d = tmp_path_factory.mktemp("docx")
    torch.save({"state_dict": {"module." + k: v for k, v in docxlayout_dla34_state_dict(seed=0).items()}}, str(d / "pytorch_model.bin"))
    return str(d)


@pytest.fixture(scope="module")
def pages():
    from pdf_table_amd.synth_pages import make_page
    return [make_page(i, 1024)[0] for i in range(3)]


def test_stage_fp32_equals_restatement_chain():
    """three 256 x 320 pages at resolution (128, 160), pair mode: the stage's final lists equal the fp32 restatement chain's.  The golden
    generator's margin rule is asserted on the pages first.  Measured on an MI355X: the restatement's decisions on these pages hold for head
    maps within 1e-5 .. 2e-5 of max|head| (printed), the engine's maps are within 7e-5 at worst (tests/test_gpu_docxlayout.py) -- no seed of
    0 .. 99 reaches the 2e-4 that tests/docxlayout_ref.py writes down as the safe margin, so the second leg repeats the comparison with the
    network taken out: the restatement's decode and host chain on the engine's own head maps, exact whatever the margins."""
    from pdf_table_amd.engine import HipEngine
    sd = docxlayout_dla34_state_dict(seed=CHAIN_SEED, **CHAIN_KW)
    pgs = _chain_pages()
    hw = pgs[0].shape[:2]
    with torch.no_grad():
        z = {k: v.numpy() for k, v in R.docx_forward(sd, torch.cat([_restated_input(p, *CHAIN_RES) for p in pgs])).items()}
    # the golden generator's margin check on these pages first: every decision settled by more than 4 x the sigmoid's rounding
    xs = torch.from_numpy(np.concatenate([z["hm"].reshape(-1), z["hm_sub"].reshape(-1)]))
    bound = 4.0 * float((torch.sigmoid(xs).double() - torch.sigmoid(xs.double())).abs().max())
    for i in range(3):
        why = R.chain_margins(z, hw, i, score_bound=bound)
        assert why is None, (i, why)
    print(f"docxlayout chain: sigmoid bound {bound:.2e}; the restatement's decisions hold for head maps within "
          f"{[f'{R.chain_headroom(z, hw, i):.1e}' for i in range(3)]} of max|head| per page")
    want = [R.page_chain(z, hw, i) for i in range(3)]
    assert min(len(w) for w in want) >= 1, [len(w) for w in want]
    eng = HipEngine(0)
    try:
        eng.set_precision(L.PT_PRECISION_BF16X3)
        eng.load_weights(L.PT_MODEL_DOCX_DLA34, pack_docxlayout_dla34(sd))
        cfg = DocXLayoutConfig()
        cfg.resolution = CHAIN_RES
        st = DocXLayoutStage(eng, cfg, micro_batch=2)      # 3 pages: micro-batches of 2 + 1 into one decode launch
        dev = torch.from_numpy(np.stack(pgs)).cuda()
        got = st(dev)
        print(f"docxlayout chain: regions per page {[len(w) for w in want]}, labels {sorted({r['label'] for w in want for r in w})}")
        _same_layout(got, want)
        # the same pages with the network taken out of the comparison: the restatement's decode and host chain on the engine's own head maps give
        # the stage's lists exactly, whatever the margins above
        x = eng.docx_preprocess(dev, st._tables(3, *hw), *CHAIN_RES)
        hd = eng.docx_forward_net(x)
        torch.cuda.synchronize()
        zh = {k: hd[k].cpu()[..., :c].permute(0, 3, 1, 2).contiguous().numpy() for k, c in R.HEADS.items()}
        _same_layout(got, [R.page_chain(zh, hw, i) for i in range(3)])
        # eager call = two forwards in flight (two landing buffers, and a landing= key of its own)
        a, b = dev[:2].contiguous(), dev[1:].contiguous()
        na, ta = st.forward(a)
        nb, tb = st.forward(b)
        nc, tc = st.forward(a, landing="second")
        assert ta[1][1].data_ptr() != tb[1][1].data_ptr() and tc[1][1].data_ptr() not in (ta[1][1].data_ptr(), tb[1][1].data_ptr())
        _same_layout(st.finish(na, ta, hw), want[:2])
        _same_layout(st.finish(nb, tb, hw), want[1:])
        _same_layout(st.finish(nc, tc, hw), want[:2])
    finally:
        eng.close()


def test_task_doors(ckpt, pages, tmp_path):
    import PIL.Image
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    task = OcrLayoutTask(model="DocXLayout", task_path=ckpt)
    try:
        assert type(task._stage) is DocXLayoutStage and task.model_provider == "model_scope" and task._stage.config.resolution == (768, 768)
        dev = torch.from_numpy(np.stack(pages[:2])).to(task._engine._tdev)
        want = task.detect_pages(dev)
        assert all(5 <= len(w) <= 100 for w in want), [len(w) for w in want]
        assert all(set(r) == {"bbox", "label", "score", "category_id"} and r["bbox"].shape == (4,) for w in want for r in w)
        assert any(r["label"] == "table" for w in want for r in w)
        _same_layout(task._stage(dev), want)
        res = task(pages[1])                                    # the reference-shaped door: an RGB ndarray
        assert isinstance(res, list) and len(res) == 1
        _same_layout(res, [want[1]])
        f = tmp_path / "page.png"
        PIL.Image.fromarray(pages[1]).save(str(f))
        _same_layout(task([str(f), pages[0]]), [want[1], want[0]])      # a PNG file and an array, one batch per image
        # the file form of task_path, on the same engine
        one = tmp_path / "docx.pth"
        torch.save(docxlayout_dla34_state_dict(seed=0), str(one))
        t2 = OcrLayoutTask(model="DocXLayout", task_path=str(one), engine=task._engine)
        _same_layout(t2.detect_pages(dev), want)
        with pytest.raises(RuntimeError, match="task_path"):
            OcrLayoutTask(model="DocXLayout", synthetic_seed=0, engine=task._engine)
    finally:
        task._engine.close()


def _text_detector(p):
    """bench.py's detector on the pipeline's engine (tests/test_gpu_onnx_layout_pipeline.py): the boxes are the pages' lines"""
    from pdf_table_amd.det_stage import DetConfig
    from pdf_table_amd.synth_weights import db_resnet18_state_dict
    from pdf_table_amd.weights import pack_db_resnet18
    p.engine.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=p.engine.weight_fmt))
    p.text_detector._stage.cfg = DetConfig(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5).resolved()
    return p


def _same(ra, rb):
    assert len(ra) == len(rb)
    for a, b in zip(ra, rb):
        _same_layout([a.layout_result], [b.layout_result])
        assert np.array_equal(a.det_result, b.det_result)
        assert [e["text"] for e in a.ocr_result] == [e["text"] for e in b.ocr_result]
        assert len(a.table_structure_result) == len(b.table_structure_result)
        for ta, tb in zip(a.table_structure_result, b.table_structure_result):
            if ta is None or tb is None:
                assert ta is None and tb is None
                continue
            assert np.array_equal(ta["polygons"], tb["polygons"]) and np.array_equal(ta["logi"], tb["logi"])


def _picodet_results(pages):
    from pdf_table_amd.layout_stage import LayoutStage
    from pdf_table_amd.pipeline import OcrTablePipeline
    p = _text_detector(OcrTablePipeline(synthetic_seed=0, layout=True))
    try:
        assert type(p.layout_task._stage) is LayoutStage
        return p.predict(pages[:2])
    finally:
        p.engine.close()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_pipeline_predict_stream_and_tables(ckpt, pages, precision):
    from pdf_table_amd.pipeline import OcrTablePipeline
    pico_before = _picodet_results(pages) if precision == "bf16" else None
    p = _text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path=ckpt, table_structure=True,
                                        precision=precision))
    try:
        assert type(p.layout_task._stage) is DocXLayoutStage and p.layout_task.synthetic_seed is None and p.text_detector.synthetic_seed == 0
        batches = [[pages[0], pages[1]], [pages[1], pages[2]], [pages[2], pages[0]]]
        want = [p.predict(b) for b in batches]
        direct = [p.layout_task._stage(torch.from_numpy(np.stack(b)).to(p.engine._tdev)) for b in batches]
        for w, d in zip(want, direct):
            _same_layout([r.layout_result for r in w], d)
        assert all(len(r.layout_result) >= 5 for w in want for r in w)
        # the tables the Lore stage gets are this layout's "table" regions: as many results as regions that leave a crop, and the same
        # results when those regions are handed in as table_boxes
        tb = p._layout_table_boxes(direct[0])
        kept = p._drop_empty_crops(tb, pages[0].shape[:2])
        assert sum(len(k) for k in kept) >= 1
        assert [len(r.table_structure_result) for r in want[0]] == [len(k) for k in kept]
        _same(p.predict(batches[0], table_boxes=kept), want[0])
        got = list(p.predict_stream(batches))
        assert len(got) == 3
        for g, w in zip(got, want):
            _same(g, w)
        print(f"docxlayout pipeline {precision}: regions per page {[len(r.layout_result) for r in want[0]]}, table crops {[len(k) for k in kept]}")
        if precision == "fp32":      # printed only: how far the 16-bit default is from the pair mode on these pages
            q = OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path=ckpt)
            try:
                lo = q.layout_task.detect_pages(torch.from_numpy(np.stack(batches[0])).to(q.engine._tdev))
            finally:
                q.engine.close()
            for i, (a, b) in enumerate(zip(lo, direct[0])):
                same = sum(1 for x in a if any(x["label"] == y["label"] and np.abs(x["bbox"] - y["bbox"]).max() <= 2 for y in b))
                print(f"docxlayout bf16 against fp32, page {i}: {len(a)} / {len(b)} regions, {same} of the bf16 regions within 2 px of an fp32 region")
    finally:
        p.engine.close()
    if pico_before is not None:      # the in-tree PicoDet pipeline, built in the same process, gives what it gave
        after = _picodet_results(pages)
        assert len(after) == len(pico_before)
        for a, b in zip(after, pico_before):
            _same_layout([a.layout_result], [b.layout_result])
            assert np.array_equal(a.det_result, b.det_result)
