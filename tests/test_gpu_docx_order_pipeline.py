"""device_order=True through the stage, the task and the pipeline: DocXLayoutStage queues pt_op_docx_order behind pt_docx_decode and lands its rows with
the records; with the knob on and off the SAME landed records are read, so the lists are compared dict for dict in every precision.  (The pages' quads
come from a network and are slightly turned: each comparison first asserts the stability rule of tests/docx_order_ref.py on the landed records.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docx_order_ref as O  # noqa: E402
import test_gpu_docxlayout_pipeline as P  # noqa: E402  (helpers: _text_detector, _same, _same_layout)
from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.docxlayout_stage import DocXLayoutConfig, DocXLayoutStage, docx_page_result  # noqa: E402
from pdf_table_amd.synth_weights import docxlayout_dla34_state_dict  # noqa: E402
from pdf_table_amd.weights import pack_docxlayout_dla34  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_RES = (128, 96)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("docx_order")
    torch.save({"state_dict": {"module." + k: v for k, v in docxlayout_dla34_state_dict(seed=0).items()}}, str(d / "pytorch_model.bin"))
    return str(d)


@pytest.fixture(scope="module")
def pages():
    from pdf_table_amd.synth_pages import make_page
    return [make_page(i, 1024)[0] for i in range(3)]


def _parent_finish(stage, n, ticket, org):
    """what finish() did before the knob existed, on the landed records"""
    done, host = ticket
    done.synchronize()
    counts, recs, keep = (h[:n].numpy() for h in host[:3])
    inp_h, inp_w = stage.config.resolution
    out = []
    for i in range(n):
        main, sub = O.kept_rows(counts, recs, keep, i, stage.config.use_nms)
        out.append(docx_page_result(main, sub, (int(org[0]), int(org[1])), (inp_h // 4, inp_w // 4), stage.config))
    return out


def _assert_stable(stage, ticket, n, org):
    counts, recs, keep = (h[:n].numpy() for h in ticket[1][:3])
    inp_h, inp_w = stage.config.resolution
    for i in range(n):
        main, sub = O.kept_rows(counts, recs, keep, i, stage.config.use_nms)
        assert O.page_is_stable(main, sub, org, (inp_h // 4, inp_w // 4), stage.config), f"page {i}: the host chain is not stable on these records"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage_on_equals_off(precision):
    """a seeded checkpoint written to a temporary file, 3 pages of 256 x 192"""
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_pages import make_page
    sd = docxlayout_dla34_state_dict(seed=P.CHAIN_SEED)
    pgs = [np.ascontiguousarray(make_page(i, 1024)[0][100:356, 60:252]) for i in range(3)]
    hw = pgs[0].shape[:2]
    assert hw == (256, 192)
    eng = HipEngine(0)
    try:
        if precision == "fp32":
            eng.set_precision(L.PT_PRECISION_BF16X3)
        eng.load_weights(L.PT_MODEL_DOCX_DLA34, pack_docxlayout_dla34(sd, x3=True, fmt=eng.weight_fmt))
        stages = []
        for on in (False, True):
            cfg = DocXLayoutConfig()
            cfg.resolution = SMALL_RES
            stages.append(DocXLayoutStage(eng, cfg, micro_batch=2, device_order=on))
        off, on = stages
        dev = torch.from_numpy(np.stack(pgs)).cuda()
        n, t_off = off.forward(dev)
        assert len(t_off[1]) == 3                       # knob off: the three tensors the parent lands, nothing else
        want = off.finish(n, t_off, hw)
        P._same_layout(want, _parent_finish(off, n, t_off, hw))
        n, t_on = on.forward(dev)
        assert len(t_on[1]) == 6
        got = on.finish(n, t_on, hw)
        for a, b in zip(t_off[1], t_on[1][:3]):         # the same landed records
            assert torch.equal(a[:n], b[:n])
        _assert_stable(on, t_on, n, hw)
        assert on.last_fallback == [] and off.last_fallback == []
        print(f"docx order stage {precision}: regions per page {[len(w) for w in want]}")
        P._same_layout(got, want)
        P._same_layout(on(dev), want)
        # two forwards in flight and a landing= key of its own, as the pipeline uses them
        a, b = dev[:2].contiguous(), dev[1:].contiguous()
        na, ta = on.forward(a)
        nb, tb = on.forward(b)
        nc, tc = on.forward(a, landing="second")
        P._same_layout(on.finish(na, ta, hw), want[:2])
        P._same_layout(on.finish(nb, tb, hw), want[1:])
        P._same_layout(on.finish(nc, tc, hw), want[:2])
    finally:
        eng.close()


def test_order_records_fallback_on_a_crafted_page():
    """70 sub-fields: the kernel flags the page, order_records() serves it through the host route; a small page beside it is served by the kernel"""
    from pdf_table_amd.engine import HipEngine
    import test_gpu_docx_order as T
    rng = np.random.RandomState(0)
    fields = [(T.box(90 * (k % 8), 45 * (k // 8), 90 * (k % 8) + 80, 45 * (k // 8) + 35), 0.5 + 0.005 * k, k % 2) for k in range(70)]
    inside = [(T.box(90 * (k % 8) + 5, 45 * (k // 8) + 5, 90 * (k % 8) + 60, 45 * (k // 8) + 25), float(np.float32(rng.uniform(0.4, 0.9))), int(rng.randint(0, 11)))
              for k in range(0, 70, 3)]
    big = (T.rows(inside), T.rows(fields))
    small = T.columns_page(5, nf=2, per=4, loose=2)
    eng = HipEngine(0)
    try:
        cfg = DocXLayoutConfig()
        cfg.resolution = (T.PAGE[0], T.PAGE[1])       # head maps of 192 x 192: the x4 map
        stage = DocXLayoutStage(eng, cfg, device_order=True)
        counts, recs, keep = T.pack([big, small], cfg.top_k, junk=False)
        got = stage.order_records(counts, recs, keep, T.PAGE)
        assert stage.last_fallback == [0]
        want = [docx_page_result(*O.kept_rows(counts, recs, keep, i), T.PAGE, T.MAP, cfg) for i in range(2)]
        assert len(want[0]) == len(inside) and len(want[1]) == 10
        P._same_layout(got, want)
    finally:
        eng.close()


def _pipeline(ckpt, on, **kw):
    from pdf_table_amd.pipeline import OcrTablePipeline
    extra = {"layout_device_order": True} if on else {}
    return P._text_detector(OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path=ckpt, **extra, **kw))


def test_pipeline_predict_stream_tables_and_vote(ckpt, pages):
    """one pipeline with the knob, one without, both with the Lore stage and the orientation classifier: predict() == predict_stream() == the stage,
    on == off; the "table" regions feed the Lore stage as before; the vote's second layout pass (landing=) goes through the kernel too"""
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    flipped = np.ascontiguousarray(pages[1][::-1, ::-1])
    batches = [[pages[0], pages[1]], [pages[1], pages[2]]]
    vote_batches = [[pages[0], flipped], [flipped, pages[2]]]
    res = {}
    for on in (False, True):
        p = _pipeline(ckpt, on, table_structure=True, text_orientation=True)
        try:
            p.engine.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True), fmt=p.engine.weight_fmt))
            stage = p.layout_task._stage
            assert type(stage) is DocXLayoutStage and stage.device_order == on
            want = [p.predict(b) for b in batches]
            hw = pages[0].shape[:2]
            for b, w in zip(batches, want):
                dev = torch.from_numpy(np.stack(b)).to(p.engine._tdev)
                n, ticket = stage.forward(dev)
                assert len(ticket[1]) == (6 if on else 3)      # knob off: no new tensor lands
                direct = stage.finish(n, ticket, hw)
                if on:
                    _assert_stable(stage, ticket, n, hw)
                    assert stage.last_fallback == []
                else:
                    P._same_layout(direct, _parent_finish(stage, n, ticket, hw))
                P._same_layout([r.layout_result for r in w], direct)
            assert all(len(r.layout_result) >= 5 for w in want for r in w)
            assert sum(len(r.table_structure_result) for w in want for r in w) >= 1
            got = list(p.predict_stream(batches, orientation_vote=True))      # a pipeline with the orientation task streams only with the vote
            assert len(got) == len(batches)
            for g, w in zip(got, want):
                P._same(g, w)
            vote_want = [p.predict(b) for b in vote_batches]
            assert [r.rotated_180 for w in vote_want for r in w] == [False, True, True, False]
            vote_got = list(p.predict_stream(vote_batches, orientation_vote=True))
            for g, w in zip(vote_got, vote_want):
                P._same(g, w)
            res[on] = (want, vote_want)
        finally:
            p.engine.close()
    for a, b in zip(res[True], res[False]):
        for ga, gb in zip(a, b):
            P._same(ga, gb)


def test_task_door_with_the_knob(ckpt, pages):
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    task = OcrLayoutTask(model="DocXLayout", task_path=ckpt, device_order=True)
    try:
        assert task._stage.device_order
        dev = torch.from_numpy(np.stack(pages[:2])).to(task._engine._tdev)
        got = task.detect_pages(dev)
        door = OcrLayoutTask(model="DocXLayout", task_path=ckpt, engine=task._engine)      # the knob is per task
        assert not door._stage.device_order
        P._same_layout(got, door.detect_pages(dev))
        P._same_layout(task(pages[1]), [got[1]])
    finally:
        task._engine.close()
