"""pt_cls_forward_lines_direct -- the text-line classifier of predict_stream(orientation_vote=True): crop, resize and normalise in one kernel
(cls_line_resize_norm_kernel) and the network in an arena of its own -- gives bit for bit the logits of pt_cls_forward_lines (rec_warp_kernel ->
cls_desc_from_lines_kernel -> cls_resize_norm_kernel, PT_ARENA_LAYOUT) in bf16, f16 and BF16X3, and may run beside the recogniser and the
layout net on other streams."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.rec_stage import build_lines
from pdf_table_amd.synth_pages import make_page

pytestmark = pytest.mark.gpu

SIZE = (80, 160)


def _quad(cx, cy, w, h, ang):
    c, s = np.cos(ang), np.sin(ang)
    pts = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
    return (pts @ np.array([[c, s], [-s, c]]) + [cx, cy]).reshape(8)


def _lines(n_pages, size, rng, n_random):
    """hand-picked lines (rotated, partly outside the page, crops wider / narrower than 160 and taller / shorter than 80, 1-px crops) plus
    n_random random ones"""
    per = [[] for _ in range(n_pages)]
    fixed = [(200, 100, 300, 20, 0.0), (300, 400, 90, 140, 0.3), (500, 500, 600, 40, -0.2), (20, 30, 120, 60, 0.0),        # partly outside (left / top)
             (size - 10, size - 5, 200, 30, 0.1), (400, 300, 160, 80, 0.0), (250, 700, 50, 300, 1.2), (600, 200, 40, 12, 2.9)]
    for i, (cx, cy, w, h, a) in enumerate(fixed):
        per[i % n_pages].append(_quad(cx, cy, w, h, a))
    for _ in range(n_random):
        per[int(rng.integers(n_pages))].append(_quad(rng.uniform(-20, size + 20), rng.uniform(-20, size + 20), rng.uniform(8, 500),
                                                     rng.uniform(6, 120), rng.uniform(-np.pi, np.pi)))
    lines = build_lines([np.array(q, np.float32).reshape(-1, 8) for q in per])
    # 1-px crops: one pixel wide, one pixel high, and one by one (the records' matrices stay valid)
    lines["crop_w"][0], lines["crop_h"][1] = 1, 1
    lines["crop_w"][2], lines["crop_h"][2] = 1, 1
    assert (lines["crop_w"] > 0).all() and (lines["crop_h"] > 0).all()
    assert (lines["crop_w"] > 160).any() and (lines["crop_w"] < 160).any() and (lines["crop_h"] > 80).any() and (lines["crop_h"] < 80).any()
    return lines


def _engine(precision):
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    eng = HipEngine(0)
    eng.set_precision(precision)
    eng.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True), fmt=eng.weight_fmt))
    return eng


@pytest.mark.parametrize("precision", [L.PT_PRECISION_BF16, L.PT_PRECISION_F16, L.PT_PRECISION_BF16X3])
def test_direct_equals_crop_buffer_chain(precision):
    eng = _engine(precision)
    pages = torch.from_numpy(np.stack([make_page(i)[0] for i in range(2)])).cuda()
    rng = np.random.default_rng(3)
    for n_random in (40, 1100):          # the second call needs two micro-batches of PT_CLS_MICROBATCH (default 1024)
        lines = _lines(2, 1024, rng, n_random)
        ref = eng.cls_forward_lines(pages, lines, SIZE, 0, True)
        got = eng.cls_forward_lines_direct(pages, lines, SIZE, 0, True)
        torch.cuda.synchronize()
        assert got.shape == ref.shape == (len(lines), 2)
        assert torch.isfinite(ref).all()
        assert torch.equal(got, ref), (precision, n_random, int((got != ref).any(1).sum()))
    eng.close()


def test_direct_beside_recogniser_and_layout():
    """the direct classifier on one stream, the recogniser on a second and the layout net on a third: the serial results"""
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    p = OcrTablePipeline(device=0, synthetic_seed=0, layout=True, text_orientation=True)
    eng = p.engine
    eng.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True), fmt=eng.weight_fmt))
    eng.set_lstm_cluster(False)          # the recogniser shares the GPU (pt_engine_set_lstm_cluster)
    pages = torch.from_numpy(np.stack([make_page(i)[0] for i in range(4)])).cuda()
    lines = _lines(4, 1024, np.random.default_rng(5), 1500)
    rec_lines = build_lines(p.text_detector._stage(pages))

    def run():
        c = eng.cls_forward_lines_direct(pages, lines, SIZE, 0, True)
        r, _ = eng.rec_forward(pages, rec_lines, want_maxlogit=False)
        n, cand = eng.layout_forward(pages, 800, 608, 5)
        return c, r, n, cand

    ref = [t.clone() for t in run()]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    main = torch.cuda.current_stream()
    for _ in range(3):
        for s in streams:
            s.wait_stream(main)
        with torch.cuda.stream(streams[0]):
            c = eng.cls_forward_lines_direct(pages, lines, SIZE, 0, True)
        with torch.cuda.stream(streams[1]):
            r, _ = eng.rec_forward(pages, rec_lines, want_maxlogit=False)
        with torch.cuda.stream(streams[2]):
            n, cand = eng.layout_forward(pages, 800, 608, 5)
        torch.cuda.synchronize()
        assert torch.equal(c, ref[0])
        assert torch.equal(r, ref[1])
        assert torch.equal(n, ref[2])
        for i in range(n.shape[0]):      # the candidate compaction appends through an atomic counter: the same records, in any order
            k = int(n[i])
            a, b = cand[i, :k].cpu().numpy(), ref[3][i, :k].cpu().numpy()
            assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])])
    eng.close()
