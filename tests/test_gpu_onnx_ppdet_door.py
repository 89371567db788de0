"""The PP-OCRv4 mobile stand-ins of tools/onnx_export_ppdet.py through the product doors: ``OcrDetectionTask(model="db_pp", task_path=...)`` on
``LcnetV3DetLike`` -- pt_det_preprocess -> generic executor (LearnableAffineBlocks folded or on pt_op_affine_act, the DB head's tail layer by layer or,
with ``fused_head=True``, as one pt_op_db_tail launch) -> bitmap / boxes -- and ``OcrRecognitionTask(model="PP-OCRv4", task_path=...)`` on
``LcnetV3RecLike``.  The real ``*_infer`` files are not available offline: these are seeded modules with the models' layer geometry.  Checker: the fp32
module on the oracle's pre-processing of the same pixels.

Recogniser seed: chosen on the CPU so that the fp32 module alone leaves out no more than the 2 % cap (positions whose two best logits are closer than
1e-3): seed 3 with head scale 6.0 has 0 such positions of 240 on these crops."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

IMG_W = 320
REC_SEED, REC_HEAD_SCALE, REC_TIES = 3, 6.0, 0        # ties: positions of the fp32 module with a top-2 margin below 1e-3 (of 240)


DET_SEED, DET_BOX_THRESH, DET_BOXES_ORACLE = 5, 0.2, 133      # boxes the CPU oracle (oracle/db_post.py) finds on the fp32 module's map of the test page


@pytest.fixture(scope="module")
def det_door(tmp_path_factory):
    """a directory with model.onnx, a synthetic page and the module's fp32 probability map on the oracle's pre-processed pixels.

    The stand-in is seeded with ``blob_map=True`` (tools/onnx_export_ppdet.py: smooth up-sampling in the head, the two coarse FPN levels only, centred
    logits) and scaled on this page, so that its map is made of regions the box stage can work on -- a plainly seeded head gives pixel noise without one
    component of 16 pixels, and the door returned no box.  Seed and box threshold were chosen on the CPU from the fp32 module and the oracle's own
    post-processing alone: seed 5 puts 12.9 % of the page above thresh = 0.3 in 679 components (below the 1000-candidate cap), and with
    box_thresh = 0.2 (the mean probability inside a box; these regions are faint, the default 0.6 keeps none) the oracle returns 133 boxes."""
    import onnx_export_ppdet as D
    from oracle import db_post, db_pre
    from pdf_table_amd.synth_pages import make_page
    page = make_page(2)[0][:480, :640].copy()
    chw, _ = db_pre.preprocess_db_pp(page)
    pix = torch.from_numpy(np.ascontiguousarray(chw))[None]
    m = D.seeded_ppdet(D.LcnetV3DetLike(), DET_SEED, example=pix, blob_map=True)
    d = tmp_path_factory.mktemp("ppocrv4_det")
    (d / "model.onnx").write_bytes(D.torch_export(m, torch.zeros(1, 3, 64, 64)))
    with torch.no_grad():
        want = m(pix)[:, 0].numpy()
    ref_boxes, _ = db_post.boxes_from_bitmap(want[0], want[0] > 0.3, page.shape[1], page.shape[0], DET_BOX_THRESH, 1.5)
    assert len(ref_boxes) == DET_BOXES_ORACLE
    return d, page, want


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_detector_door(det_door, precision):
    """The probability map through the task against the fp32 module, with the layered and with the fused head, and the boxes in the reference's format
    -- [n, 8] corner coordinates in source pixels, more than none.

    precision="fp32" holds the executor's 1e-3 contract; the two heads then agree to about 1e-5, and they must return the same number of boxes with
    corners within 1 px (measured: 133 and 133, the oracle's count, largest corner difference 0).
    precision="fp16" (the reference's own arithmetic): the 6e-3 that test_detection_task_route_in_the_tolerance_and_half_modes asks of the 14-layer
    FpnLike does not hold for this 116-layer graph (measured 1.0e-2 with either head), so the row uses the bound the 16-bit modes have for this graph
    in tests/test_gpu_onnx_ppdet.py, quoted from test_fpn_like_detector: 4e-2 * scale + 1e-3.  In this mode the layered head rounds the probability
    and the intermediate to 11 bits and the fused one does not, so pixels on the threshold fall either way (measured: 131 and 134 boxes): the counts
    are printed and both must be non-empty, not equal."""
    from pdf_table_amd import lib as L
    from pdf_table_amd.ocr_detection_task import OcrDetectionTask
    d, page, want = det_door
    tol = 1e-3 if precision == "fp32" else 4e-2 * float(np.abs(want).max()) + 1e-3
    boxes, errs = {}, {}
    for fused in (False, True):
        task = OcrDetectionTask(model="db_pp", task_path=str(d), thresh=0.3, box_thresh=DET_BOX_THRESH, precision=precision, fused_head=fused)
        try:
            assert task._engine.precision == {"fp32": L.PT_PRECISION_BF16X3, "fp16": L.PT_PRECISION_F16}[precision]
            prob, _, _ = task._stage.forward(torch.from_numpy(page[None]).cuda())
            got = prob.cpu().numpy()
            assert got.shape == want.shape
            errs[fused] = float(np.abs(got - want).max())
            print(f"LcnetV3DetLike through OcrDetectionTask(precision={precision!r}, fused_head={fused}): max|dprob| = {errs[fused]:.3e} (bound {tol:.1e}); "
                  f"module map: {100 * float((want > 0.3).mean()):.1f} % above 0.3")
            out = task(page)
            assert len(out) == 1 and out[0].ndim == 2 and out[0].shape[1] == 8
            boxes[fused] = np.asarray(out[0], np.float64)
        finally:
            task._engine.close()
    n0, n1 = len(boxes[False]), len(boxes[True])
    worst = float(np.abs(boxes[False] - boxes[True]).max()) if n0 == n1 and n0 else float("nan")
    print(f"boxes [{precision}]: {n0} layered, {n1} fused (the CPU oracle on the fp32 module's map: {DET_BOXES_ORACLE}); largest corner difference {worst} px")
    assert errs[False] <= tol and errs[True] <= tol
    assert n0 > 0 and n1 > 0
    if precision == "fp32":
        assert n0 == n1 and worst <= 1.0
    for b in boxes.values():
        assert float(b.min()) >= 0 and float(b[:, 0::2].max()) <= page.shape[1] and float(b[:, 1::2].max()) <= page.shape[0]


@pytest.fixture(scope="module")
def rec_door(tmp_path_factory):
    import onnx_export_ppdet as D
    from oracle import rec_pp as orp
    from pdf_table_amd.synth_pages import make_page
    d = tmp_path_factory.mktemp("ppocrv4_rec")
    chars = [chr(0x61 + i % 26) + str(i // 26) for i in range(95)]
    (d / "en_dict.txt").write_text("\n".join(chars) + "\n", encoding="utf-8")
    m = D.seeded_ppdet(D.LcnetV3RecLike(classes=97), REC_SEED, head_scale=REC_HEAD_SCALE)       # blank + 95 entries + space
    (d / "model.onnx").write_bytes(D.torch_export(m, torch.zeros(2, 3, 48, IMG_W), dynamic_batch=True))
    page = make_page(4, 1024)[0]
    crops = [page[100:130, 50:450].copy(), page[300:336, 300:900].copy(), page[500:524, 100:420].copy(), page[620:650, 40:1000].copy(),
             page[700:740, 200:640].copy(), page[40:76, 500:1000].copy()]
    batches = orp.rec_pp_preprocess(crops, rec_image_shape=(3, 48, IMG_W), limited_max_width=IMG_W)
    with torch.no_grad():
        logits = [m.logits(torch.from_numpy(np.ascontiguousarray(b["image"]))).numpy() for b in batches]
    return d, crops, batches, logits


def test_recogniser_door_fp32_strings(rec_door):
    """precision="fp32": the strings of the fp32 module under the same CTC rule.  Positions whose two best logits are closer than 1e-3 in the module may
    be left out, at most 2 % of them; the seed was chosen on the CPU so that the module stays inside the cap (REC_TIES of 240, asserted)."""
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.ocr_recognition_task import OcrRecognitionTask
    from pdf_table_amd.rec_postprocess import CTCLabelDecode
    d, crops, batches, logits = rec_door
    eng = HipEngine(0)
    try:
        task = OcrRecognitionTask(model="PP-OCRv4", task_type="en", task_path=str(d), engine=eng, precision="fp32")
        assert task._exec.precision == "bf16x3"
        assert sum(1 for l in task._exec.layers if l.attrs.get("affine_folded")) == 28 and any(l.op == "affine" for l in task._exec.layers)
        got = task(crops)
        assert isinstance(got, list) and len(got) == len(crops) and all(isinstance(t, str) for t in got)
        ctc = CTCLabelDecode(str(d / "en_dict.txt"), use_space_char=True)
        left_out = positions = 0
        for b, lg in zip(batches, logits):
            assert lg.shape[1:] == (IMG_W // 8, 97)
            top2 = np.sort(lg, -1)[..., -2:]
            tie = (top2[..., 1] - top2[..., 0]) < 1e-3
            left_out += int(tie.sum())
            positions += tie.size
            p = torch.softmax(torch.from_numpy(lg), -1).numpy()
            want = ctc.decode_ids(p.argmax(-1), p.max(-1))
            ids_e = None
            for i, (text, _) in enumerate(want):
                k = int(b["indices"][b["batch_beg_img_no"] + i])
                if not tie[i].any():
                    assert got[k] == text, (k, got[k], text)
                else:                                                   # a line with a left-out position: compare the others id by id
                    if ids_e is None:
                        ids_e = task._exec.run(b["image"])[0].argmax(-1)
                    keep = ~tie[i]
                    assert np.array_equal(ids_e[i][keep], lg[i].argmax(-1)[keep])
        print(f"PP-OCRv4 door on LcnetV3RecLike, precision='fp32': {len(crops)} lines, {positions} positions, {left_out} left out as module ties")
        assert positions == 240 and left_out == REC_TIES and left_out <= 0.02 * positions
    finally:
        eng.close()
