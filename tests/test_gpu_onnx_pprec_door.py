"""Recognisers with the geometry of the PP-OCR text-line models end to end through the public doors: ``OcrRecognitionTask(model="PP-OCRv4",
task_path=...)`` on ``SvtrLcnetRecLike`` and ``model="PP-Table"`` on ``MobileV3RecLike`` (tools/onnx_export_pprec.py), and ``HipOnnxSession``:
PPOcrRecPreProcessor kernel -> generic executor (per-axis strides, [1,3] kernels and rectangular pools on csrc/rect_ops.hip) -> CTCLabelDecode.  The
real ``*_rec_infer`` files are not available offline; the graphs come from PyTorch's exporter at width 320 with a dynamic batch, so a line gives
T = 80 (W / 4) and T = 40 (W / 8) tokens where the square stand-in of tests/test_gpu_onnx_crnn_door.py gave W / 64.  Checker: the exported module
in fp32 on the oracle's pre-processing of the same crops.  Seeds and head scales were chosen on the CPU so that the fp32 module alone has at most
one position (of 480 / 240) whose two best logits are closer than 1e-3."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

IMG_W = 320
#        task model     stand-in            seed  head scale  tokens per line
DOORS = {"PP-OCRv4": ("SvtrLcnetRecLike", 3, 6.0, IMG_W // 8), "PP-Table": ("MobileV3RecLike", 2, 3.0, IMG_W // 4)}


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=list(DOORS))
def door(request, tmp_path_factory):
    """model.onnx + dictionary under a directory, the module, the crops, and the module's fp32 logits per oracle mini-batch"""
    import onnx_export as X
    import onnx_export_pprec as P
    from oracle import rec_pp as orp
    from pdf_table_amd.synth_pages import make_page
    name = request.param
    cls, seed, head_scale, T = DOORS[name]
    d = tmp_path_factory.mktemp(name.replace("-", "_").lower())
    chars = [chr(0x61 + i % 26) + str(i // 26) for i in range(95)]
    (d / "en_dict.txt").write_text("\n".join(chars) + "\n", encoding="utf-8")
    m = P.seeded_pprec(getattr(P, cls)(classes=97), seed, head_scale=head_scale)      # blank + 95 entries + space
    (d / "model.onnx").write_bytes(X.torch_export(m, torch.zeros(2, 3, 48, IMG_W), dynamic_batch=True))
    page = make_page(4, 1024)[0]
    crops = [page[100:130, 50:450].copy(), page[300:336, 300:900].copy(), page[500:524, 100:420].copy(), page[620:650, 40:1000].copy(),
             page[700:740, 200:640].copy(), page[40:76, 500:1000].copy()]
    batches = orp.rec_pp_preprocess(crops, rec_image_shape=(3, 48, IMG_W), limited_max_width=IMG_W)
    with torch.no_grad():
        logits = [m.logits(torch.from_numpy(np.ascontiguousarray(b["image"]))).numpy() for b in batches]
    return name, T, d, m, crops, batches, logits


def test_door_fp32_strings(eng, door):
    """precision="fp32" (the executor's bf16x3 mode): the strings of the fp32 module under the same CTC rule, token for token.  Positions where the
    module's two best logits are closer than 1e-3 may be left out (their arg-max is not defined at the mode's 1e-3 tolerance): at most 2 % of the
    positions; the count is printed."""
    from pdf_table_amd.ocr_recognition_task import OcrRecognitionTask
    from pdf_table_amd.rec_postprocess import CTCLabelDecode
    name, T, d, m, crops, batches, logits = door
    task = OcrRecognitionTask(model=name, task_type="en", task_path=str(d), engine=eng, precision="fp32")
    assert task._exec.precision == "bf16x3" and not task._batch1
    assert any(task._exec._is_rect(l) for l in task._exec.layers if l.op == "conv")
    got = task(crops)
    assert isinstance(got, list) and len(got) == len(crops) and all(isinstance(t, str) for t in got)
    ctc = CTCLabelDecode(str(d / "en_dict.txt"), use_space_char=True)
    left_out = positions = 0
    for b, lg in zip(batches, logits):
        assert lg.shape[1:] == (T, 97)
        top2 = np.sort(lg, -1)[..., -2:]
        tie = (top2[..., 1] - top2[..., 0]) < 1e-3
        left_out += int(tie.sum())
        positions += tie.size
        p = torch.softmax(torch.from_numpy(lg), -1).numpy()
        want = ctc.decode_ids(p.argmax(-1), p.max(-1))
        ids_e = None
        for i, (text, _) in enumerate(want):
            k = int(b["indices"][b["batch_beg_img_no"] + i])
            assert len(text) >= 2                                       # the seeded head does emit characters
            if not tie[i].any():
                assert got[k] == text, (k, got[k], text)
            else:                                                       # a line with a left-out position: compare the others id by id
                if ids_e is None:
                    ids_e = task._exec.run(b["image"])[0].argmax(-1)
                keep = ~tie[i]
                assert np.array_equal(ids_e[i][keep], lg[i].argmax(-1)[keep])
    print(f"{name} door, precision='fp32': {len(crops)} lines, {positions} positions, {left_out} left out as module ties (< 1e-3 between the two best logits)")
    assert left_out <= 0.02 * positions


def test_door_bf16_shapes(eng, door):
    """bf16: every line returns a string, and the ids have the recogniser's own token count -- W / 4 for the mobile geometry, W / 8 for the SVTR one"""
    from pdf_table_amd.ocr_recognition_task import OcrRecognitionTask
    name, T, d, m, crops, batches, logits = door
    task = OcrRecognitionTask(model=name, task_type="en", task_path=str(d), engine=eng)
    assert task._exec.precision == "bf16"
    got = task(crops)
    assert len(got) == len(crops) and all(isinstance(t, str) for t in got)
    same = n = 0
    for b, lg in zip(batches, logits):
        ids = task._exec.run(b["image"])[0].argmax(-1)
        assert ids.shape == (b["image"].shape[0], T) and T == {"PP-Table": 80, "PP-OCRv4": 40}[name]
        same += int((ids == lg.argmax(-1)).sum())
        n += ids.size
    print(f"{name} door, bf16: arg-max equal to the fp32 module on {100 * same / n:.1f} % of {n} positions")


def test_onnx_session_returns_the_softmax(eng, door):
    from pdf_table_amd.onnx_import import HipOnnxSession
    name, T, d, m, crops, batches, logits = door
    sess = HipOnnxSession(str(d / "model.onnx"), engine=eng)
    assert sess.arch == "generic" and sess.get_providers() == ["HipExecutionProvider"]
    img = batches[0]["image"]
    (out,) = sess.run(None, {sess.get_inputs()[0].name: img})
    with torch.no_grad():
        want = m(torch.from_numpy(np.ascontiguousarray(img))).numpy()
    assert out.shape == want.shape == (img.shape[0], T, 97) and out.dtype == np.float32
    assert np.abs(out.sum(-1) - 1.0).max() <= 1e-4                         # a final Softmax stays fp32
    assert np.abs(out - want).max() <= 4e-2 * float(np.abs(want).max()) + 1e-3
