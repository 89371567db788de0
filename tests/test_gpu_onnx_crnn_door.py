"""A CRNN-type PP-OCR recogniser end to end through the public doors (``OcrRecognitionTask(model="PP-Table", task_path=...)`` and
``HipOnnxSession``): PPOcrRecPreProcessor kernel -> generic executor (conv backbone, two BiLSTMs of 48 units on pt_op_lstm, CTC head with its
Softmax) -> CTCLabelDecode.  The real ``en_ppocr_mobile_v2.0_table_rec`` file is not available offline; the graph is ``MobileCrnn``
(tools/onnx_export_rnn.py) from PyTorch's exporter with a dynamic batch, so the zero initial states arrive as a Shape -> Expand chain.
Checker: the exported module in fp32 on the oracle's pre-processing of the same crops."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

IMG_W = 640          # the export's width: the pre-processor pads every mini-batch to it (PaddleOCR's static rec_image_shape) -> T = 10 per line


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def door(tmp_path_factory):
    """model.onnx + dictionary under a directory, the module, the crops, and the module's fp32 logits per oracle mini-batch"""
    import onnx_export as X
    import onnx_export_rnn as XR
    from oracle import rec_pp as orp
    from pdf_table_amd.synth_pages import make_page
    d = tmp_path_factory.mktemp("pp_table")
    chars = [chr(0x61 + i % 26) + str(i // 26) for i in range(95)]
    (d / "en_dict.txt").write_text("\n".join(chars) + "\n", encoding="utf-8")
    m = XR.seeded_rnn(XR.MobileCrnn(classes=97), 8)                       # blank + 95 entries + space
    with torch.no_grad():
        m.head.weight *= 4.0                                              # a random head made decisive: fewer near-ties between its two best classes
    (d / "model.onnx").write_bytes(X.torch_export(m, torch.zeros(2, 3, 48, IMG_W), dynamic_batch=True))
    page = make_page(4, 1024)[0]
    crops = [page[100:130, 50:450].copy(), page[300:336, 300:900].copy(), page[500:524, 100:420].copy(), page[620:650, 40:1000].copy(),
             page[700:740, 200:640].copy(), page[40:76, 500:1000].copy()]
    batches = orp.rec_pp_preprocess(crops, rec_image_shape=(3, 48, IMG_W), limited_max_width=IMG_W)
    with torch.no_grad():
        logits = [m.logits(torch.from_numpy(np.ascontiguousarray(b["image"]))).numpy() for b in batches]
    return d, m, crops, batches, logits


def _emulate_bf16(m, img):
    """MobileCrnn in the engine's bf16 arithmetic on the CPU: BatchNorm folded in float64, 16-bit operands, fp32 sums, every stored activation
    rounded once (convolution + bias + activation, pooling exact), the recurrent layers and the head through onnx_lstm_ref -> logits [B, T, classes]"""
    import onnx_export_rnn as XR
    import onnx_lstm_ref as LR
    x = LR.round_to(img, "bf16")
    for blk in (m.s1, m.s2, m.s3, m.s4):
        conv, bn, act = blk[0], blk[1], blk[2]
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = LR.round_to((conv.weight.double() * s.reshape(-1, 1, 1, 1)).float(), "bf16")
        b = ((0.0 - bn.running_mean.double()) * s + bn.bias.double()).float()
        x = LR.round_to(act(torch.nn.functional.conv2d(x, w, b, 2, 1)), "bf16")
    x = m.pool(m.pool(x))
    xs = x.squeeze(2).permute(2, 0, 1).detach().numpy()
    y = LR.stack_emulated(xs, [XR.onnx_lstm_params(m.rnn1), XR.onnx_lstm_params(m.rnn2)], (m.head.weight.detach().numpy(), m.head.bias.detach().numpy()), "bf16")
    return y.transpose(1, 0, 2)


def test_pp_table_door_fp32_strings(eng, door):
    """precision="fp32" (the executor's bf16x3 mode): the strings of the fp32 module under the same CTC rule, token for token.  Positions where the
    module's two best logits are closer than 1e-3 may be left out (their arg-max is not defined at the mode's 1e-3 tolerance): at most 2 % of the
    positions; the count is printed -- 0 of 60 on the committed seed."""
    from pdf_table_amd.ocr_recognition_task import OcrRecognitionTask
    from pdf_table_amd.rec_postprocess import CTCLabelDecode
    d, m, crops, batches, logits = door
    task = OcrRecognitionTask(model="PP-Table", task_type="en", task_path=str(d), engine=eng, precision="fp32")
    assert task._exec.precision == "bf16x3" and [l.op for l in task._exec.layers].count("lstm") == 2 and not task._batch1
    got = task(crops)
    assert isinstance(got, list) and len(got) == len(crops) and all(isinstance(t, str) for t in got)
    ctc = CTCLabelDecode(str(d / "en_dict.txt"), use_space_char=True)
    left_out = positions = 0
    for b, lg in zip(batches, logits):
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
    print(f"PP-Table door, precision='fp32': {len(crops)} lines, {positions} positions, {left_out} left out as module ties (< 1e-3 between the two best logits)")
    assert left_out <= 0.02 * positions


def test_pp_table_door_bf16_argmax_share(eng, door):
    """bf16: the arg-max ids agree with the fp32 module on at least the share the CPU emulation of the same arithmetic reaches on these lines,
    minus 2 points"""
    from pdf_table_amd.ocr_recognition_task import OcrRecognitionTask
    d, m, crops, batches, logits = door
    task = OcrRecognitionTask(model="PP-Table", task_type="en", task_path=str(d), engine=eng)
    assert task._exec.precision == "bf16"
    assert len(task(crops)) == len(crops)
    same_e = same_c = n = 0
    for b, lg in zip(batches, logits):
        want = lg.argmax(-1)
        with torch.no_grad():
            emu = _emulate_bf16(m, b["image"]).argmax(-1)
        ids = task._exec.run(b["image"])[0].argmax(-1)
        assert ids.shape == want.shape == emu.shape
        same_e += int((ids == want).sum())
        same_c += int((emu == want).sum())
        n += want.size
    print(f"PP-Table door, bf16: arg-max equal to the fp32 module on {100 * same_e / n:.1f} % of {n} positions (CPU emulation of bf16: {100 * same_c / n:.1f} %)")
    assert same_e / n >= same_c / n - 0.02


def test_onnx_session_returns_the_softmax(eng, door):
    from pdf_table_amd.onnx_import import HipOnnxSession
    d, m, crops, batches, logits = door
    sess = HipOnnxSession(str(d / "model.onnx"), engine=eng)
    assert sess.arch == "generic" and sess.get_providers() == ["HipExecutionProvider"]
    img = batches[0]["image"]
    (out,) = sess.run(None, {sess.get_inputs()[0].name: img})
    with torch.no_grad():
        want = m(torch.from_numpy(np.ascontiguousarray(img))).numpy()
    assert out.shape == want.shape == (img.shape[0], IMG_W // 64, 97) and out.dtype == np.float32
    assert np.abs(out.sum(-1) - 1.0).max() <= 1e-4                         # a final Softmax stays fp32
