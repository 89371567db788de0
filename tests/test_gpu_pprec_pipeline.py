"""The PP-OCR ONNX recognisers through the product API: ``OcrTablePipeline(recognizer="PP-OCRv4" | "PP-Table", rec_task_path=...)`` -- PPRecStage
(pdf_table_amd/pprec_stage.py): PPOcrRecPreProcessor.lines over the resident pages, the generic executor with its planned CTC tail
(pt_op_ctc_greedy), CTCLabelDecode.  Stand-ins as in tests/test_gpu_onnx_pprec_door.py (SvtrLcnetRecLike / MobileV3RecLike, 97 classes, dynamic
batch, width 320, the same seeds and head scales; the real ``*_rec_infer`` files are not available offline).  Pages: two generator pages of
1024 x 1024; the detector is the seeded DB-ResNet18 with the text channel (bench.py's), whose boxes are the generator's lines.

The composition check chains the parts that have tests of their own by hand on the same boxes -- ``task._pp.lines`` -> the layered executor walk
(ctc_tail=False) -> ``values()`` -> np.argmax / max on the host -> ``CTCLabelDecode.decode_ids`` -- and asks for the same strings, line for line.
Scores: tests/test_gpu_ctc_ops.py measured the layered route's largest relative error of a token's probability against float64 at 5.824e-7
(the fused kernel's: 4.212e-7) and bounds the fused kernel by 4 x the layered figure; a score is a mean of such probabilities, so the two routes'
scores are asked to agree within 4 x 5.824e-7 relative."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

IMG_W = 320
STANDINS = {"PP-OCRv4": ("SvtrLcnetRecLike", 3, 6.0), "PP-Table": ("MobileV3RecLike", 2, 3.0)}
SCORE_REL = 4 * 5.824e-7


@pytest.fixture(scope="module")
def standins(tmp_path_factory):
    """per recogniser a directory with model.onnx and the dictionary; for the SVTR stand-in also its logits (no Softmax) as a second file"""
    import onnx_export as X
    import onnx_export_pprec as P
    out = {}
    for name, (cls, seed, head_scale) in STANDINS.items():
        d = tmp_path_factory.mktemp(name.replace("-", "_").lower())
        chars = [chr(0x61 + i % 26) + str(i // 26) for i in range(95)]
        (d / "en_dict.txt").write_text("\n".join(chars) + "\n", encoding="utf-8")
        m = P.seeded_pprec(getattr(P, cls)(classes=97), seed, head_scale=head_scale)      # blank + 95 entries + space
        (d / "model.onnx").write_bytes(X.torch_export(m, torch.zeros(2, 3, 48, IMG_W), dynamic_batch=True))
        if name == "PP-OCRv4":
            class Logits(torch.nn.Module):
                def __init__(self, net):
                    super().__init__()
                    self.net = net

                def forward(self, x):
                    return self.net.logits(x)
            (d / "logits.onnx").write_bytes(X.torch_export(Logits(m), torch.zeros(2, 3, 48, IMG_W), dynamic_batch=True))
        out[name] = d
    return out


@pytest.fixture(scope="module")
def pages():
    from pdf_table_amd.synth_pages import make_page
    return [make_page(i, 1024)[0] for i in range(2)]


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
def pipes(standins):
    """pipelines made on first use, one per (recogniser, precision, knobs), with predict() of the two pages alongside"""
    from pdf_table_amd.pipeline import OcrTablePipeline
    made = {}

    def get(name, precision="bf16", **kw):
        key = (name, precision, tuple(sorted(kw.items())))
        if key not in made:
            extra = {} if name == "CRNN" else {"rec_task_path": str(standins[name])}
            made[key] = _text_detector(OcrTablePipeline(synthetic_seed=0, recognizer=name, precision=precision, **extra, **kw))
        return made[key]
    yield get
    for p in made.values():
        p.engine.close()


@pytest.mark.parametrize("name", list(STANDINS))
def test_predict_returns_a_string_and_a_score_per_box(pipes, pages, name):
    p = pipes(name)
    from pdf_table_amd.pprec_stage import PPRecStage
    assert isinstance(p.text_recognizer._stage, PPRecStage) and p.text_recognizer._stage.exec.ctc_tail_layer is not None
    res = p.predict(pages)
    assert len(res) == 2 and sum(len(r.det_result) for r in res) >= 20
    for r in res:
        assert len(r.ocr_result) == len(r.det_result)
        for e in r.ocr_result:
            assert isinstance(e["text"], str) and isinstance(e["score"], float) and 0.0 <= e["score"] <= 1.0
    assert sum(bool(e["text"]) for r in res for e in r.ocr_result) >= 20          # the seeded heads do emit characters
    # the task's batched door is the same stage
    texts = p.text_recognizer.recognize_quads(torch.from_numpy(np.stack(pages)).to(p.engine._tdev), [r.det_result for r in res])
    assert texts == [[e["text"] for e in r.ocr_result] for r in res]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(STANDINS))
def test_stage_equals_the_parts_chained_by_hand(pipes, pages, name, precision):
    p = pipes(name, precision)
    task = p.text_recognizer
    assert task._exec.precision == task._exec_tail.precision == {"fp32": "bf16x3", "bf16": "bf16"}[precision]
    assert task._exec.ctc_tail_layer is None and task._exec_tail.ctc_tail_layer is not None
    res = p.predict(pages)
    boxes = [r.det_result for r in res]
    n = sum(len(b) for b in boxes)
    pages_t = torch.from_numpy(np.stack(pages)).to(p.engine._tdev)
    ex = task._exec
    texts, scores = [None] * n, [None] * n
    for b in task._pp.lines(pages_t, boxes):
        x = b["image"].permute(0, 2, 3, 1).contiguous()
        (a,) = ex.run_device(x if ex.split else x.to(ex.adt), 3)               # the layered walk: fp32 probabilities
        v = ex.values(a).cpu().numpy()
        v = v.reshape(v.shape[0], v.shape[-2], v.shape[-1])
        assert v.shape[1:] == ({"PP-OCRv4": IMG_W // 8, "PP-Table": IMG_W // 4}[name], 97)
        for i, (text, sc) in enumerate(task._ctc.decode_ids(np.argmax(v, -1), v.max(-1))):
            k = int(b["indices"][b["batch_beg_img_no"] + i])
            texts[k], scores[k] = text, float(sc)
    assert all(t is not None for t in texts)                                   # no detected box is degenerate: every line was kept
    got_t = [e["text"] for r in res for e in r.ocr_result]
    got_s = np.array([e["score"] for r in res for e in r.ocr_result])
    assert got_t == texts
    worst = float((np.abs(got_s - np.array(scores)) / np.maximum(np.array(scores), 1e-30)).max())
    print(f"{name} {precision}: {n} lines, {sum(bool(t) for t in texts)} non-empty; largest relative score difference to the layered route {worst:.3e}")
    assert worst <= SCORE_REL


class _FixedBoxes:
    """a detection stage that returns hand-made boxes (for OcrTablePipeline.from_engine)"""

    def __init__(self, per_page):
        self.per_page = per_page

    def forward(self, pages_t, slot=0, early_copy=False):
        return None, None, None

    def boxes(self, prob, bitmap, shape, ev):
        return [np.array(b, dtype=np.float32).reshape(-1, 8) for b in self.per_page]


def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra.det_result, rb.det_result)
        assert [e["text"] for e in ra.ocr_result] == [e["text"] for e in rb.ocr_result]
        assert [e["score"] for e in ra.ocr_result] == [e["score"] for e in rb.ocr_result]
        assert all(np.array_equal(x["bbox"], y["bbox"]) for x, y in zip(ra.ocr_result, rb.ocr_result))


def test_stream_equals_predict(pipes, pages):
    from pdf_table_amd.pipeline import OcrTablePipeline
    p = pipes("PP-OCRv4")
    blank = np.full_like(pages[0], 255)                                        # a page without a box
    b0, b1 = list(pages), [pages[1], blank]
    want0, want1 = p.predict(b0), p.predict(b1)
    assert len(want1[1].det_result) == 0 and want1[1].ocr_result == []
    got = list(p.predict_stream([b0, b1, b0]))
    assert len(got) == 3
    _same(got[0], want0)
    _same(got[1], want1)
    _same(got[2], want0)
    # hand-made boxes through from_engine: a quad of zero width has no crop -> '' with score 0, its neighbours are unaffected
    real = want0[0].det_result[:3]
    flat = [100, 100, 100, 100, 100, 130, 100, 130]
    q = OcrTablePipeline.from_engine(p.engine, _FixedBoxes([np.concatenate([real[:1], np.array([flat], np.float32), real[1:]]), real]),
                                     p.text_recognizer._stage)
    ref = p.text_recognizer._stage(torch.from_numpy(np.stack(pages)).to(p.engine._tdev), [real, real])
    one = q.predict(b0)
    by_text = {tuple(np.round(e["bbox"].reshape(-1), 3)): (e["text"], e["score"]) for e in one[0].ocr_result}
    assert len(one[0].ocr_result) == 4 and ("", 0.0) in by_text.values()
    assert sorted(t for t, _ in by_text.values()) == sorted(ref[0] + [""]) and sorted(e["text"] for e in one[1].ocr_result) == sorted(ref[1])
    streamed = list(q.predict_stream([b0, b0]))
    _same(streamed[0], one)
    _same(streamed[1], one)


def test_executor_tail_falls_back_and_replays(standins):
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.onnx_exec import HipGraphExecutor, _CtcOut
    eng = HipEngine(0)
    try:
        d = standins["PP-OCRv4"]
        x = torch.randn(3, 3, 48, IMG_W, generator=torch.Generator().manual_seed(5))
        # a graph that ends in logits: nothing to plan, the layered route, bit for bit
        plain, tail = HipGraphExecutor(str(d / "logits.onnx"), engine=eng), HipGraphExecutor(str(d / "logits.onnx"), engine=eng, ctc_tail=True)
        assert tail.ctc_tail_layer is None
        (a,), (b,) = plain.run(x), tail.run(x)
        assert a.shape == (3, IMG_W // 8, 97) and np.array_equal(a, b)
        # the Softmax graph: the walk ends in the tail; the captured replay returns the eager walk's ids
        ex = HipGraphExecutor(str(d / "model.onnx"), engine=eng, ctc_tail=True)
        assert ex.ctc_tail_layer is not None
        nhwc = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(eng._tdev)
        (e0,) = ex.run_device(nhwc, 3)
        assert isinstance(e0, _CtcOut) and e0.ids.dtype == torch.int32 and tuple(e0.ids.shape) == tuple(e0.conf.shape) == (3, IMG_W // 8)
        ids0, conf0 = e0.ids.cpu().numpy(), e0.conf.cpu().numpy()
        for _ in range(3):                                                      # eager (remembered), capture, replay
            (g,) = ex.run_device_graphed(nhwc, 3)
            assert np.array_equal(g.ids.cpu().numpy(), ids0) and np.array_equal(g.conf.cpu().numpy(), conf0)
        assert len(ex._graphs) == 1 or os.environ.get("PT_ONNX_GRAPH", "1") == "0"
        # and they are the arg-max of the layered route's probabilities
        (pr,) = HipGraphExecutor(str(d / "model.onnx"), engine=eng).run(x)
        assert np.array_equal(np.argmax(pr, -1), ids0)
        ids_r, conf_r = ex.run(x)                                               # the host API returns the pair
        assert np.array_equal(ids_r, ids0) and np.array_equal(conf_r, conf0)
    finally:
        eng.close()


def test_width_bucket(pipes, pages):
    p = pipes("PP-OCRv4", rec_batch_num=64, rec_width_bucket=32)
    stage = p.text_recognizer._stage
    assert stage.pp.config.rec_batch_num == 64 and stage.pp.config.rec_width_bucket == 32
    res = p.predict(pages)
    n = sum(len(r.det_result) for r in res)
    assert n >= 20 and stage.last_widths and all(w % 32 == 0 and w <= IMG_W for w in stage.last_widths)
    assert len(stage.last_widths) == -(-n // 64)
    assert all(isinstance(e["text"], str) and isinstance(e["score"], float) for r in res for e in r.ocr_result)
    assert sum(bool(e["text"]) for r in res for e in r.ocr_result) >= 20


def test_crnn_pipeline_is_unchanged(pipes, pages):
    from pdf_table_amd.rec_stage import RecStage
    p = pipes("CRNN")
    assert type(p.text_recognizer._stage) is RecStage
    res = p.predict(pages)
    assert sum(len(r.det_result) for r in res) >= 20
    direct = RecStage(p.engine, p.text_recognizer._vocab, recognizer="CRNN")(torch.from_numpy(np.stack(pages)).to(p.engine._tdev),
                                                                             [r.det_result for r in res])
    for r, want in zip(res, direct):
        assert [e["text"] for e in r.ocr_result] == want
        assert all(set(e) == {"index", "text", "bbox"} for e in r.ocr_result)
    for got in p.predict_stream([pages]):
        assert all("score" not in e for r in got for e in r.ocr_result)


def test_static_batch1_export(pages, tmp_path):
    """an export with its batch size baked in as 1 (like the shipped PP-OCR files): the lines of a mini-batch are walked one by one inside one
    captured graph, each walk ending in the tail -- the strings of the layered walk of every line, chained by hand"""
    import onnx_export as X
    from pdf_table_amd.pipeline import OcrTablePipeline
    chars = [chr(0x4E00 + i) for i in range(95)]
    (tmp_path / "ppocr_keys_v1.txt").write_text("\n".join(chars) + "\n", encoding="utf-8")
    (tmp_path / "inference.onnx").write_bytes(X.torch_export(X.seeded(X.SvtrTiny(classes=97), 31), torch.zeros(1, 3, 48, IMG_W)))
    p = _text_detector(OcrTablePipeline(synthetic_seed=0, recognizer="PP-OCRv3", rec_task_path=str(tmp_path)))
    try:
        task = p.text_recognizer
        assert task._batch1 and task._stage.batch1 and task._exec_tail.ctc_tail_layer is not None
        one = pages[:1]
        res = p.predict(one)
        again = p.predict(one)                                                 # captured, then replayed
        boxes = [r.det_result for r in res]
        n = len(boxes[0])
        assert n >= 20
        ex = task._exec
        texts, scores = [None] * n, [None] * n
        for b in task._pp.lines(torch.from_numpy(np.stack(one)).to(p.engine._tdev), boxes):
            x = b["image"].permute(0, 2, 3, 1).contiguous().to(ex.adt)
            for i in range(x.shape[0]):
                (a,) = ex.run_device(x[i:i + 1], 3)
                v = ex.values(a).cpu().numpy().reshape(1, -1, 97)
                (text, sc), = task._ctc.decode_ids(np.argmax(v, -1), v.max(-1))
                k = int(b["indices"][b["batch_beg_img_no"] + i])
                texts[k], scores[k] = text, float(sc)
        for r in (res, again):
            assert [e["text"] for e in r[0].ocr_result] == texts
            got_s = np.array([e["score"] for e in r[0].ocr_result])
            assert (np.abs(got_s - np.array(scores)) <= SCORE_REL * np.array(scores)).all()
        assert sum(bool(t) for t in texts) >= 20
    finally:
        p.engine.close()
