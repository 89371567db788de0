"""tools/pprec_stage_bench.py [--parts tail,stage,stream] [--pages N] [--windows W]: what serving the PP-OCR recognisers through PPRecStage costs.

  tail    pt_op_ctc_greedy against the layered route for the same result -- pt_op_softmax to fp32 probabilities, then torch.max -- on token rows
          [256 * 40, 6625] (a 6625-class dictionary, 256 lines of 40 tokens) and [6 * 40, 97] (one reference mini-batch of the stand-ins), in bf16 and
          in the (hi | lo) pair mode.  The two routes alternate inside every window; device events around each run of ITERS calls.
  stage   lines/s of PPRecStage over N generator pages (bench.py's pages, 1024 x 1024) and the boxes the seeded text detector finds on them, for both
          stand-ins (SvtrLcnetRecLike as "PP-OCRv4", MobileV3RecLike as "PP-Table"; 97 classes, dynamic batch, width 320: the real *_rec_infer files
          are not available offline), with rec_batch_num=6 and with rec_batch_num=64, rec_width_bucket=32 -- against the crop door
          (OcrRecognitionTask._predict_pp) fed host crops of the same boxes, the only route there was before the stage.
  stream  predict_stream() pages/s (detection + recognition, 64-page steps) with recognizer="PP-OCRv4" beside the in-tree CRNN.

Every figure is a median over W windows with its range; each window ends in a device synchronise."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from pdf_table_amd import lib as L                                        # noqa: E402
from pdf_table_amd.det_stage import DetConfig                             # noqa: E402
from pdf_table_amd.engine import HipEngine                                # noqa: E402
from pdf_table_amd.pipeline import OcrTablePipeline                       # noqa: E402
from pdf_table_amd.synth_pages import make_page                           # noqa: E402
from pdf_table_amd.synth_weights import crnn_state_dict, db_resnet18_state_dict   # noqa: E402
from pdf_table_amd.weights import pack_crnn, pack_db_resnet18             # noqa: E402

STANDINS = {"PP-OCRv4": ("SvtrLcnetRecLike", 3, 6.0), "PP-Table": ("MobileV3RecLike", 2, 3.0)}      # seeds and head scales of tests/test_gpu_onnx_pprec_door.py


def med(xs):
    return f"median {statistics.median(xs):.4g} (range {min(xs):.4g} .. {max(xs):.4g}, {len(xs)} windows)"


def part_tail(windows):
    print("== tail: op_ctc_greedy vs op_softmax(f32=True) + torch.max, microseconds per call ==")
    for mode, prec in (("bf16", L.PT_PRECISION_BF16), ("split", L.PT_PRECISION_BF16X3)):
        eng = HipEngine(0)
        eng.set_precision(prec)
        split = mode == "split"
        for rows, C, Cp, iters in ((256 * 40, 6625, 6656, 20), (6 * 40, 97, 128, 200)):
            g = torch.Generator().manual_seed(7)
            x = (torch.randn(rows, Cp * (2 if split else 1), generator=g) * 6.0)
            if split:
                x[:, Cp:] *= 2.0 ** -9                     # a lo half below half an ulp of hi
            x = x.to(torch.bfloat16).cuda()

            def fused():
                return eng.op_ctc_greedy(x, C, split=split)

            def layered():
                return eng.op_softmax(x, C, f32=True, split=split).max(-1)
            ids, conf = fused()
            lc, li = layered()
            torch.cuda.synchronize()
            same = float((ids.long() == li.reshape(-1)).float().mean())
            dconf = float((conf - lc.reshape(-1)).abs().max())
            for fn in (fused, layered):                    # warm clocks and code objects
                for _ in range(iters):
                    fn()
            torch.cuda.synchronize()
            t = {"fused": [], "layered": []}
            for _ in range(windows):
                for name, fn in (("fused", fused), ("layered", layered)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    t[name].append(e0.elapsed_time(e1) * 1000.0 / iters)
            nbytes = rows * C * 2 * (2 if split else 1)
            print(f"{mode} [{rows}, {C}] (Cp {Cp}): fused {med(t['fused'])} us; layered {med(t['layered'])} us; "
                  f"ratio of medians {statistics.median(t['layered']) / statistics.median(t['fused']):.2f}x; logits read at "
                  f"{nbytes / statistics.median(t['fused']) / 1e6:.2f} TB/s by the fused kernel; same ids on {100 * same:.3f} % of rows (torch.max has no tie "
                  f"order), max |conf difference| {dconf:.2e}")
        eng.close()


def export_standins(tmp):
    import onnx_export as X
    import onnx_export_pprec as P
    dirs = {}
    for name, (cls, seed, scale) in STANDINS.items():
        d = os.path.join(tmp, name.replace("-", "_").lower())
        os.makedirs(d)
        chars = [chr(0x61 + i % 26) + str(i // 26) for i in range(95)]
        with open(os.path.join(d, "en_dict.txt"), "w", encoding="utf-8") as f:
            f.write("\n".join(chars) + "\n")
        m = P.seeded_pprec(getattr(P, cls)(classes=97), seed, head_scale=scale)
        with open(os.path.join(d, "model.onnx"), "wb") as f:
            f.write(X.torch_export(m, torch.zeros(2, 3, 48, 320), dynamic_batch=True))
        dirs[name] = d
    return dirs


def bench_detector(p):
    """bench.py's detector: the seeded DB-ResNet18 with the text channel, its boxes are the generator's lines"""
    eng = p.engine
    eng.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=eng.weight_fmt))
    p.text_detector._stage.cfg = DetConfig(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5).resolved()


def detect(p, pages):
    from pdf_table_amd.det_stage import sort_boxes_reading_order
    st = p.text_detector._stage
    prob, bitmap, ev = st.forward(pages)
    return [sort_boxes_reading_order(b) for b in st.boxes(prob, bitmap, tuple(pages.shape[1:3]), ev)]


def part_stage(dirs, npages, windows):
    print(f"== stage: PPRecStage lines/s on {npages} generator pages and the seeded detector's boxes ==")
    pages_np = np.stack([make_page(i)[0] for i in range(npages)])
    pages = torch.from_numpy(pages_np).cuda()
    for name, d in dirs.items():
        boxes = None
        for label, kw in (("rec_batch_num=6", {}), ("rec_batch_num=64, rec_width_bucket=32", {"rec_batch_num": 64, "rec_width_bucket": 32})):
            p = OcrTablePipeline(device=0, synthetic_seed=0, recognizer=name, rec_task_path=d, **kw)
            bench_detector(p)
            if boxes is None:
                boxes = detect(p, pages)
            nl = sum(len(b) for b in boxes)
            stage = p.text_recognizer._stage
            for _ in range(3):                         # eager walk, capture, replay
                texts = stage(pages, boxes)
            torch.cuda.synchronize()
            rates = []
            for _ in range(windows):
                t0 = time.perf_counter()
                for _ in range(2):
                    stage(pages, boxes)
                torch.cuda.synchronize()
                rates.append(2 * nl / (time.perf_counter() - t0))
            print(f"{name} PPRecStage, {label}: {nl} lines, {len(set(stage.last_widths))} distinct widths, tail "
                  f"{'fused' if stage.exec.ctc_tail_layer is not None else 'layered'}: {med(rates)} lines/s; non-empty strings {sum(bool(t) for pg in texts for t in pg)}")
            if not kw:
                # the only route before the stage: host crops (the boxes' bounding rectangles; the generator's lines are axis-aligned) through the crop door
                crops = []
                for k, bx in enumerate(boxes):
                    for q in np.asarray(bx).reshape(-1, 4, 2):
                        x0, y0 = np.floor(q.min(0)).astype(int).clip(0)
                        x1, y1 = np.ceil(q.max(0)).astype(int)
                        if x1 > x0 and y1 > y0:
                            crops.append(np.ascontiguousarray(pages_np[k, y0:y1, x0:x1]))
                task = p.text_recognizer
                for _ in range(3):
                    task._predict_pp(crops)
                torch.cuda.synchronize()
                rates = []
                for _ in range(windows):
                    t0 = time.perf_counter()
                    task._predict_pp(crops)
                    torch.cuda.synchronize()
                    rates.append(len(crops) / (time.perf_counter() - t0))
                print(f"{name} crop door (_predict_pp, host crops, rec_batch_num=6): {len(crops)} lines: {med(rates)} lines/s")
            p.engine.close()


def part_stream(dirs, windows, steps=6):
    print(f"== stream: predict_stream() pages/s, detection + recognition, 64-page steps, {steps} steps per window ==")
    pages = torch.from_numpy(np.stack([make_page(i)[0] for i in range(64)])).cuda()
    for name in ("CRNN", "PP-OCRv4"):
        kw = {} if name == "CRNN" else {"rec_task_path": dirs[name], "rec_batch_num": 64, "rec_width_bucket": 32}
        p = OcrTablePipeline(device=0, synthetic_seed=0, recognizer=name, overlap_rec=False, **kw)
        bench_detector(p)
        if name == "CRNN":
            p.engine.load_weights(L.PT_MODEL_CRNN, pack_crnn(crnn_state_dict(seed=1, conditioned=True), fmt=p.engine.weight_fmt))
        lines = 0
        for res in p.predict_stream([pages] * 4):          # spin-up: arenas, captures
            lines = sum(len(r.ocr_result) for r in res)
        torch.cuda.synchronize()
        rates = []
        for _ in range(windows):
            t0 = time.perf_counter()
            n = sum(len(res) for res in p.predict_stream([pages] * steps))
            torch.cuda.synchronize()
            rates.append(n / (time.perf_counter() - t0))
        print(f"recognizer={name}{'' if name == 'CRNN' else ' (rec_batch_num=64, rec_width_bucket=32)'}: {lines} lines per step: {med(rates)} pages/s")
        p.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="tail,stage,stream")
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    parts = a.parts.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("pprec_stage_bench: no GPU -- nothing is measured without one")
    print(f"device: {torch.cuda.get_device_name(0)}")
    if "tail" in parts:
        part_tail(a.windows)
    if "stage" in parts or "stream" in parts:
        with tempfile.TemporaryDirectory() as tmp:
            dirs = export_standins(tmp)
            if "stage" in parts:
                part_stage(dirs, a.pages, a.windows)
            if "stream" in parts:
                part_stream(dirs, a.windows)


if __name__ == "__main__":
    main()
