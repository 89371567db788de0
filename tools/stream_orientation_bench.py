"""tools/stream_orientation_bench.py [steps] [warmup]: what the text-line orientation vote costs inside OcrTablePipeline.predict_stream().

64-page steps of 1024 x 1024 generator pages (device-resident, bench.py's batch) through the four stages (layout, detection, recognition, Lore table
structure on the layout stage's regions) on one compute stream, as bench.py's timed loop runs them -- W untimed warm-up steps after the spin-up,
then K timed steps -- once with predict_stream() and once with predict_stream(orientation_vote=True) and the fitted synthetic orientation head
(pplcnet_state_dict(seed=5, class_num=2, textline_head=True)), in one process.  Prints pages/s both ways, lines classified per page, pages rotated,
the host seconds of the vote's phases, the classifier's device milliseconds per step (engine profiler, every launch of one
pt_cls_forward_lines_direct over a step's lines) and its fused pre-process kernel against the three-launch chain of pt_cls_forward_lines on the
same lines."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdf_table_amd import lib as L                                        # noqa: E402
from pdf_table_amd.det_stage import DetConfig                             # noqa: E402
from pdf_table_amd.pipeline import OcrTablePipeline                       # noqa: E402
from pdf_table_amd.rec_stage import build_lines                           # noqa: E402
from pdf_table_amd.synth_pages import make_page                           # noqa: E402
from pdf_table_amd.synth_weights import (crnn_state_dict, db_resnet18_state_dict, picodet_state_dict,   # noqa: E402
                                          pplcnet_state_dict)
from pdf_table_amd.weights import pack_crnn, pack_db_resnet18, pack_picodet, pack_pplcnet   # noqa: E402

PAGES, SPIN = 64, 2


def timed_run(p, pages, steps, vote):
    rot = lines = n = 0
    t0 = time.perf_counter()
    for res in p.predict_stream([pages] * steps, orientation_vote=vote):
        for r in res:
            n += 1
            rot += int(r.rotated_180)
            lines += len(r.text_line_orientation or ())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n, rot, lines, dict(p.metric["host_seconds"])


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    p = OcrTablePipeline(device=0, synthetic_seed=0, layout=True, table_structure=True, text_orientation=True, overlap_rec=False)
    eng = p.engine
    # bench.py's checkpoints: the detector with the text channel (its boxes are the lines), the conditioned recogniser, the layout head fitted to
    # the generator's pages (its "table" regions feed the table stage)
    eng.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=eng.weight_fmt))
    p.text_detector._stage.cfg = DetConfig(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5).resolved()
    eng.load_weights(L.PT_MODEL_CRNN, pack_crnn(crnn_state_dict(seed=1, conditioned=True), fmt=eng.weight_fmt))
    eng.load_weights(L.PT_MODEL_PICODET, pack_picodet(picodet_state_dict(seed=4, num_classes=5, table_head=True), 5, fmt=eng.weight_fmt))
    eng.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True), fmt=eng.weight_fmt))
    pages = torch.from_numpy(np.stack([make_page(i)[0] for i in range(PAGES)])).cuda()
    out = {}
    for vote in (False, True):
        # predict_stream() refuses a pipeline with the classifier attached unless the vote is asked for: detached for the plain leg
        task, p.orientation_task = p.orientation_task, (p.orientation_task if vote else None)
        try:
            timed_run(p, pages, SPIN + warm, vote)
            dt, n, rot, lines, host = timed_run(p, pages, steps, vote)
        finally:
            p.orientation_task = task
        out[vote] = (dt, n, rot, lines, host)
        print(f"orientation_vote={vote}: {n / dt:.1f} pages/s ({steps} x {PAGES} pages, {dt:.3f} s; drain inside the timed region)"
              + (f"; {lines / n:.1f} lines classified per page, {rot} of {n} pages rotated" if vote else ""), flush=True)
        print("  host seconds:", {k: round(v, 3) for k, v in host.items() if k in ("orient", "collect.orientation", "halves.cls_start",
                                                                                      "halves.orient", "host_halves", "collect")}, flush=True)
    off, on = out[False], out[True]
    print(f"price of the vote: {(on[0] / on[1] - off[0] / off[1]) * PAGES * 1e3:.1f} ms per {PAGES}-page step "
          f"({off[1] / off[0]:.1f} -> {on[1] / on[0]:.1f} pages/s)")

    # the classifier alone over one step's lines (the first detection of the 64 pages)
    det = p.text_detector._stage
    prob, bitmap, ev = det.forward(pages)
    lines = build_lines(det.boxes(prob, bitmap, tuple(pages.shape[1:3]), ev))
    cls = p.orientation_task._stage
    for _ in range(2):
        eng.cls_forward_lines_direct(pages, lines, cls.cfg["size"], 0, True)
        eng.cls_forward_lines(pages, lines, cls.cfg["size"], 0, True)
    torch.cuda.synchronize()
    for name, fn in (("direct", eng.cls_forward_lines_direct), ("crop-buffer chain", eng.cls_forward_lines)):
        eng.profile_read_labels()
        eng.profile_enable(1)
        reps = 5
        for _ in range(reps):
            fn(pages, lines, cls.cfg["size"], 0, True)
        torch.cuda.synchronize()
        eng.profile_enable(0)
        lab = eng.profile_read_labels()
        tot = sum(v["ms"] for v in lab.values()) / reps
        pre = {k: round(v["ms"] / reps, 3) for k, v in lab.items() if k.startswith("cls ")}
        print(f"{name}: {len(lines)} lines ({len(lines) / PAGES:.1f} per page): {tot:.2f} device ms per step (every launch, events), "
              f"pre-process {pre}", flush=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(pages, lines, cls.cfg["size"], 0, True)
        e1.record()
        torch.cuda.synchronize()
        print(f"  wall on the stream: {e0.elapsed_time(e1) / reps:.2f} ms per call", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
