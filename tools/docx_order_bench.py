"""DocXLayout's region list and reading order on the device (pt_op_docx_order, device_order=True), measured (profiles/r24/docx_order.txt): one
process, warm-up first, medians with ranges of 7 windows; "on" and "off" alternate inside every window.  Off is the route without the knob
(records landed, docx_page_result on the host), not a variant of the new code.

  kernel  pt_op_docx_order per call at 64 pages: the seeded net's records, and 64 copies of a crafted page of 63 loose blocks (the longest list the
          kernel sorts).  Device events around 20 back-to-back calls; ms per call.
  stage   DocXLayoutStage forward + finish per 64 pages of 1024 x 1024 (bf16), on against off; finish alone on the landed tensors, on against off;
          the share of pages that took the host fallback.
  stream  predict_stream() with detection, recognition and this layout on seeded pages (8 batches of 16), on against off.  pages/s.

    python tools/docx_order_bench.py [out.txt]
"""
from __future__ import annotations

import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.centernet_stage import centernet_decode_affine  # noqa: E402
from pdf_table_amd.docxlayout_stage import DocXLayoutConfig, DocXLayoutStage  # noqa: E402
from pdf_table_amd.engine import HipEngine  # noqa: E402
from pdf_table_amd.synth_weights import docxlayout_dla34_state_dict  # noqa: E402
from pdf_table_amd.weights import pack_docxlayout_dla34  # noqa: E402

B, RUNS = 64, 7


def stats(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _crafted_63(K=100):
    """one page of 63 loose axis-aligned regions, seeded, as records in map pixels (x4 to the page)"""
    rng = np.random.RandomState(63)
    counts = np.zeros((1, 2), np.int32)
    recs = np.zeros((1, 2, K, 12), np.float32)
    keep = np.ones((1, 2, K), np.uint8)
    for k in range(63):
        x, y, w, h = rng.randint(0, 540), rng.randint(0, 570), rng.randint(10, 60), rng.randint(5, 30)
        recs[0, 0, k, :8] = np.array([x, y, x + w, y, x + w, y + h, x, y + h], np.float32) / 4
        recs[0, 0, k, 8], recs[0, 0, k, 9] = rng.uniform(0.35, 0.98), 2
    counts[0, 0] = 63
    return counts, recs, keep


def stage_and_kernel_bench(out):
    from pdf_table_amd.synth_pages import make_page
    eng = HipEngine(0)
    eng.load_weights(L.PT_MODEL_DOCX_DLA34, pack_docxlayout_dla34(docxlayout_dla34_state_dict(seed=0), fmt=eng.weight_fmt))
    off, on = DocXLayoutStage(eng, DocXLayoutConfig()), DocXLayoutStage(eng, DocXLayoutConfig(), device_order=True)
    pages = torch.from_numpy(np.stack([make_page(i % 8, 1024)[0] for i in range(B)])).to(eng._tdev)
    org = tuple(pages.shape[1:3])
    for s in (off, on):      # warm-up
        n, t = s.forward(pages)
        res = s.finish(n, t, org)
    nreg = [len(r) for r in res]
    fallback = len(on.last_fallback)
    # the launch alone, on the records of these pages (still on the device) and on the crafted page
    counts, recs, keep = (h[:B].to(eng._tdev) for h in t[1][:3])
    bufs = on._order_launch(counts, recs, keep, org)
    inv = centernet_decode_affine(org[0], org[1], 192, 192)
    net = lambda: eng.op_docx_order(counts, recs, keep, inv, out=bufs)
    c63 = tuple(torch.from_numpy(np.repeat(v, B, 0)).to(eng._tdev) for v in _crafted_63())
    bufs63 = eng.op_docx_order(*c63, inv)
    big = lambda: eng.op_docx_order(*c63, inv, out=bufs63)
    torch.cuda.synchronize()
    assert int(bufs63[1].sum()) == 0 and int(bufs63[0].min()) == 63
    t_net = [_events(net, 20) for _ in range(RUNS)]
    t_big = [_events(big, 20) for _ in range(RUNS)]
    out.append(f"== kernel: pt_op_docx_order, {B} pages per call; ms per call, median (min .. max) of {RUNS} windows of 20 calls ==")
    out.append(f"seeded net's records ({min(nreg)} .. {max(nreg)} regions a page): {stats(t_net)}")
    out.append(f"{B} copies of a crafted page of 63 loose blocks:        {stats(t_big)}")
    # forward + finish and finish alone, on and off alternating in every window
    both = {"off": (off, [], []), "on": (on, [], [])}
    for rep in range(RUNS + 1):
        for name, (s, all_ms, fin_ms) in both.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n, ticket = s.forward(pages)
            s.finish(n, ticket, org)
            t1 = time.perf_counter()
            s.finish(n, ticket, org)      # the copy has landed: the host half alone
            t2 = time.perf_counter()
            if rep:
                all_ms.append((t1 - t0) * 1e3)
                fin_ms.append((t2 - t1) * 1e3)
    out.append(f"== stage: DocXLayoutStage (seeded checkpoint, bf16), per {B} pages of 1024 x 1024 at 768 x 768; ms (host clock), median (min .. max) of "
               f"{RUNS} windows, on and off alternating, the first window dropped ==")
    for name, (_, all_ms, fin_ms) in both.items():
        out.append(f"forward + finish, device_order {name:3s}: {stats(all_ms)}")
    for name, (_, all_ms, fin_ms) in both.items():
        out.append(f"finish alone,     device_order {name:3s}: {stats(fin_ms)}")
    lo_off, hi_on = min(both["off"][1]), max(both["on"][1])
    out.append(f"forward + finish: the on range lies {'clear below' if hi_on < lo_off else 'NOT clear below (the ranges overlap)'} the off range")
    out.append(f"pages that took the host fallback: {fallback} of {B}")
    eng.close()


def stream_bench(out, ckpt):
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_pages import make_page
    pipes = {"off": OcrTablePipeline(device=0, synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path=ckpt),
             "on": OcrTablePipeline(device=0, synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path=ckpt, layout_device_order=True)}
    pps = {k: [] for k in pipes}
    for rep in range(RUNS + 1):
        for name, pipe in pipes.items():
            pages = torch.from_numpy(np.stack([make_page(i % 8)[0] for i in range(16)])).to(pipe.engine._tdev)
            batches = [pages] * 8
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(len(r) for r in pipe.predict_stream(batches))
            if rep:
                pps[name].append(n / (time.perf_counter() - t0))
    out.append(f"== stream: predict_stream(), detection + recognition + DocXLayout, seeded, bf16, 8 batches of 16 pages of 1024 x 1024 per run; pages/s, "
               f"median (min .. max) of {RUNS}, on and off alternating ==")
    for name in pipes:
        out.append(f"layout_device_order {name:3s}: {stats(pps[name])}")
    for pipe in pipes.values():
        pipe.engine.close()


if __name__ == "__main__":
    lines = ["how: python tools/docx_order_bench.py profiles/r24/docx_order.txt -- one process on one MI355X, nothing else on the device"]
    with tempfile.TemporaryDirectory() as tmp:
        torch.save(docxlayout_dla34_state_dict(seed=0), os.path.join(tmp, "pytorch_model.bin"))
        stage_and_kernel_bench(lines)
        stream_bench(lines, tmp)
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)
