"""The layout decode on the device (pt_op_layout_decode, device_decode=True), measured (profiles/r20/layout_decode.txt): one process, warm-up first,
medians with ranges of 7 windows, on and off alternating.  Off is the route before the knob existed (records to the host, LayoutStage.decode_page).

  kernel  pt_op_layout_decode per call at 64 pages of 474 records (the ONNX stand-in's count) and at 64 full pages of max_cands = 2048 records,
          five classes, four levels.  Device events around 20 back-to-back calls; ms per call.  The host decode of the same pages beside it.
  stage   forward() + finish() per 64 pages of 1024 x 1024, knob off against on, for LayoutStage (seeded in-tree net) and OnnxLayoutStage (the
          PicoLike stand-in of tests/test_gpu_onnx_layout_pipeline.py).  Host clock around forward + finish, ms per call.
  stream  predict_stream() with detection, recognition and layout on seeded pages (8 batches of 16), the layout stage object swapped between an
          off and an on stage of the same pipeline, alternating.  pages/s.

    python tools/layout_decode_bench.py [out.txt]
"""
from __future__ import annotations

import os
import statistics
import sys
import tempfile
import time
import warnings
from pathlib import Path

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from pdf_table_amd.engine import HipEngine  # noqa: E402
from pdf_table_amd.layout_stage import LayoutStage, OnnxLayoutStage  # noqa: E402

B, RUNS = 64, 7


def stats(v):
    return f"{statistics.median(v):9.4f} ({min(v):.4f} .. {max(v):.4f})"


def verdict(on, off, smaller_is_better=True):
    below = max(on) < min(off) if smaller_is_better else min(on) > max(off)
    return "the on range lies clear of the off range" if below else "the ranges overlap: no difference shown"


def kernel_bench(out):
    import layout_decode_ref as R
    eng = HipEngine(0)
    cfg = R.make_cfg(ncls=5, strides=(8, 16, 32, 64))
    out.append(f"== kernel: pt_op_layout_decode, {B} pages per call, 5 classes, 4 levels, logits; median (min .. max) of {RUNS} windows of 20 calls ==")
    for name, n, per_level, max_cands in (("474 records", 474, [300, 120, 40, 14], 2048), ("2048 records (max_cands)", 2048, [1400, 500, 120, 28], 2048)):
        cases = [R.random_case(f"b{k}", 1000 + k, n, cfg, (1024, 1024), False, level_counts=per_level, hot=0.5) for k in range(8)]
        cands = np.zeros((B, max_cands, R.REC), np.float32)
        for i in range(B):
            cands[i, :n] = cases[i % 8]["rec"]
        counts_d = torch.full((B,), n, dtype=torch.int32, device=eng._tdev)
        cands_d = torch.from_numpy(cands).to(eng._tdev)
        call = lambda: eng.op_layout_decode(counts_d, cands_d, 5, cfg.strides, cfg.img_height, cfg.img_width, 1024, 1024, probs=False,
                                            score_threshold=cfg.score_threshold, nms_threshold=cfg.nms_threshold, nms_top_k=cfg.nms_top_k,
                                            candidate_size=200, keep_top_k=cfg.keep_top_k)
        ndet = call()[0].cpu().numpy()
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(RUNS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / 20)
        host_ms = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(3):
                t0 = time.perf_counter()
                nh = [len(R.host_decode(cases[i % 8])) for i in range(B)]
                host_ms.append((time.perf_counter() - t0) * 1e3)
        out.append(f"{name:26s}: kernel {stats(ms)} ms per call   decode_page on the host {stats(host_ms)} ms per {B} pages (3 runs)   "
                   f"detections per page {int(ndet.min())} .. {int(ndet.max())}, counts equal to decode_page's: {nh == ndet.tolist()}")
    eng.close()


def _time_stage(stage, pages_t, org):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, ticket = stage.forward(pages_t)
    res = stage.finish(n, ticket, org)
    return (time.perf_counter() - t0) * 1e3, res


def stage_bench(out, standin):
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    from pdf_table_amd.synth_pages import make_page
    pages = np.stack([make_page(i % 8, 1024)[0] for i in range(B)])
    for what, kw in (("LayoutStage (seeded in-tree net, bf16)", dict(synthetic_seed=4)), ("OnnxLayoutStage (PicoLike stand-in, bf16)", dict(task_path=standin))):
        task = OcrLayoutTask(model="picodet", task_type="en", **kw)
        off = task._stage
        on = (OnnxLayoutStage(task._engine, task._exec, task._config, device_decode=True) if isinstance(off, OnnxLayoutStage)
              else LayoutStage(task._engine, task._config, device_decode=True))
        pages_t = torch.from_numpy(pages).to(task._engine._tdev)
        org = tuple(pages_t.shape[1:3])
        for _ in range(3):
            for s in (off, on):
                _time_stage(s, pages_t, org)
        ms = {id(off): [], id(on): []}
        for _ in range(RUNS):
            for s in (off, on):
                t, res = _time_stage(s, pages_t, org)
                ms[id(s)].append(t)
        nreg = [len(r) for r in res]
        n, ticket = off.forward(pages_t)
        ticket[0].synchronize()
        cnt = ticket[1][0][:n].numpy().copy()
        off.finish(n, ticket, org)
        out.append(f"== stage: {what}, forward + finish per {B} pages of 1024 x 1024; candidates per page {cnt.min()} .. {cnt.max()} (mean {cnt.mean():.0f}), "
                   f"regions per page {min(nreg)} .. {max(nreg)}; host clock, ms per call, median (min .. max) of {RUNS}, alternating ==")
        out.append(f"device_decode=False: {stats(ms[id(off)])}")
        out.append(f"device_decode=True : {stats(ms[id(on)])}   {verdict(ms[id(on)], ms[id(off)])}")
        task._engine.close()


def stream_bench(out, standin):
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_pages import make_page
    pipe = OcrTablePipeline(device=0, synthetic_seed=0, layout=True, layout_task_path=standin)
    off = pipe.layout_task._stage
    on = OnnxLayoutStage(pipe.engine, off.exec, off.config, device_decode=True)
    pages = torch.from_numpy(np.stack([make_page(i % 8)[0] for i in range(16)])).to(pipe.engine._tdev)
    batches = [pages] * 8

    def run(stage):
        pipe.layout_task._stage = stage
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(len(r) for r in pipe.predict_stream(batches))
        return n / (time.perf_counter() - t0)

    for s in (off, on):
        run(s)
    pps = {id(off): [], id(on): []}
    for _ in range(RUNS):
        for s in (off, on):
            pps[id(s)].append(run(s))
    out.append(f"== stream: predict_stream(), detection + recognition + ONNX layout (stand-in), seeded, bf16, 8 batches of 16 pages of 1024 x 1024 per run; "
               f"median (min .. max) of {RUNS}, alternating ==")
    out.append(f"device_decode=False: {stats(pps[id(off)])} pages/s")
    out.append(f"device_decode=True : {stats(pps[id(on)])} pages/s   {verdict(pps[id(on)], pps[id(off)], smaller_is_better=False)}")
    pipe.layout_task._stage = off
    pipe.engine.close()


if __name__ == "__main__":
    import test_gpu_onnx_layout_pipeline as P
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        standin = str(P._export(Path(tmp)))
        kernel_bench(lines)
        stage_bench(lines, standin)
        stream_bench(lines, standin)
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)
