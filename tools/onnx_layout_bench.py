"""tools/onnx_layout_bench.py [--parts kernel,stage,stream] [--pages N] [--windows W] [--out FILE]: what serving a PicoDet ONNX export through
OnnxLayoutStage costs.  Stand-in: tools/onnx_export.py:PicoLike(ncls=5, levels=4), seeded as in tests/test_gpu_onnx_layout_pipeline.py, exported at
800 x 608 with a dynamic batch (the real *_layout_infer files are not available offline).  Pages: the generator's (bench.py's), 1024 x 1024.

  kernel  pt_op_pico_candidates alone on the graph's outputs for N pages, in bf16 and in the (hi | lo) pair mode: microseconds per call (device
          events around runs of ITERS calls), the bytes it NEEDS to read -- the real score channels of every anchor plus the 32 distribution values
          of the kept anchors -- and the rate that implies.  (What it moves is more: a row's real channels sit in a padded row of their own, so
          every anchor costs at least one memory transaction.)
  stage   OnnxLayoutStage.forward + finish per N pages against OcrLayoutTask._detect_pages_host on the same graph and pages, alternating inside
          every window; the host route split into graph (to a device synchronise), the 2 L copies, and the numpy filter + decode.
  stream  predict_stream() pages/s over detection + recognition + layout in N-page steps, the ONNX stand-in and the in-tree layout net
          alternating inside every window.

Every figure is a median over W windows with its range; every window ends in a device synchronise.  The lines are printed and written to FILE
(default profiles/r17/onnx_layout.txt)."""
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
from pdf_table_amd.ocr_layout_task import OcrLayoutTask                   # noqa: E402
from pdf_table_amd.pipeline import OcrTablePipeline                       # noqa: E402
from pdf_table_amd.synth_pages import make_page                           # noqa: E402
from pdf_table_amd.synth_weights import crnn_state_dict, db_resnet18_state_dict   # noqa: E402
from pdf_table_amd.weights import pack_crnn, pack_db_resnet18             # noqa: E402

LINES = []
REPS = 8          # stage calls per timed window


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return f"median {statistics.median(xs):.4g} (range {min(xs):.4g} .. {max(xs):.4g}, {len(xs)} windows)"


def export_standin(tmp):
    import onnx_export as X
    m = X.seeded(X.PicoLike(ncls=5, levels=4), 21)
    with torch.no_grad():
        for h in m.heads:
            h.bias[:5] -= 2.0
            h.weight[:5] *= 3.0
    with open(os.path.join(tmp, "model.onnx"), "wb") as f:
        f.write(X.torch_export(m, torch.zeros(1, 3, 800, 608), dynamic_batch=True))
    return tmp


def part_kernel(d, pages, windows, iters=50):
    say(f"== kernel: pt_op_pico_candidates on the outputs of PicoLike(levels=4) at [{pages.shape[0]}, 3, 800, 608], microseconds per call ==")
    for precision in ("bf16", "fp32"):
        task = OcrLayoutTask(model="picodet", task_type="en", task_path=d, precision=precision)
        eng, ex, cfg = task._engine, task._exec, task._config
        x = eng.layout_preprocess(pages.to(eng._tdev), cfg.img_height, cfg.img_width)
        acts = ex.run_device(x, 3)                        # eager: the tensors stay ours
        half = len(acts) // 2
        sc, bd = [a.t for a in acts[:half]], [a.t for a in acts[half:]]
        ncls, m = len(cfg.labels), ex.m
        out = eng.op_pico_candidates(sc, bd, ncls, cfg.score_threshold - 1e-3, split=ex.split)

        def call():
            eng.op_pico_candidates(sc, bd, ncls, cfg.score_threshold - 1e-3, split=ex.split, out=out)
        for _ in range(iters):
            call()
        torch.cuda.synchronize()
        kept = int(out[0].sum())
        t = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                call()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / iters)
        anchors = sum(int(a.t.shape[2]) for a in acts[:half])
        need = pages.shape[0] * anchors * ncls * 2 * m + kept * 32 * 2 * m
        rows = pages.shape[0] * anchors * sc[0].shape[-1] * 2
        say(f"{ex.precision}: {anchors} anchors per page in {half} levels, {kept} kept on {pages.shape[0]} pages (largest page {int(out[0].max())}): "
            f"{med(t)} us per call (memset + launch); bytes needed {need} (score channels {pages.shape[0] * anchors * ncls * 2 * m}, kept "
            f"distributions {kept * 32 * 2 * m}) -> {need / statistics.median(t) / 1e3:.2f} GB/s; the padded score rows those channels sit in are "
            f"{rows} bytes -> {rows / statistics.median(t) / 1e3:.1f} GB/s if every row costs its whole width; records written {kept * 192} bytes")
        eng.close()


def part_stage(d, pages, windows):
    n = pages.shape[0]
    say(f"== stage: OnnxLayoutStage.forward + finish against _detect_pages_host, milliseconds per {n} pages (same graph, same pages, alternating, {REPS} calls per window) ==")
    for precision in ("bf16", "fp32"):
        task = OcrLayoutTask(model="picodet", task_type="en", task_path=d, precision=precision)
        stage, dev = task._stage, task._engine._tdev
        pg = pages.to(dev)
        org = tuple(pg.shape[1:3])
        for _ in range(3):                                # eager walk, capture, replay
            got = stage(pg)
            want = task._detect_pages_host(pg)
        same = all(len(a) == len(b) and all(x["bbox"].tobytes() == y["bbox"].tobytes() and x["score"] == y["score"] and x["label"] == y["label"]
                                            for x, y in zip(a, b)) for a, b in zip(got, want))
        torch.cuda.synchronize()
        t = {"stage": [], "host": [], "graph": [], "copies": [], "filter": []}
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(REPS):
                nn, ticket = stage.forward(pg)
                stage.finish(nn, ticket, org)
            torch.cuda.synchronize()
            t["stage"].append((time.perf_counter() - t0) * 1e3 / REPS)
            t0 = time.perf_counter()
            for _ in range(REPS):
                task._detect_pages_host(pg)
            torch.cuda.synchronize()
            t["host"].append((time.perf_counter() - t0) * 1e3 / REPS)
            # the host route in its three parts
            t0 = time.perf_counter()
            _, acts = stage._graph_outputs(pg)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            outs = [stage.exec.values(a)[:, 0].cpu().numpy() for a in acts]
            t2 = time.perf_counter()
            half = len(outs) // 2
            for i in range(n):
                stage.decode_outputs([s_[i] for s_ in outs[:half]], [b_[i] for b_ in outs[half:]], org)
            t3 = time.perf_counter()
            t["graph"].append((t1 - t0) * 1e3)
            t["copies"].append((t2 - t1) * 1e3)
            t["filter"].append((t3 - t2) * 1e3)
        say(f"{stage.exec.precision}: regions per page {min(len(g) for g in got)} .. {max(len(g) for g in got)}, results equal bit for bit: {same}; device tail "
            f"used: {all(stage._tail_ok.values())}")
        say(f"  forward + finish      {med(t['stage'])} ms")
        say(f"  _detect_pages_host    {med(t['host'])} ms; ratio of medians host / stage {statistics.median(t['host']) / statistics.median(t['stage']):.2f}x; "
            f"stage slower than host in {sum(s_ > h_ for s_, h_ in zip(t['stage'], t['host']))} of {windows} windows")
        say(f"  host route in parts   pre-process + graph to a synchronise {med(t['graph'])} ms; values() + {len(outs)} .cpu().numpy() copies "
            f"{med(t['copies'])} ms; numpy filter + decode + NMS {med(t['filter'])} ms")
        task._engine.close()


def bench_detector(p):
    """bench.py's detector: the seeded DB-ResNet18 with the text channel, its boxes are the generator's lines"""
    eng = p.engine
    eng.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=eng.weight_fmt))
    p.text_detector._stage.cfg = DetConfig(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5).resolved()
    eng.load_weights(L.PT_MODEL_CRNN, pack_crnn(crnn_state_dict(seed=1, conditioned=True), fmt=eng.weight_fmt))


def part_stream(d, pages, windows, steps=10):
    n = pages.shape[0]
    say(f"== stream: predict_stream() pages/s, detection + recognition + layout, {n}-page steps, {steps} steps per window, the two pipelines alternating ==")
    pg = pages.cuda()
    pipes = {"ONNX stand-in (OnnxLayoutStage)": OcrTablePipeline(device=0, synthetic_seed=0, layout=True, layout_task_path=d, overlap_rec=False),
             "in-tree layout net (LayoutStage)": OcrTablePipeline(device=0, synthetic_seed=0, layout=True, overlap_rec=False)}
    regions = {}
    for name, p in pipes.items():
        bench_detector(p)
        for res in p.predict_stream([pg] * 4):            # spin-up: arenas, captures
            regions[name] = sum(len(r.layout_result) for r in res)
    torch.cuda.synchronize()
    rates = {name: [] for name in pipes}
    for _ in range(windows):
        for name, p in pipes.items():
            t0 = time.perf_counter()
            k = sum(len(res) for res in p.predict_stream([pg] * steps))
            torch.cuda.synchronize()
            rates[name].append(k / (time.perf_counter() - t0))
    for name, p in pipes.items():
        say(f"{name}: stage {type(p.layout_task._stage).__name__}, {regions[name]} layout regions per step: {med(rates[name])} pages/s")
        p.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,stage,stream")
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17", "onnx_layout.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("onnx_layout_bench: no GPU -- nothing is measured without one")
    say(f"python tools/onnx_layout_bench.py --parts {a.parts} --pages {a.pages} --windows {a.windows}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    pages = torch.from_numpy(np.stack([make_page(i)[0] for i in range(a.pages)]))
    with tempfile.TemporaryDirectory() as tmp:
        d = export_standin(tmp)
        if "kernel" in parts:
            part_kernel(d, pages, a.windows)
        if "stage" in parts:
            part_stage(d, pages, a.windows)
        if "stream" in parts:
            part_stream(d, pages, a.windows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
