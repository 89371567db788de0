"""Times the generic ONNX executor's LSTM layer (pdf_table_amd/onnx_exec.py, csrc/lstm_op.hip) on the GPU -- a project tool, not a bench.py leg.

Two workloads at B = 256 lines, T = 80 steps (a mini-batch of 5120-px lines through MobileCrnn):
  * ``bare``: 2 x BiLSTM(48) on token rows [T, B, 40] (LstmOnly, two layers) -- the recurrent layers alone: per layer one row GEMM and one
    pt_op_lstm launch;
  * ``crnn``: the MobileCrnn graph (four convs, two pools, 2 x BiLSTM(48), Linear, Softmax) on [B, 3, 48, 64 T] images.
Yardstick: ``torch.nn.LSTM`` (MIOpen) on the same GPU for ``bare``, and the eager torch module for ``crnn``, in fp16 and fp32.

Method: every shape is warmed up (weights uploaded, HIP graph captured: run_device_graphed is what the recogniser door calls), then ``--steps``
calls are timed between two device events on the current stream, repeated ``--repeats`` times; the median and the spread (min .. max) of the
repeats are reported, engine and yardstick alternating within one process.  Outputs are compared with the fp32 module first (max |difference|
is printed): a fast wrong answer is not a result.  Algorithmic work of the recurrence: 2 * 4H * H * T * B * D FLOP per layer.

    python tools/onnx_lstm_bench.py [--steps 20] [--repeats 5] [--out profiles/r08/onnx_lstm.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def _time(fn, steps: int, repeats: int):
    """-> (median, min, max) milliseconds per call over `repeats` windows of `steps` calls, device events around each window"""
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("onnx_lstm_bench: no GPU (timings are taken on the device only)")
    import onnx_export as X
    import onnx_export_rnn as XR
    from pdf_table_amd import lib as L
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    B, T = args.batch, args.T
    dev = torch.device("cuda", 0)
    lines = [f"onnx_lstm_bench: B = {B}, T = {T}, {args.steps} calls per window, {args.repeats} windows (median, min .. max), {torch.cuda.get_device_name(0)}"]
    engines = {"bf16": HipEngine(0), "f16": HipEngine(0)}
    engines["f16"].set_precision(L.PT_PRECISION_F16)
    g = torch.Generator().manual_seed(1)
    bare = XR.seeded_rnn(XR.LstmOnly(40, 48, bidirectional=True, layers=2), 1)
    crnn = XR.seeded_rnn(XR.MobileCrnn(), 2)
    work = {"bare": (bare, torch.randn(B, 40, 1, T, generator=g)), "crnn": (crnn, torch.randn(B, 3, 48, 64 * T, generator=g) * 0.5)}
    flop_rec = 2 * (2 * 4 * 48 * 48 * T * B * 2)                       # two layers, two directions
    for name, (m, x) in work.items():
        data = X.torch_export(m, x[:2], dynamic_batch=True)
        with torch.no_grad():
            want = m(x[:8]).numpy()
        for prec in ("bf16", "f16", "bf16x3"):
            ex = HipGraphExecutor(data, engine=engines["f16" if prec == "f16" else "bf16"], precision=prec)
            err = float(np.abs(ex.run(x[:8].numpy())[0] - want).max())
            nhwc = x.permute(0, 2, 3, 1).contiguous().to(dev)
            nhwc = nhwc if prec == "bf16x3" else nhwc.to(ex.adt)
            for _ in range(3):                                     # eager, capture, replay
                ex.run_device_graphed(nhwc, x.shape[1])
            torch.cuda.synchronize()
            med, lo, hi = _time(lambda: ex.run_device_graphed(nhwc, x.shape[1]), args.steps, args.repeats)
            extra = f", recurrence {flop_rec / 1e9:.2f} GFLOP per call" if name == "bare" else ""
            lines.append(f"  {name:5s} engine {prec:7s}: {med:8.3f} ms per call ({lo:.3f} .. {hi:.3f}); {B / med * 1e3:10.0f} lines/s; max|d| vs fp32 module on 8 lines {err:.2e}{extra}")
        for dt in (torch.float16, torch.float32):
            mt = m.to(dev).to(dt)
            xt = x.to(dev).to(dt)
            with torch.no_grad():
                for _ in range(3):
                    mt(xt)
                torch.cuda.synchronize()
                med, lo, hi = _time(lambda: mt(xt), args.steps, args.repeats)
            lines.append(f"  {name:5s} torch  {str(dt).split('.')[-1]:7s}: {med:8.3f} ms per call ({lo:.3f} .. {hi:.3f}); {B / med * 1e3:10.0f} lines/s (eager module, nn.LSTM)")
            m.to("cpu").to(torch.float32)
    for e in engines.values():
        e.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
