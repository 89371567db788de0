"""Times the per-axis convolution kernel (csrc/rect_ops.hip: pt_op_conv2d_rect) and the recogniser-shaped graphs that use it on the GPU -- a project
tool, not a bench.py leg.

1. Kernel against the way the same result had to be computed before (entry points that predate ABI 18), on the same operands, B = 64 lines:
     stride (2,1):  pt_op_conv2d 3x3 / stride 1, then every other row dropped with a strided copy;
     [1,3] kernel:  pt_op_conv2d 3x3 whose first and last tap rows are zero.
   Shapes a recogniser batch runs: (3,3,2,1) 128 -> 128 on 24 x 160 and 256 -> 256 on 12 x 160, [1,3] 512 -> 64 and 1024 -> 64 on 1 x 40.  The two
   outputs are compared first (bf16: each is within 2^-8 |ref| + 4 K 2^-24 S of the exact sum, so they differ by at most twice that).  FLOP/s is
   the executed shape's 2 B Ho Wo N kh kw Cin over the median time, next to the 2.5 PFLOP/s dense bf16 MFMA peak of the MI355X.
2. End to end: SvtrLcnetRecLike and MobileV3RecLike (tools/onnx_export_pprec.py) on [256, 3, 48, 320] in bf16, f16 and bf16x3 through
   run_device_graphed (what the recogniser door calls), max |difference| against the fp32 module on 8 lines, the eager torch module as a yardstick.

Method: every shape is warmed up; a window is ``--steps`` calls captured into one HIP graph and replayed between two device events, so the host's
launch cost is not in the figure; ``--repeats`` windows per variant, the variants alternating within one process; median and min .. max.  A shape on which the new
kernel's median is not below every baseline window, or whose outputs disagree, is listed and the tool exits non-zero: it belongs on the square-kernel route.

    python tools/onnx_rect_bench.py [--steps 20] [--repeats 7] [--out profiles/r09/onnx_rect.txt]
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

PEAK_BF16 = 2.5e15          # dense bf16 MFMA peak, FLOP/s


def _window(fn, steps: int):
    """`steps` calls of fn captured into one HIP graph -> a function that replays it and returns the milliseconds per call"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            fn()
    g.replay()
    torch.cuda.synchronize()

    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps
    return run


def _alternate(windows: dict, repeats: int):
    """{name: window} -> {name: (median, min, max)}, one window of each per round"""
    ms = {k: [] for k in windows}
    for _ in range(repeats):
        for k, w in windows.items():
            ms[k].append(w())
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def _time_eager(fn, steps: int, repeats: int):
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


KERNEL_SHAPES = [((3, 3, 2, 1), 128, 128, 24, 160), ((3, 3, 2, 1), 256, 256, 12, 160), ((1, 3, 1, 1), 512, 64, 1, 40), ((1, 3, 1, 1), 1024, 64, 1, 40)]


def kernel_table(eng, B: int, steps: int, repeats: int):
    from pdf_table_amd.weights import tile_conv_weight
    dev = eng._tdev
    failed = []
    lines = [f"1. pt_op_conv2d_rect against the square-kernel route, bf16, B = {B} ({steps} replayed calls per window, {repeats} windows each, alternating)"]
    for (kh, kw, sh, sw), cin, n, H, W in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(cin + n + H)
        x = torch.randn(B, H, W, cin, generator=g).to(torch.bfloat16).to(dev)
        w = torch.randn(n, cin, kh, kw, generator=g) * (1.0 / (kh * kw * cin) ** 0.5)
        bias = (torch.randn(n, generator=g) * 0.2).to(dev)
        w33 = torch.zeros(n, cin, 3, 3)
        w33[:, :, (3 - kh) // 2:(3 - kh) // 2 + kh, (3 - kw) // 2:(3 - kw) // 2 + kw] = w
        up = lambda t: torch.from_numpy(np.ascontiguousarray(tile_conv_weight(t)).view(np.int16)).to(dev)
        wt, wt33 = up(w), up(w33)
        new = lambda: eng.op_conv2d_rect(x, wt, bias, kh, kw, sh, sw, act=1)
        if (sh, sw) == (1, 1):
            base = lambda: eng.op_conv2d(x, wt33, bias, 3, 1, relu=1)
            how = "3x3 with zero taps"
        else:
            base = lambda: eng.op_conv2d(x, wt33, bias, 3, 1, relu=1)[:, ::sh, ::sw].contiguous()
            how = "3x3 / stride 1 + strided copy"
        a, b_ = new().float(), base().float()
        torch.cuda.synchronize()
        K = kh * kw * cin
        S = float(x.float().abs().max()) * float(w.abs().max())
        d = (a - b_).abs()
        tol = 2 * (2.0 ** -8 * b_.abs() + 4 * K * 2.0 ** -24 * S)
        ok = bool((d <= tol).all()) and a.shape == b_.shape
        t = _alternate({"new": _window(new, steps), "base": _window(base, steps)}, repeats)
        Ho, Wo = a.shape[1], a.shape[2]
        flop = 2.0 * B * Ho * Wo * n * K
        rate = flop / (t["new"][0] * 1e-3)
        # the bar: the new kernel's median below the fastest of the baseline's windows, i.e. below its median by more than its spread
        verdict = "every window faster" if t["new"][2] < t["base"][1] else ("median below the baseline's spread" if t["new"][0] < t["base"][1] else "NOT FASTER")
        if verdict == "NOT FASTER" or not ok:
            failed.append(f"({kh},{kw},{sh},{sw}) {cin} -> {n} on {H} x {W}")
        lines.append(f"  ({kh},{kw},{sh},{sw}) {cin:4d} -> {n:3d} on {H:2d} x {W}: rect {t['new'][0] * 1e3:8.1f} us ({t['new'][1] * 1e3:.1f} .. {t['new'][2] * 1e3:.1f}); "
                     f"{how} {t['base'][0] * 1e3:8.1f} us ({t['base'][1] * 1e3:.1f} .. {t['base'][2] * 1e3:.1f}); {verdict}; "
                     f"{rate / 1e12:6.1f} TFLOP/s executed = {100 * rate / PEAK_BF16:.1f} % of the 2.5 PFLOP/s bf16 peak; outputs agree: {ok} (max|d| {float(d.max()):.2e})")
    lines.append("  speed bar (rect median below every baseline window): " + ("met on every shape" if not failed else "MISSED on " + "; ".join(failed) +
                                                                                " -- dispatch these shapes to the square-kernel route in onnx_exec._conv"))
    return lines, failed


def end_to_end(B: int, steps: int, repeats: int):
    import onnx_export as X
    import onnx_export_pprec as P
    from pdf_table_amd import lib as L
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    dev = torch.device("cuda", 0)
    engines = {"bf16": HipEngine(0), "f16": HipEngine(0)}
    engines["f16"].set_precision(L.PT_PRECISION_F16)
    lines = [f"2. end to end on [{B}, 3, 48, 320] (run_device_graphed; {steps} calls per window, {repeats} windows)"]
    g = torch.Generator().manual_seed(1)
    for name, m in (("SvtrLcnetRecLike", P.seeded_pprec(P.SvtrLcnetRecLike(), 3, head_scale=6.0)), ("MobileV3RecLike", P.seeded_pprec(P.MobileV3RecLike(), 2))):
        x = torch.randn(B, 3, 48, 320, generator=g) * 0.5
        data = X.torch_export(m, x[:2], dynamic_batch=True)
        with torch.no_grad():
            want = m(x[:8]).numpy()
        for prec in ("bf16", "f16", "bf16x3"):
            ex = HipGraphExecutor(data, engine=engines["f16" if prec == "f16" else "bf16"], precision=prec)
            err = float(np.abs(ex.run(x[:8].numpy())[0] - want).max())
            nhwc = x.permute(0, 2, 3, 1).contiguous().to(dev)
            nhwc = nhwc if prec == "bf16x3" else nhwc.to(ex.adt)
            for _ in range(3):                                     # eager, capture, replay
                ex.run_device_graphed(nhwc, 3)
            torch.cuda.synchronize()
            med, lo, hi = _time_eager(lambda: ex.run_device_graphed(nhwc, 3), steps, repeats)
            lines.append(f"  {name:16s} engine {prec:7s}: {med:8.3f} ms per call ({lo:.3f} .. {hi:.3f}); {B / med * 1e3:9.0f} lines/s; max|d| vs fp32 module on 8 lines {err:.2e} "
                         f"(output scale {float(np.abs(want).max()):.2f})")
            del ex
        for dt in (torch.float16, torch.float32):
            mt, xt = m.to(dev).to(dt), x.to(dev).to(dt)
            with torch.no_grad():
                for _ in range(3):
                    mt(xt)
                torch.cuda.synchronize()
                med, lo, hi = _time_eager(lambda: mt(xt), steps, repeats)
            lines.append(f"  {name:16s} torch  {str(dt).split('.')[-1]:7s}: {med:8.3f} ms per call ({lo:.3f} .. {hi:.3f}); {B / med * 1e3:9.0f} lines/s (eager module: a yardstick only)")
            m.to("cpu").to(torch.float32)
    for e in engines.values():
        e.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--kernel-batch", type=int, default=64)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", choices=["kernel", "e2e"], default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "onnx_rect.txt"), help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("onnx_rect_bench: no GPU (timings are taken on the device only)")
    from pdf_table_amd.engine import HipEngine
    lines = [f"onnx_rect_bench: {torch.cuda.get_device_name(0)}"]
    failed = []
    if args.only in (None, "kernel"):
        eng = HipEngine(0)
        tab, failed = kernel_table(eng, args.kernel_batch, args.steps, args.repeats)
        lines += tab
        eng.close()
    if args.only in (None, "e2e"):
        lines += end_to_end(args.batch, args.steps, args.repeats)
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")
    if failed:
        raise SystemExit("onnx_rect_bench: pt_op_conv2d_rect is slower than the square-kernel route, or disagrees with it, on: " + "; ".join(failed))


if __name__ == "__main__":
    main()
