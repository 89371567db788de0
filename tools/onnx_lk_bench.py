"""Times the large-kernel convolution (csrc/large_conv.hip: pt_op_conv2d_large) on the shapes of the PP-OCRv4 server detector's LKPAN neck, and the
server-detector stand-in (tools/onnx_export_ppdet_server.py) end to end, on the GPU -- a project tool, not a bench.py leg.

1. Kernel, per shape and storage mode (bf16, f16, bf16x3): median and min .. max of the windows, the EXECUTED FLOP/s -- 2 B H W N kh kw Cin of the
   launched shape (N padded to the 64-channel tile as the executor pads it; three MFMA passes in bf16x3) over the median -- next to the 2.5 PFLOP/s
   dense bf16 MFMA peak of the MI355X (BASELINE.md's formula: FLOP x rate / peak), and torch's own F.conv2d (channels-last, the same 16-bit dtype, the
   same GPU) as the outside comparison.  The parent has no route for these layers, so there is no earlier time of this project's to compare with.
   The largest difference between the two 16-bit outputs is printed as a sanity figure.  Shapes, at a batch that makes a launch last about a millisecond or more:
     9x9 256 -> 64 on 240 x 240 and on 30 x 30, 9x9 64 -> 64 on 240 x 240, 7x7 and 7x1 32 -> 32 on 120 x 120.
2. Accuracy of HgnetLkpanDetLike on the [2, 3, 96, 128] input of tests/test_gpu_onnx_ppdet_server.py: max |d| against the fp32 module per mode, and of
   the layered torch module run in the same 16-bit dtype on the CPU (the figure the test's 16-bit bound is 4 times of).
3. End to end: HgnetLkpanDetLike(neck=256) -- the 256 -> 64 widths of the real neck -- on [16, 3, 960, 960] through run_device_graphed in the three
   modes, with the convolution FLOP per page counted from the module (whole graph, and the neck alone).

Method: every shape is warmed up; a window is ``--steps`` calls captured into one HIP graph and replayed between two device events, so the host's
launch cost is not in the figure; ``--repeats`` windows per variant, the variants alternating within one process; median and min .. max.

    python tools/onnx_lk_bench.py [--steps 10] [--repeats 7] [--out profiles/r12/onnx_lk.txt]
"""
from __future__ import annotations

import argparse
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from onnx_rect_bench import PEAK_BF16, _alternate, _time_eager, _window  # noqa: E402

#                kh kw  cin  n   H    W    B
KERNEL_SHAPES = [(9, 9, 256, 64, 240, 240, 4), (9, 9, 256, 64, 30, 30, 128), (9, 9, 64, 64, 240, 240, 8), (7, 7, 32, 32, 120, 120, 64),
                 (7, 1, 32, 32, 120, 120, 256)]


def kernel_table(engines, steps: int, repeats: int):
    from pdf_table_amd.weights import tile_conv_weight, tile_conv_weight_x3
    lines = [f"1. pt_op_conv2d_large on the neck's shapes ({steps} replayed calls per window, {repeats} windows each, alternating with torch's F.conv2d)"]
    for kh, kw, cin, n, H, W, B in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(cin + n + H + kh + kw)
        np_, cp = (n + 63) // 64 * 64, (cin + 63) // 64 * 64          # what the executor launches: channels padded to the 64-channel tile with zeros
        xf = torch.zeros(B, H, W, cp)
        xf[..., :cin] = torch.randn(B, H, W, cin, generator=g)
        w = torch.zeros(np_, cp, kh, kw)
        w[:n, :cin] = torch.randn(n, cin, kh, kw, generator=g) * (1.0 / (kh * kw * cin) ** 0.5)
        bias = torch.zeros(np_)
        bias[:n] = torch.randn(n, generator=g) * 0.2
        K = kh * kw * cp
        flop = 2.0 * B * H * W * np_ * K
        lines.append(f"  {kh}x{kw} {cin} -> {n} on {H} x {W}, B = {B} (launched {cp} -> {np_}: {flop / 1e9:.1f} GFLOP per pass, {2.0 * B * H * W * n * kh * kw * cin / 1e9:.1f} of them on real channels)")
        for mode in ("bf16", "f16", "bf16x3"):
            eng = engines["f16" if mode == "f16" else "bf16"]
            dev, dt = eng._tdev, (torch.float16 if mode == "f16" else torch.bfloat16)
            split = mode == "bf16x3"
            hi = xf.to(dt)
            x = (torch.cat([hi, (xf - hi.float()).to(dt)], -1) if split else hi).contiguous().to(dev)
            tiles = tile_conv_weight_x3(w) if split else tile_conv_weight(w, "f16" if mode == "f16" else "bf16")
            wt = torch.from_numpy(np.ascontiguousarray(tiles).view(np.int16)).to(dev)
            bd = bias.to(dev)
            new = lambda: eng.op_conv2d_large(x, wt, bd, kh, kw, act=1, split=int(split))      # noqa: E731
            xt = hi.to(dev).permute(0, 3, 1, 2)                                                  # NCHW view of the NHWC memory: channels-last
            wt_t = w.to(dt).to(dev).contiguous(memory_format=torch.channels_last)
            bt = bias.to(dt).to(dev)
            ref = lambda: torch.relu(F.conv2d(xt, wt_t, bt, 1, (kh // 2, kw // 2)))              # noqa: E731
            agree = ""
            if not split:
                a, b_ = new().float(), ref().permute(0, 2, 3, 1).float()
                torch.cuda.synchronize()
                # a sanity figure, not a check: the kernel is held to a float64 reference in tests/test_gpu_large_conv_ops.py; the library's
                # result is a 16-bit value of its own rounding, so the two differ by units in the last place of the output's scale
                agree = f"; max|d| against F.conv2d {float((a - b_).abs().max()):.2e} at an output scale of {float(b_.abs().max()):.1f}"
                del a, b_
            try:
                torch_window = _window(ref, steps)
            except Exception:      # noqa: BLE001 -- a library convolution that cannot be captured is timed eagerly: the yardstick then includes its launches
                torch.cuda.synchronize()
                torch_window = lambda: _time_eager(ref, steps, 1)[0]      # noqa: E731
            t = _alternate({"new": _window(new, steps), "torch": torch_window}, repeats)
            passes = 3 if split else 1
            rate = passes * flop / (t["new"][0] * 1e-3)
            lines.append(f"    {mode:7s}: {t['new'][0]:8.3f} ms ({t['new'][1]:.3f} .. {t['new'][2]:.3f}); {rate / 1e15:6.3f} PFLOP/s executed = {100 * rate / PEAK_BF16:5.1f} % of the "
                         f"2.5 PFLOP/s bf16 peak; torch F.conv2d in {str(dt).split('.')[-1]}: {t['torch'][0]:8.3f} ms ({t['torch'][1]:.3f} .. {t['torch'][2]:.3f}){agree}")
            del x, wt, xt, wt_t
            torch.cuda.empty_cache()
    return lines


def _conv_flop(m: nn.Module, x: torch.Tensor):
    """convolution FLOP of one forward pass per image, {module: FLOP}, from forward hooks"""
    out = {}

    def hook(mod, _inp, y):
        w = mod.weight
        out[mod] = out.get(mod, 0.0) + 2.0 * y.numel() / y.shape[0] * (w[0].numel() if isinstance(mod, nn.Conv2d) else w.shape[0])      # a 2x2 / stride-2 transposed convolution: one tap per output pixel
    hs = [c.register_forward_hook(hook) for c in m.modules() if isinstance(c, (nn.Conv2d, nn.ConvTranspose2d))]
    with torch.no_grad():
        m(x)
    for h in hs:
        h.remove()
    return out


def accuracy(engines):
    import onnx_export_ppdet_server as S
    from oracle import db_pre
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    from pdf_table_amd.synth_pages import make_page
    pages = [make_page(2)[0][:96, :128].copy(), make_page(3)[0][200:296, 100:228].copy()]
    pix = torch.from_numpy(np.stack([db_pre.preprocess_db_pp(p)[0] for p in pages]))
    m = S.seeded_ppdet_server(S.HgnetLkpanDetLike(), 7, example=pix, blob_map=True)
    blob = S.torch_export(m, torch.zeros(1, 3, 64, 64))
    lines = ["2. HgnetLkpanDetLike (seed 7, blob_map) on [2, 3, 96, 128]: max |d| of the probability map against the fp32 module"]
    with torch.no_grad():
        want = m(pix).numpy()
        for prec, dt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("bf16x3", None)):
            ex = HipGraphExecutor(blob, engine=engines["f16" if prec == "f16" else "bf16"], precision=prec)
            err = float(np.abs(ex.run(pix.numpy())[0] - want).max())
            cpu = "" if dt is None else f"; the layered torch module in {str(dt).split('.')[-1]} on the CPU: {float(np.abs(copy.deepcopy(m).to(dt)(pix.to(dt)).float().numpy() - want).max()):.3e}"
            lines.append(f"  engine {prec:7s}: {err:.3e}{cpu}")
    return lines


def end_to_end(engines, B: int, steps: int, repeats: int):
    import onnx_export_ppdet_server as S
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    g = torch.Generator().manual_seed(1)
    m = S.seeded_ppdet_server(S.HgnetLkpanDetLike(neck=256), 1)
    small = torch.randn(1, 3, 96, 128, generator=g)
    fl = _conv_flop(m, small)
    scale = 960 * 960 / (96 * 128)          # every layer's output scales with the page (sizes are multiples of 32)
    neck_mods = {c for part in (m.ins, m.inp, m.pan_head, m.pan_lat, m.incl) for c in part.modules()}
    total, neck = sum(fl.values()) * scale, sum(v for k, v in fl.items() if k in neck_mods) * scale
    large = sum(v for k, v in fl.items() if isinstance(k, nn.Conv2d) and k.groups == 1 and max(k.kernel_size) >= 5) * scale
    lines = [f"3. HgnetLkpanDetLike(neck=256) on [{B}, 3, 960, 960] through run_device_graphed ({steps} calls per window, {repeats} windows): {total / 1e9:.1f} GFLOP of "
             f"convolutions per page, {neck / 1e9:.1f} of them in the LKPAN neck, {large / 1e9:.1f} in kernels with a side of 5 or more (real channels)"]
    blob = S.torch_export(m, torch.zeros(1, 3, 64, 64))
    x = torch.randn(B, 3, 960, 960, generator=g) * 0.5
    for prec in ("bf16", "f16", "bf16x3"):
        ex = HipGraphExecutor(blob, engine=engines["f16" if prec == "f16" else "bf16"], precision=prec)
        nhwc = x.permute(0, 2, 3, 1).contiguous().to(ex.eng._tdev)
        nhwc = nhwc if prec == "bf16x3" else nhwc.to(ex.adt)
        for _ in range(3):                                     # eager, capture, replay
            ex.run_device_graphed(nhwc, 3)
        torch.cuda.synchronize()
        med, lo, hi = _time_eager(lambda: ex.run_device_graphed(nhwc, 3), steps, repeats)
        lines.append(f"  engine {prec:7s}: {med:8.2f} ms per call ({lo:.2f} .. {hi:.2f}); {B / med * 1e3:7.1f} pages/s; {total * B / med * 1e3 / 1e12:6.1f} TFLOP/s of real-channel "
                     f"convolution work = {100 * total * B / (med * 1e-3) / PEAK_BF16:.1f} % of the bf16 peak (a whole-graph rate, not a kernel's)")
        del ex, nhwc
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--only", choices=["kernel", "accuracy", "e2e"], default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "onnx_lk.txt"), help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("onnx_lk_bench: no GPU (timings are taken on the device only)")
    from pdf_table_amd import lib as L
    from pdf_table_amd.engine import HipEngine
    engines = {"bf16": HipEngine(0), "f16": HipEngine(0)}
    engines["f16"].set_precision(L.PT_PRECISION_F16)
    lines = [f"onnx_lk_bench: {torch.cuda.get_device_name(0)}"]
    if args.only in (None, "kernel"):
        lines += kernel_table(engines, args.steps, args.repeats)
    if args.only in (None, "accuracy"):
        lines += accuracy(engines)
    if args.only in (None, "e2e"):
        lines += end_to_end(engines, args.batch, args.steps, args.repeats)
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
