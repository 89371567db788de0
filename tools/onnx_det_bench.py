"""Times the two kernels of csrc/det_ops.hip and the detector-shaped graph that uses them on the GPU -- a project tool, not a bench.py leg.

1. The DB head's tail alone, [64, 240, 240, 24 -> 24 -> 1] (64 pages of a 960 x 960 net input), bf16 and bf16x3: the fused launch (pt_op_db_tail) against
   the layered route on the same operands -- two pt_op_conv2d pixel-shuffle GEMMs, pt_op_act (sigmoid) over the [64, 960, 960, 64] map and the
   strided slice of channel 0.  The two outputs are compared first.  Bytes the fused launch needs: the input rows as stored (64 channels of 2 bytes,
   twice that in the pair mode) + one fp32 per output pixel; GB/s = those bytes over the median time, next to the 8 TB/s HBM3E peak of the MI355X
   (about 6.3 TB/s is what a plain copy reaches).
2. ``LcnetV3DetLike`` (tools/onnx_export_ppdet.py) on [B, 3, 960, 960] through run_device_graphed, ``fuse_db_tail`` off and on, bf16.
3. pt_op_affine_act on [64, 240, 240, 96] (rows of 128 channels), bf16: read + write of the stored rows over the median time.

Method: every shape is warmed up; a window is ``--steps`` calls captured into one HIP graph and replayed between two device events, so the host's
launch cost is not in the figure; ``--repeats`` windows per variant, the variants alternating within one process; median and min .. max.  The condition
on step 1 is that the fused tail is faster than the layered route in every timed window; where it is not, the tool says so and exits non-zero.

    python tools/onnx_det_bench.py [--steps 10] [--repeats 7] [--out profiles/r10/onnx_det.txt]
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

from onnx_rect_bench import _alternate, _time_eager, _window  # noqa: E402

PEAK_HBM = 8.0e12           # HBM3E peak, bytes/s


def _tiles(w, split):
    from pdf_table_amd.weights import tile_conv_weight, tile_conv_weight_x3
    t = tile_conv_weight_x3(w) if split else tile_conv_weight(w)
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int16))


def tail_table(B: int, H: int, steps: int, repeats: int):
    from pdf_table_amd import lib as L
    from pdf_table_amd.engine import HipEngine
    dev = torch.device("cuda", 0)
    C = C1 = 24
    failed = []
    lines = [f"1. the DB head's tail, [{B}, {H}, {H}, {C} -> {C1} -> 1] -> [{B}, {4 * H}, {4 * H}] ({steps} replayed calls per window, {repeats} windows each, alternating)"]
    for prec in ("bf16", "bf16x3"):
        split = prec == "bf16x3"
        eng = HipEngine(0)
        eng.set_precision(L.PT_PRECISION_BF16X3 if split else L.PT_PRECISION_BF16)
        g = torch.Generator().manual_seed(24)
        xf = torch.zeros(B, H, H, 64)
        xf[..., :C] = torch.randn(B, H, H, C, generator=g)
        hi = xf.to(torch.bfloat16)
        x = (torch.cat([hi, (xf - hi.float()).to(torch.bfloat16)], -1) if split else hi).contiguous().to(dev)
        w1, b1 = torch.randn(C, C1, 2, 2, generator=g) * (1.0 / C) ** 0.5, torch.randn(C1, generator=g) * 0.2
        w2, b2 = torch.randn(C1, 1, 2, 2, generator=g) * (2.0 / C1) ** 0.5, torch.randn(1, generator=g) * 0.2
        dw = [t.to(dev) for t in (w1, b1, w2, b2)]

        def pack(w, b):
            ci, co = w.shape[:2]
            wq = torch.zeros(2, 2, 64, 64)
            wq[:, :, :co, :ci] = w.permute(2, 3, 1, 0)
            bq = torch.zeros(64)
            bq[:co] = b
            return _tiles(wq.reshape(256, 64, 1, 1), split).to(dev), bq.repeat(4).to(dev)
        (t1, q1), (t2, q2) = pack(w1, b1), pack(w2, b2)

        def fused():
            return eng.op_db_tail(x, C, *dw, split=split)

        def layered():
            h = eng.op_conv2d(x, t1, q1, 1, 1, relu=1, shuffle_cout=64, split=int(split))
            p = eng.op_act(eng.op_conv2d(h, t2, q2, 1, 1, relu=0, shuffle_cout=64, split=int(split)), 4, split=split)
            v = p[..., 0].float()
            return (v + p[..., 64].float()) if split else v.clone()          # values(a)[..., 0].clone() of the detection task
        a, b_ = fused()[..., 0], layered()
        torch.cuda.synchronize()
        d = float((a - b_).abs().max())
        ok = a.shape == b_.shape and d <= (2.0 ** -14 if split else 2.0 ** -8) * 8          # the layered route's 16-bit roundings (tests/test_gpu_det_ops.py has the bound)
        t = _alternate({"fused": _window(fused, steps), "layered": _window(layered, steps)}, repeats)
        nbytes = x.numel() * 2 + a.numel() * 4
        rate = nbytes / (t["fused"][0] * 1e-3)
        faster = t["fused"][2] < t["layered"][1]
        if not faster or not ok:
            failed.append(prec)
        lines.append(f"  {prec:6s}: fused {t['fused'][0]:7.3f} ms ({t['fused'][1]:.3f} .. {t['fused'][2]:.3f}); layered {t['layered'][0]:7.3f} ms ({t['layered'][1]:.3f} .. "
                     f"{t['layered'][2]:.3f}); ratio of medians {t['layered'][0] / t['fused'][0]:.1f}x; {'every fused window below every layered window' if faster else 'NOT FASTER in every window'}; "
                     f"fused: {nbytes / 1e6:.0f} MB needed -> {rate / 1e9:.0f} GB/s = {100 * rate / PEAK_HBM:.0f} % of the 8 TB/s HBM peak; outputs agree: {ok} (max|d| {d:.2e})")
        del x
        eng.close()
        torch.cuda.empty_cache()
    return lines, failed


def graph_table(B: int, S: int, steps: int, repeats: int):
    import onnx_export_ppdet as D
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    dev = torch.device("cuda", 0)
    eng = HipEngine(0)
    m = D.seeded_ppdet(D.LcnetV3DetLike(), 3)
    data = D.torch_export(m, torch.zeros(1, 3, 64, 64))
    x = torch.randn(B, S, S, 3, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)      # the distribution the stand-in was scaled on
    lines = [f"2. LcnetV3DetLike on [{B}, 3, {S}, {S}], bf16, run_device_graphed ({steps} calls per window, {repeats} windows)"]
    res = {}
    for fuse in (False, True):
        ex = HipGraphExecutor(data, engine=eng, precision="bf16", fuse_db_tail=fuse)
        for _ in range(3):                                     # eager, capture, replay
            (a,) = ex.run_device_graphed(x, 3)
        torch.cuda.synchronize()
        res[fuse] = ex.values(a)[..., 0].float().clone()
        med, lo, hi = _time_eager(lambda: ex.run_device_graphed(x, 3), steps, repeats)
        lines.append(f"  fuse_db_tail={str(fuse):5s}: {med:8.2f} ms per call ({lo:.2f} .. {hi:.2f}); {B / med * 1e3:7.0f} pages/s; {len(ex.layers)} layers")
        del ex
        torch.cuda.empty_cache()
    d = (res[True] - res[False]).abs()
    lines.append(f"  |fused - layered| on the probability map (bf16; the layered route rounds the 24-channel intermediate and the probability to 8 bits): mean {float(d.mean()):.2e}, "
                 f"99.9th percentile {float(d.flatten()[::97].float().quantile(0.999)):.2e}, max {float(d.max()):.2e}; probabilities above 0.3: {100 * float((res[False] > 0.3).float().mean()):.1f} %")
    eng.close()
    return lines


def affine_table(B: int, H: int, steps: int, repeats: int):
    from pdf_table_amd.engine import HipEngine
    dev = torch.device("cuda", 0)
    eng = HipEngine(0)
    C, cp = 96, 128
    x = torch.zeros(B, H, H, cp)
    x[..., :C] = torch.randn(B, H, H, C, generator=torch.Generator().manual_seed(2))
    x = x.to(torch.bfloat16).to(dev)
    vec = [torch.full((cp,), v, device=dev) for v in (1.1, 0.1, 0.9, -0.1)]
    fn = lambda: eng.op_affine_act(x, C, vec[0], vec[1], 2, vec[2], vec[3])      # noqa: E731
    t = _alternate({"affine": _window(fn, steps)}, repeats)["affine"]
    nbytes = 2 * x.numel() * 2
    eng.close()
    return [f"3. pt_op_affine_act (hardswish) on [{B}, {H}, {H}, {C}] in rows of {cp}, bf16: {t[0] * 1e3:.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f}); "
            f"{nbytes / 1e6:.0f} MB read + written -> {nbytes / (t[0] * 1e-3) / 1e9:.0f} GB/s = {100 * nbytes / (t[0] * 1e-3) / PEAK_HBM:.0f} % of the 8 TB/s HBM peak"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=960, help="net input side of the detector (the tail then runs on size / 4)")
    ap.add_argument("--only", choices=["tail", "graph", "affine"], default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "onnx_det.txt"), help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("onnx_det_bench: no GPU (timings are taken on the device only)")
    lines = [f"onnx_det_bench: {torch.cuda.get_device_name(0)}"]
    failed = []
    if args.only in (None, "tail"):
        tab, failed = tail_table(args.batch, args.size // 4, args.steps, args.repeats)
        lines += tab
    if args.only in (None, "graph"):
        lines += graph_table(args.batch, args.size, args.steps, args.repeats)
    if args.only in (None, "affine"):
        lines += affine_table(args.batch, args.size // 4, args.steps, args.repeats)
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(report + "\n")
    if failed:
        raise SystemExit("onnx_det_bench: the fused tail is not faster than the layered route in every window, or disagrees with it, in: " + ", ".join(failed))


if __name__ == "__main__":
    main()
