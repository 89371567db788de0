"""SLANet on the engine, measured (profiles/r15/slanet.txt): one process, warm-up first, medians with ranges.

  head   pt_op_sla_decode at the model's sizes (N = 256 tokens, H = 256, C = 96, V = 50, L = 8, T = 501, eos_id = -1: every table walks all steps),
         B = 1 / 16 / 64, in bf16, f16 and the (hi | lo) pair mode -- against the SAME recurrence as per-step torch operators on the same GPU in the
         same 16-bit dtype (fp32 for the pair mode): the route a layer-by-layer executor would take, about 20 launches per step.  Both times, the ratio.
  door   tables per second through OcrTableStructureTask(model="SLANet").recognize_tables on the stand-in of tools/onnx_export_slanet.py
         (still a stand-in: the shipped PaddleOCR files are not available offline) at 488 x 488, T = 501, 64 tables per call.  The seeded head ends
         its walks after about ten steps (eos_id set), as a trained one does on small tables: the figure is the door's, not 501 steps per table.

    python tools/slanet_bench.py [out.txt]
"""
from __future__ import annotations

import os
import statistics
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd import weights as W  # noqa: E402
from pdf_table_amd.engine import HipEngine  # noqa: E402

N, H, C, V, LOC, T = 256, 256, 96, 50, 8, 501
DEV = torch.device("cuda", 0)


def timed(fn, warm=2, runs=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_walk(p, fea, steps):
    """the recurrence as per-step torch operators (what a layered route launches); p: tensors by role on the device, fea [B, N, C]"""
    B = fea.shape[0]
    Hh = p["h2h_w"].shape[0]
    P = fea @ p["i2h_w"].T
    h = torch.zeros(B, Hh, dtype=fea.dtype, device=fea.device)
    prev = torch.zeros(B, dtype=torch.long, device=fea.device)
    w_ctx, w_hot = p["w_ih"][:, :C].T.contiguous(), p["w_ih"][:, C:].T.contiguous()
    logits, locs = [], []
    for _ in range(steps):
        q = torch.addmm(p["h2h_b"], h, p["h2h_w"].T)
        e = torch.tanh(P + q[:, None, :]) @ p["score_w"]
        alpha = torch.softmax(e.float(), dim=1).to(fea.dtype)
        ctx = torch.bmm(alpha[:, None, :], fea)[:, 0]
        gi = torch.addmm(p["b_ih"], ctx, w_ctx) + w_hot[prev]
        gh = torch.addmm(p["b_hh"], h, p["w_hh"].T)
        r = torch.sigmoid(gi[:, :Hh] + gh[:, :Hh])
        z = torch.sigmoid(gi[:, Hh:2 * Hh] + gh[:, Hh:2 * Hh])
        c = torch.tanh(gi[:, 2 * Hh:] + r * gh[:, 2 * Hh:])
        h = (h - c) * z + c
        s = torch.addmm(p["s2_b"], torch.addmm(p["s1_b"], h, p["s1_w"].T), p["s2_w"].T)
        locs.append(torch.sigmoid(torch.addmm(p["l2_b"], torch.addmm(p["l1_b"], h, p["l1_w"].T), p["l2_w"].T)))
        logits.append(s)
        prev = s.argmax(1)
    return torch.softmax(torch.stack(logits, 1).float(), -1), torch.stack(locs, 1)


def head_bench(out):
    import slanet_ref as R
    p64 = R.make_head(1, H, C, V, LOC)
    out.append(f"== head: pt_op_sla_decode vs the same recurrence as per-step torch operators; N={N} H={H} C={C} V={V} L={LOC} T={T}, eos_id=-1; ms per call, "
               "median (min .. max) of 7 after 2 warm-up calls ==")
    for mode, prec, dt in (("bf16", L.PT_PRECISION_BF16, torch.bfloat16), ("f16", L.PT_PRECISION_F16, torch.float16), ("pairs", L.PT_PRECISION_BF16X3, torch.bfloat16)):
        eng = HipEngine(0)
        eng.set_precision(prec)
        split = mode == "pairs"
        w16, vec = W.pack_sla_head(p64, fmt="f16" if mode == "f16" else "bf16", split=split)
        d_w16, d_vec = torch.from_numpy(w16.view(np.int16)).to(DEV), torch.from_numpy(vec).to(DEV)
        tdt = torch.float32 if split else dt
        pt = {k: torch.from_numpy(np.asarray(v, np.float32)).to(DEV).to(tdt) for k, v in p64.items()}
        for B in (1, 16, 64):
            f32 = torch.from_numpy(R.make_fea(2, B, N, C).astype(np.float32))
            hi = f32.to(dt)
            fea = torch.cat([hi, (f32 - hi.float()).to(dt)], -1) if split else hi
            fea = fea.contiguous().to(DEV)
            scratch = torch.empty(eng.op_sla_scratch_bytes(B, N, H), dtype=torch.uint8, device=DEV)
            k = timed(lambda: eng.op_sla_decode(fea, C, d_w16, d_vec, H, V, LOC, T, split=split, scratch=scratch))
            ft = f32.to(DEV).to(tdt)
            t = timed(lambda: torch_walk(pt, ft, T), warm=1, runs=3)
            out.append(f"{mode:5s} B={B:3d}: kernel {k[0]:8.2f} ({k[1]:.2f} .. {k[2]:.2f})   torch per-step {t[0]:8.2f} ({t[1]:.2f} .. {t[2]:.2f}; 3 runs)   "
                       f"ratio {t[0] / k[0]:6.1f}x   {B * 1000.0 / k[0]:8.0f} tables/s of {T} steps")
        eng.close()


def door_bench(out):
    from onnx_export_slanet import SlaNetLike, export_slanet, seeded_slanet
    from pdf_table_amd.ocr_table_structure_task import OcrTableStructureTask
    from pdf_table_amd.rec_postprocess import TableLabelDecode
    from test_gpu_slanet_door import DICTS, crops
    d = tempfile.mkdtemp()
    dec = TableLabelDecode(os.path.join(DICTS, "table_structure_dict_ch.txt"), merge_no_span_structure=True)
    net = seeded_slanet(SlaNetLike(n_cls=50, n_loc=8, steps=T), 2, cell_ids=(dec.dict["<td"], dec.dict["<td></td>"]), cell_bias=9.0)
    with open(os.path.join(d, "model.onnx"), "wb") as f:
        f.write(export_slanet(net, 488))
    for name in os.listdir(DICTS):
        with open(os.path.join(DICTS, name), "rb") as src, open(os.path.join(d, name), "wb") as dst:
            dst.write(src.read())
    pages = torch.from_numpy(np.stack(crops(64, 300, 488, 3))).to(DEV)
    boxes = [np.array([[0, 0, 488, 300]])] * 64
    out.append("== door: OcrTableStructureTask(model='SLANet', lang='ch').recognize_tables, stand-in graph, 488 x 488, T = 501, 64 tables of 300 x 488 "
               "pixels per call; ms per call, median (min .. max) of 7 after 2 warm-up calls ==")
    for prec in ("bf16", "fp16", "fp32"):
        task = OcrTableStructureTask(model="SLANet", task_path=d, lang="ch", precision=prec)
        res = task.recognize_tables(pages, boxes)
        walked = [len(r[0]["structure_str_list"]) - 6 for r in res]
        m = timed(lambda: task.recognize_tables(pages, boxes))
        out.append(f"{prec:5s}: {m[0]:8.2f} ({m[1]:.2f} .. {m[2]:.2f})   {64 * 1000.0 / m[0]:8.0f} tables/s   tokens per table {min(walked)} .. {max(walked)}")


if __name__ == "__main__":
    lines = []
    head_bench(lines)
    door_bench(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)
