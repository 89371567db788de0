"""Text lines -> cells on the device (pt_op_table_match), measured (profiles/r16/table_match.txt): one process, warm-up first, medians with ranges of 7.

  kernel  pt_op_table_match at the model's sizes: T = 501 rows, L = 8, 64 tables per call, 30 and 100 lines per table, about 60 % of the rows cells
          (a dense table: ~300 cells).  Device events around 20 back-to-back calls; ms per call.
  host    the numpy route on the same inputs: filter_lines + match_result (pdf_table_amd/table_structure_match.py) per table, polygons already built;
          ms per table and per 64 tables.
  stage   SlaNetStage.__call__ on the stand-in graph (tools/onnx_export_slanet.py; 488 x 488, T = 501, lang ch, 64 tables of 300 x 488 pixels per
          call) without text_boxes, with them (the kernel behind the head, its result on the stage's copy), and without them followed by the host
          match on the results -- what a host route would cost.  The three alternate inside each repeat.  The seeded head ends its walks after about
          ten steps, so a table has few cells here: the host match is at its cheapest.

    python tools/table_match_bench.py [out.txt]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pdf_table_amd import table_structure_match as M  # noqa: E402
from pdf_table_amd.engine import HipEngine  # noqa: E402

B, T, LOC, V = 64, 501, 8, 50
CELL_IDS = (5, 7)
DEV = torch.device("cuda", 0)
RUNS = 7


def stats(v):
    return f"{statistics.median(v):9.4f} ({min(v):.4f} .. {max(v):.4f})"


def inputs(n_lines, seed):
    g = np.random.default_rng(seed)
    xy = g.uniform(0.0, 0.9, (B, T, 1, 2))
    wh = g.uniform(0.01, 0.1, (B, T, 1, 2))
    corners = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)[None, None]
    loc = (xy + wh * corners).reshape(B, T, LOC).astype(np.float32)
    others = [i for i in range(1, V - 1) if i not in CELL_IDS]
    ids = np.where(g.uniform(size=(B, T)) < 0.6, g.choice(CELL_IDS, (B, T)), g.choice(others, (B, T))).astype(np.int32)
    steps = np.full(B, T, np.int32)
    frames = np.tile(np.array([[488, 300, 12, 34]], np.float32), (B, 1))
    lxy = np.stack([g.integers(12, 440, B * n_lines), g.integers(34, 310, B * n_lines)], 1)
    lines = np.concatenate([lxy, lxy + np.stack([g.integers(10, 60, B * n_lines), g.integers(8, 24, B * n_lines)], 1)], 1).astype(np.float32)
    offsets = (np.arange(B + 1) * n_lines).astype(np.int32)
    return loc, ids, steps, frames, lines, offsets


def polygons(loc, ids, frame):
    rows = np.flatnonzero(np.isin(ids, CELL_IDS))
    p = loc[rows].copy()
    p[:, 0::2] *= float(frame[0])
    p[:, 1::2] *= float(frame[1])
    return p + np.tile(frame[2:4], 4)[None], rows


def kernel_and_host(out):
    eng = HipEngine(0)
    flags = np.zeros(V, np.uint8)
    flags[list(CELL_IDS)] = 1
    out.append(f"== kernel vs host: T={T} L={LOC} {B} tables per call, ~60 % of the rows cells; median (min .. max) of {RUNS} ==")
    for n_lines in (30, 100):
        loc, ids, steps, frames, lines, offsets = inputs(n_lines, n_lines)
        d = [torch.from_numpy(a).to(DEV) for a in (loc, ids, steps, flags, frames, lines, offsets)]
        call = lambda: eng.op_table_match(*d)
        got = call().cpu().numpy()
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
        polys = [polygons(loc[b], ids[b], frames[b]) for b in range(B)]
        lb = lines.astype(np.float64)
        host_ms, same = [], True
        for r in range(RUNS + 1):
            t0 = time.perf_counter()
            for b in range(B):
                mine = lb[offsets[b]:offsets[b + 1]]
                kept = M.filter_lines(polys[b][0], mine)
                m = M.match_result(mine[kept], polys[b][0])
                if r == 0:                                           # the first pass checks the kernel and is not timed
                    want = np.full(len(mine), -1, np.int32)
                    for c, ls in m.items():
                        want[kept[ls]] = polys[b][1][c]
                    same = same and np.array_equal(want, got[offsets[b]:offsets[b + 1]])
            if r:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        cells = np.mean([len(p[0]) for p in polys])
        out.append(f"{n_lines:3d} lines per table ({cells:.0f} cells per table): kernel {stats(ms)} ms per call of {B} tables   host {stats([h / B for h in host_ms])} ms "
                   f"per table = {statistics.median(host_ms):8.2f} ms per {B} tables   ratio {statistics.median(host_ms) / statistics.median(ms):7.1f}x   "
                   f"results {'equal' if same else 'DIFFER'}")
    eng.close()


def stage_bench(out):
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
    pages = torch.from_numpy(np.stack(crops(B, 300, 488, 3))).to(DEV)
    boxes = [np.array([[0, 0, 488, 300]])] * B
    task = OcrTableStructureTask(model="SLANet", task_path=d, lang="ch", precision="bf16")
    stage = task._stage
    out.append(f"== stage: SlaNetStage.__call__, stand-in graph, 488 x 488, T = {T}, {B} tables of 300 x 488 pixels per call, bf16; ms per call (host clock, the call "
               f"ends in the wait for its copy), median (min .. max) of {RUNS}, the three routes alternating ==")
    for n_lines in (30, 100):
        g = np.random.default_rng(n_lines)
        tbx = []
        for _ in range(B):
            xy = np.stack([g.integers(0, 420, n_lines), g.integers(0, 270, n_lines)], 1)
            tbx.append(np.concatenate([xy, xy + np.stack([g.integers(10, 60, n_lines), g.integers(8, 24, n_lines)], 1)], 1).astype(np.float64))

        def plain():
            return stage(pages, boxes, page_frame=True)

        def device():
            return stage(pages, boxes, page_frame=True, text_boxes=tbx)

        def host():
            res = stage(pages, boxes, page_frame=True)
            for page, lb in zip(res, tbx):
                for t in page:
                    cells = np.asarray(t["polygons"])
                    if cells.ndim == 2 and len(cells):
                        kept = M.filter_lines(cells, lb)
                        t["matched"] = M.match_result(lb[kept], cells)
            return res

        for fn in (plain, device, host):
            fn(), fn()
        ncell = [len(t["polygons"]) for page in device() for t in page]
        ms = {"plain": [], "device": [], "host": []}
        for _ in range(RUNS):
            for name, fn in (("plain", plain), ("device", device), ("host", host)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        out.append(f"{n_lines:3d} lines per table (cells per table {min(ncell)} .. {max(ncell)}): without text_boxes {stats(ms['plain'])}   with text_boxes (kernel) "
                   f"{stats(ms['device'])}   without + host match {stats(ms['host'])}")


if __name__ == "__main__":
    lines = []
    kernel_and_host(lines)
    stage_bench(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)
