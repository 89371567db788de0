"""Lore text lines -> cells on the device (pt_op_lore_match), measured (profiles/r19/lore_match.txt): one process, warm-up first, medians with ranges of 7.

  kernel  pt_op_lore_match at 64 tables of 300 cells per call, 30 and 100 lines per table.  Device events around 20 back-to-back calls; ms per call.
  host    find_top1_match (numpy) over the same 64 tables, cell boxes already built (the sort and the cell objects are not timed); results
          asserted equal to the kernel's.
  stage   TsrStage process + collect + HTML for one call of 64 tables (start() queued and finished before the clock starts), 30 seeded lines per
          table, with match= (kernel behind the processor, page_table_html(matched=...)) and without (page_table_html's own find_top1_match),
          alternating.  Host clock, ms per call; the HTML part alone is given as well.
  stream  predict_stream() with layout + Lore + table_html on seeded pages (batches of 16), device_match off (the route before this knob
          existed) against on: the SAME pipeline object, the knob toggled between runs, alternating.  pages/s and metric["host_seconds"]["collect"].

    python tools/lore_match_bench.py [out.txt]
"""
from __future__ import annotations

import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from pdf_table_amd.engine import HipEngine  # noqa: E402
from pdf_table_amd.table_text_match import find_top1_match, page_table_html  # noqa: E402

B, CELLS, RUNS = 64, 300, 7


def stats(v):
    return f"{statistics.median(v):9.4f} ({min(v):.4f} .. {max(v):.4f})"


def kernel_and_host(out):
    from lore_match_ref import page_polygons
    from pdf_table_amd.table_html import table_cells_from_logits
    from pdf_table_amd.tsr_stage import process_logic_output
    from test_gpu_lore_match import grid_table, random_lines, upload
    eng = HipEngine(0)
    out.append(f"== kernel vs host: {B} tables of {CELLS} cells per call; median (min .. max) of {RUNS} ==")
    for n_lines in (30, 100):
        rng = np.random.default_rng(n_lines)
        tables = [grid_table(rng, CELLS, crop=(900, 640)) for _ in range(B)]
        for t in tables:
            t["lines"] = random_lines(rng, t, n_lines)
        args = upload(eng, tables)
        call = lambda: eng.op_lore_match(*args)
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
        prepared = []
        for t in tables:
            polys = page_polygons(t["dets"][:CELLS], t["meta"], t["upper_left"], t["offset"])
            cells, order = table_cells_from_logits(polys, process_logic_output(t["axes"][:CELLS]), return_order=True)
            prepared.append((np.array([[c.x1, c.y1, c.x2, c.y2] for c in cells], np.float64), np.asarray(order), t["lines"].astype(np.float64)))
        host_ms, same, o = [], True, 0
        for r in range(RUNS + 1):
            t0 = time.perf_counter()
            for cb, order, lb in prepared:
                top1 = find_top1_match(lb, cb)
                if r == 0:                                             # the first pass checks the kernel and is not timed
                    same = same and np.array_equal(order[top1], got[o:o + len(lb)])
                    o += len(lb)
            if r:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        assert same, "kernel and find_top1_match differ"
        out.append(f"{n_lines:3d} lines per table: kernel {stats(ms)} ms per call of {B} tables   host {stats([h / B for h in host_ms])} ms per table = "
                   f"{statistics.median(host_ms):8.2f} ms per {B} tables   ratio {statistics.median(host_ms) / statistics.median(ms):7.1f}x   results equal")
    eng.close()


def stage_bench(out):
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_pages import make_page
    pipe = OcrTablePipeline(device=0, synthetic_seed=0, table_structure=True, table_html=True)
    stage = pipe.table_structure_task._stage
    made = [make_page(i) for i in range(16)]
    pages = torch.from_numpy(np.stack([m[0] for m in made])).to(pipe.engine._tdev)
    rng = np.random.default_rng(1)
    regions = []
    for k in range(16):                                                # four regions per page: 64 tables
        regions.append(np.array([[40 + 10 * k, 60, 500, 420], [520, 80, 1000, 500], [60, 520, 640, 980], [300, 300 + 5 * k, 900, 800]]))
    tbx = []
    for r in regions:
        rows = []
        for (x1, y1, x2, y2) in r.tolist():
            cx, cy = rng.uniform(x1, x2, 30), rng.uniform(y1, y2, 30)
            w, h = rng.uniform(20, 120, 30), rng.uniform(8, 28, 30)
            rows.append(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1))
        tbx.append(np.trunc(np.concatenate(rows)))
    quads = [np.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 1], b[:, 2], b[:, 3], b[:, 0], b[:, 3]], 1) for b in tbx]
    texts = [["12.5"] * len(b) for b in tbx]
    tables, metas = stage.tables(tuple(pages.shape[1:3]), regions)
    offs = np.stack([tables["x0"], tables["y0"]], 1).astype(np.float32)

    def run(device):
        pending = stage.start(pages, tables)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        match = stage.match_input(tables, metas, regions, tbx) if device else None
        flat = stage.collect(stage.process(pending, match) if device else stage.process(pending), metas, offs)
        t1 = time.perf_counter()
        res = stage.regroup(flat, regions)
        for k, page in enumerate(res):
            for ti, t in enumerate(page):
                if len(t["scores"]) == 0:
                    continue
                kw = {"matched": t["matched"], "matched_lines": t["matched_lines"]} if device else {}
                t["html"] = page_table_html(t["polygons"], t["logi"], regions[k][ti], quads[k], texts[k], **kw)
        t2 = time.perf_counter()
        return res, (t2 - t0) * 1e3, (t2 - t1) * 1e3

    for d in (False, True, False, True):
        res, _, _ = run(d)
    a, b = run(False)[0], run(True)[0]
    assert all(x.get("html") == y.get("html") for pa, pb in zip(a, b) for x, y in zip(pa, pb)), "HTML differs between the routes"
    ncell = [len(t["scores"]) for page in a for t in page]
    nline = [len(t["matched"]) for page in b for t in page]
    ms = {False: [], True: []}
    html = {False: [], True: []}
    for _ in range(RUNS):
        for d in (False, True):
            _, total, h = run(d)
            ms[d].append(total)
            html[d].append(h)
    out.append(f"== stage: TsrStage (wtw, seeded, bf16) process + collect + HTML for one call of {len(tables)} tables, cells per table {min(ncell)} .. "
               f"{max(ncell)} (mean {np.mean(ncell):.0f}), candidate lines per table {min(nline)} .. {max(nline)}; host clock, ms per call, median (min .. max) of "
               f"{RUNS}, alternating; the HTML is the same on both routes ==")
    out.append(f"without match: total {stats(ms[False])}   of which HTML {stats(html[False])}")
    out.append(f"with match:    total {stats(ms[True])}   of which HTML {stats(html[True])}")
    pipe.engine.close()


def stream_bench(out):
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_pages import make_page
    pipe = OcrTablePipeline(device=0, synthetic_seed=0, layout=True, table_structure=True, table_html=True)
    pages = torch.from_numpy(np.stack([make_page(i % 8)[0] for i in range(16)])).to(pipe.engine._tdev)
    batches = [pages] * 8

    def run(knob):
        pipe.device_match = knob
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(len(r) for r in pipe.predict_stream(batches))
        dt = time.perf_counter() - t0
        return n / dt, pipe.metric["host_seconds"]["collect"] * 1e3

    for k in (False, True):
        run(k)
    pps = {False: [], True: []}
    col = {False: [], True: []}
    for _ in range(RUNS):
        for k in (False, True):
            p, c = run(k)
            pps[k].append(p)
            col[k].append(c)
    out.append(f"== stream: predict_stream(), layout + Lore wtw + table_html, seeded, bf16, 8 batches of 16 pages of 1024 x 1024 per run; median (min .. max) of {RUNS}, "
               f"the knob toggled on one pipeline object, alternating ==")
    for k in (False, True):
        out.append(f"device_match={str(k):5s}: {stats(pps[k])} pages/s   host_seconds['collect'] {stats(col[k])} ms per run")
    pipe.engine.close()


if __name__ == "__main__":
    lines = []
    kernel_and_host(lines)
    stage_bench(lines)
    stream_bench(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)
