"""The WTW cell metric, device route against host route, measured (profiles/r23/cell_metric.txt): one process, warm-up first, medians with ranges of 7
windows, the routes alternating inside each window.

  pairs   256 seeded (prediction, truth) pairs per size (pdf_table_amd/cell_metric_synth.py): truth tables of 100 / 400 / 1000 / 3000 cells, the
          prediction the truth with corners moved by up to 4 pixels, about 10 % of the cells dropped and 5 % of the rest with one axis off by one.
  kernel  pt_op_cell_metric alone, from device events around the launch, summed over the chunks of a device-route call.
  device  WtwMetric(engine=HipEngine(0)).batch_evaluate: conversion and checks, packing, one pinned upload, the launch, one copy back, the per-pair
          dicts.  Seconds per 256 pairs, host clock (the call ends in the wait for its copy).  "pack + copy" is that time without the kernel.
  host    WtwMetric().batch_evaluate on the same pairs: numpy over [256, n_pred] blocks, one thread.
  loops   tests/cell_metric_ref.py -- the reference's own bubble sort and scan, loop for loop -- on the first 4 pairs of the 100- and 400-cell sets, as
          the stand-in for the reference's cost; seconds per pair, and that times 256.

    python tools/cell_metric_bench.py [out.txt] [--pairs N] [--windows N] [--sizes 100,400,1000,3000]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from pdf_table_amd import cell_metric as M  # noqa: E402
from pdf_table_amd.cell_metric_synth import table_pair  # noqa: E402


def stats(v, scale=1.0):
    return f"{statistics.median(v) * scale:9.4f} ({min(v) * scale:.4f} .. {max(v) * scale:.4f})"


def same(a, b):
    return all(np.array_equal(x["match"], y["match"]) and all(x[f] == y[f] for f in ("precision", "recall", "fp", "fn", "acc", "tp", "truep")) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="100,400,1000,3000")
    ap.add_argument("--loop-pairs", type=int, default=4)
    a = ap.parse_args()
    import torch
    import cell_metric_ref as R
    from pdf_table_amd.engine import HipEngine
    if not torch.cuda.is_available():
        raise SystemExit("cell_metric_bench: no GPU; nothing is measured without one")
    host, dev = M.WtwMetric(), M.WtwMetric(engine=HipEngine(0))
    out = [f"== WTW cell metric: {a.pairs} seeded pairs per size; median (min .. max) of {a.windows} windows, device and host route alternating in one process =="]
    for n in [int(s) for s in a.sizes.split(",")]:
        pairs = [table_pair(2300 + 7 * k + n, n) for k in range(a.pairs)]
        dev.events = []
        got = dev.batch_evaluate(pairs)                                   # warm-up: the library, the allocator's blocks, pinned memory
        dev.batch_evaluate(pairs)
        want = host.batch_evaluate(pairs[:8])
        t_dev, t_host, t_kernel = [], [], []
        for w in range(a.windows):
            dev.events = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = dev.batch_evaluate(pairs)
            t_dev.append(time.perf_counter() - t0)
            t_kernel.append(sum(e[0].elapsed_time(e[1]) for e in dev.events) * 1e-3)
            t0 = time.perf_counter()
            want = host.batch_evaluate(pairs)
            t_host.append(time.perf_counter() - t0)
            print(f"{n} cells, window {w}: device {t_dev[-1]:.4f} s (kernel {t_kernel[-1] * 1e3:.2f} ms, {len(dev.events)} chunks)   host {t_host[-1]:.4f} s", flush=True)
        s = M.WtwMetric.summarize(got)
        overhead = [d - k for d, k in zip(t_dev, t_kernel)]
        out.append(f"-- {n} cells a truth table ({min(len(p[0][0]) for p in pairs)} .. {max(len(p[0][0]) for p in pairs)} predicted), {a.pairs} pairs, "
                   f"{len(dev.events)} chunk(s) --")
        out.append(f"  host route (numpy):        {stats(t_host)} s")
        out.append(f"  device route, end to end:  {stats(t_dev)} s")
        out.append(f"    pt_op_cell_metric alone: {stats(t_kernel, 1e3)} ms (device events)")
        out.append(f"    pack + copy + dicts:     {stats(overhead)} s = {100 * statistics.median(overhead) / statistics.median(t_dev):.1f} % of the end-to-end median")
        out.append(f"  device range {'below' if max(t_dev) < min(t_host) else 'NOT below'} host range; ratio of the medians host / device "
                   f"{statistics.median(t_host) / statistics.median(t_dev):.1f}x; results equal: {same(got, want)}; fallbacks {len(dev.last_fallback)}")
        out.append(f"  acc {s['acc']:.4f}  det_precision {s['det_precision']:.4f}  det_recall {s['det_recall']:.4f}  f1 {s['f1']:.4f}")
        if n <= 400 and a.loop_pairs > 0:
            t0 = time.perf_counter()
            ref = [R.pair(R.units_of(*p), R.units_of(*g)) for p, g in pairs[:a.loop_pairs]]
            per = (time.perf_counter() - t0) / a.loop_pairs
            ok = all(r["match"] == w["match"].tolist() and (r["tp"], r["truep"]) == (w["tp"], w["truep"]) for r, w in zip(ref, want))
            out.append(f"  the reference's loops (restated, {a.loop_pairs} pairs, once): {per:.4f} s a pair = {per * a.pairs:.1f} s per {a.pairs} pairs (extrapolated); "
                       f"results equal: {ok}")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
