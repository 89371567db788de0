"""The TEDS table metric, device route against host route, measured (profiles/r22/teds.txt): one process, warm-up first, medians with ranges of 7
windows, the two routes alternating inside each window.

  pairs   256 seeded PubTabNet-like (prediction, truth) pairs (pdf_table_amd/teds_synth.py): tables of 20 x 8 to 40 x 15 cells, 3 .. 20 tokens a cell,
          some spans; the prediction is the truth with some cells' text perturbed, now and then a row dropped and a span changed.
  host    TEDS(n_jobs=16).batch_evaluate_html: the reference's own setting (ocr_table_task.py:281-285), a pool of 16 processes that is started before
          the first window.  Seconds per 256 pairs, host clock.
  device  TEDS(engine=HipEngine(0)).batch_evaluate_html on the same pairs: parse + flatten + pack in this process, one upload, pt_op_teds_cost,
          pt_op_teds_dist, one copy back per chunk.  Seconds per 256 pairs, host clock (the call ends in the wait for its copy), and of that the two
          kernels alone from device events, summed over the chunks.

    python tools/teds_bench.py [out.txt] [--pairs N] [--windows N] [--jobs N]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from pdf_table_amd import table_metric as M  # noqa: E402
from pdf_table_amd.teds_synth import table_pairs  # noqa: E402


def stats(v):
    return f"{statistics.median(v):9.4f} ({min(v):.4f} .. {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--jobs", type=int, default=16)
    a = ap.parse_args()
    import torch
    from pdf_table_amd.engine import HipEngine
    preds, trues = table_pairs(a.pairs, seed=22)
    flat = [M._prepare(p, t, False, None, False) for p, t in zip(preds, trues)]
    nodes = [max(f.t1.n, f.t2.n) for f in flat]
    conts = [f.n_cols for f in flat]
    out = [f"== TEDS: {a.pairs} seeded pairs, nodes per tree {min(nodes)} .. {max(nodes)} (median {statistics.median(nodes):.0f}), distinct cell contents per "
           f"pair {min(conts)} .. {max(conts)}; median (min .. max) of {a.windows} windows, device and host route alternating =="]
    host = M.TEDS(n_jobs=a.jobs)
    host.batch_evaluate_html(preds[:2 * a.jobs], trues[:2 * a.jobs])            # starts the pool (before this process opens the GPU), imports numpy in every worker
    dev = M.TEDS(engine=HipEngine(0))
    dev.events = []
    got = dev.batch_evaluate_html(preds, trues)                                # warm-up: the library, the allocator's blocks
    dev.batch_evaluate_html(preds, trues)
    print("warm", flush=True)
    t_dev, t_host, t_cost, t_dist, want = [], [], [], [], None
    for w in range(a.windows):
        dev.events = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.batch_evaluate_html(preds, trues)
        t_dev.append(time.perf_counter() - t0)
        t_cost.append(sum(e[0].elapsed_time(e[1]) for e in dev.events))
        t_dist.append(sum(e[1].elapsed_time(e[2]) for e in dev.events))
        t0 = time.perf_counter()
        want = host.batch_evaluate_html(preds, trues)
        t_host.append(time.perf_counter() - t0)
        print(f"window {w}: device {t_dev[-1]:.3f} s (cost {t_cost[-1]:.1f} ms, dist {t_dist[-1]:.1f} ms, {len(dev.events)} chunks)   host {t_host[-1]:.3f} s", flush=True)
    t0 = time.perf_counter()
    for p, t in zip(preds, trues):
        M._prepare(p, t, False, None, False)
    t_prep = time.perf_counter() - t0
    host.close()
    worst = max(abs(g - h) for g, h in zip(got, want))
    bound = max((f.t1.n + f.t2.n) ** 2 * 2.0 ** -52 / f.n_nodes + 2.0 ** -52 for f in flat)
    out.append(f"host route, n_jobs={a.jobs}:   {stats(t_host)} s per {a.pairs} pairs")
    out.append(f"device route:             {stats(t_dev)} s per {a.pairs} pairs   of that parse + flatten (once, alone) {t_prep:.3f} s")
    out.append(f"  pt_op_teds_cost alone:  {stats(t_cost)} ms per {a.pairs} pairs (device events, {len(dev.events)} chunks)")
    out.append(f"  pt_op_teds_dist alone:  {stats(t_dist)} ms per {a.pairs} pairs")
    out.append(f"ratio of the medians host / device {statistics.median(t_host) / statistics.median(t_dev):.1f}x; device faster in "
               f"{sum(d < h for d, h in zip(t_dev, t_host))} of {a.windows} windows")
    out.append(f"scores {min(want):.4f} .. {max(want):.4f} (mean {statistics.mean(want):.4f}); largest |device - host| {worst:.3e} (bound {bound:.3e}); fallbacks "
               f"{len(dev.last_fallback)}")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
