"""DB detection score_mode="slow" (pt_op_det_poly_scores, DetStage), measured (profiles/r25/det_slow_score.txt): one process, warm-up first, medians
with ranges of 7 windows, the two modes alternating inside every window.  The pages are the bench's: 64 synthetic 1024 x 1024 pages (8 distinct),
the seeded DB-ResNet18 with the text channel, db_pp pre/post (a 960 x 960 map), the detector's own candidates.

  kernel  pt_op_det_poly_scores alone on those candidates' contours (device events around 20 back-to-back calls; ms per call), with the vertex and
          pixel totals, the largest candidate alone and a crafted comb over the whole map alone; pt_det_box_scores on the same candidates as
          context -- it is the other mode, not a baseline.
  stage   DetStage.boxes per 64 pages in both modes, split into its timing keys (copy / cand / score / final), ms.
  host    the only route a tree without the kernel has for this mode: box_score_slow over fill_poly_mask in numpy (tests/db_slow_ref.py), timed on 4
          pages and EXTRAPOLATED to 64 -- labelled so.

    python tools/det_slow_score_bench.py [out.txt]
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

from pdf_table_amd import engine as E  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.det_stage import DetConfig, DetStage  # noqa: E402
from pdf_table_amd.engine import HipEngine  # noqa: E402
from pdf_table_amd.synth_pages import make_page  # noqa: E402
from pdf_table_amd.synth_weights import db_resnet18_state_dict  # noqa: E402
from pdf_table_amd.weights import pack_db_resnet18  # noqa: E402

B, RUNS, REPS = 64, 7, 20


def stats(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main(path):
    out = []
    eng = HipEngine(0)
    eng.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=eng.weight_fmt))
    pages = torch.from_numpy(np.stack([make_page(i % 8, 1024)[0] for i in range(B)])).to(eng._tdev)
    cfg = dict(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5)
    fast, slow = DetStage(eng, DetConfig(**cfg), workers=16), DetStage(eng, DetConfig(score_mode="slow", **cfg), workers=16)
    prob, bitmap, ev = fast.forward(pages)
    torch.cuda.synchronize()
    n, H, W = prob.shape
    bm = bitmap.cpu().numpy()
    cand, counts, pts, offs = E.db_contour_candidates_batch(bm, 1000, 3.0, 16)
    tot = int(counts.sum())
    pg = np.repeat(np.arange(n, dtype=np.int32), counts)
    lens = np.diff(offs)
    x0 = np.minimum.reduceat(pts[:, 0], offs[:-1]); x1 = np.maximum.reduceat(pts[:, 0], offs[:-1])
    y0 = np.minimum.reduceat(pts[:, 1], offs[:-1]); y1 = np.maximum.reduceat(pts[:, 1], offs[:-1])
    area = (x1 - x0 + 1).astype(np.int64) * (y1 - y0 + 1)
    big = int(np.argmax(lens.astype(np.int64) * (y1 - y0 + 1)))       # most row x vertex work
    out.append(f"== candidates: {tot} on {n} pages of {H} x {W}; {int(lens.sum())} contour vertices (median {int(np.median(lens))}, max {int(lens.max())} per "
               f"candidate); bounding rectangles {area.sum() / 1e6:.2f} Mpx (median {int(np.median(area))}, max {int(area.max())} px) ==")
    out.append(f"   the largest candidate by rows x vertices: {int(lens[big])} vertices, rectangle {int(x1[big] - x0[big] + 1)} x {int(y1[big] - y0[big] + 1)} px")
    # ---- kernel alone ----------------------------------------------------------------------------------------------------------------------------
    d_pts, d_offs, d_pg = (torch.from_numpy(np.ascontiguousarray(v)).to(eng._tdev) for v in (pts, offs, pg))
    scores = torch.empty((tot,), dtype=torch.float32, device=eng._tdev)
    sums = torch.empty((tot,), dtype=torch.float64, device=eng._tdev)
    cnts = torch.empty((tot,), dtype=torch.int32, device=eng._tdev)
    work = torch.empty((tot * L.PT_DET_POLY_WORK_BYTES,), dtype=torch.uint8, device=eng._tdev)
    poly = lambda: eng.op_det_poly_scores(prob, d_pts, d_offs, d_pg, offs, pg, sums=sums, counts=cnts, scores=scores, work=work)
    o1 = np.array([0, lens[big]], np.int32)
    d_p1 = torch.from_numpy(np.ascontiguousarray(pts[offs[big]:offs[big + 1]])).to(eng._tdev)
    d_o1, d_g1 = torch.from_numpy(o1).to(eng._tdev), torch.from_numpy(pg[big:big + 1].copy()).to(eng._tdev)
    one = lambda: eng.op_det_poly_scores(prob, d_p1, d_o1, d_g1, o1, pg[big:big + 1], scores=scores, work=work)
    valid = np.arange(cand.shape[1])[None, :] < counts[:, None]
    ab = np.zeros((tot, 9), np.float32)
    ab[:, 0], ab[:, 1:] = pg, cand[valid]
    d_ab = torch.from_numpy(ab).to(eng._tdev)
    quad = lambda: eng.det_box_scores(prob, d_ab)
    # crafted: a two-sided comb over the whole map, a tooth every second column up and down from a bar across the middle -- thousands of vertices, a
    # page-sized rectangle, every band used
    teeth, mid = (W - 8) // 2, H // 2
    cv = []
    for k in range(teeth):                      # the upper side, left to right
        x = 4 + 2 * k
        cv += [(x, mid - 10), (x, 4), (x + 1, 4), (x + 1, mid - 10)]
    for k in range(teeth - 1, -1, -1):          # the lower side, right to left
        x = 4 + 2 * k
        cv += [(x + 1, mid + 10), (x + 1, H - 4), (x, H - 4), (x, mid + 10)]
    cv = np.asarray(cv, np.int32)
    o2 = np.array([0, len(cv)], np.int32)
    d_p2, d_o2 = torch.from_numpy(cv).to(eng._tdev), torch.from_numpy(o2).to(eng._tdev)
    comb = lambda: eng.op_det_poly_scores(prob, d_p2, d_o2, d_g1, o2, pg[big:big + 1], scores=scores, work=work)
    for f in (poly, one, comb, quad):
        f()
    torch.cuda.synchronize()
    px = int(cnts.sum().item())
    t = {"poly": [], "one": [], "quad": [], "comb": []}
    for _ in range(RUNS):
        for k, f in (("poly", poly), ("quad", quad), ("one", one), ("comb", comb)):
            t[k].append(_events(f, REPS))
    out.append(f"== kernel: ms per call, median (min .. max) of {RUNS} windows of {REPS} calls ==")
    out.append(f"   pt_op_det_poly_scores, all {tot} candidates ({px / 1e6:.2f} Mpx under the masks): {stats(t['poly'])}")
    out.append(f"   pt_op_det_poly_scores, the largest candidate alone:                      {stats(t['one'])}")
    out.append(f"   pt_op_det_poly_scores, a crafted comb of {len(cv)} vertices over {W - 8} x {H - 8} px, alone: {stats(t['comb'])}")
    out.append(f"   pt_det_box_scores on the same candidates' rectangles (the other mode):    {stats(t['quad'])}")
    # ---- DetStage.boxes ----------------------------------------------------------------------------------------------------------------------------
    src = tuple(pages.shape[1:3])
    for s in (fast, slow):
        s.boxes(prob, bitmap, src, ev)
    keys = ("copy", "cand", "score", "final")
    tm = {m: {k: [] for k in keys + ("total",)} for m in ("fast", "slow")}
    nbox = {}
    for _ in range(RUNS):
        for m, s in (("fast", fast), ("slow", slow)):
            s.timing = {k: 0.0 for k in keys}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = s.boxes(prob, bitmap, src, ev)
            tm[m]["total"].append((time.perf_counter() - t0) * 1e3)
            for k in keys:
                tm[m][k].append(s.timing[k] * 1e3)
            nbox[m] = sum(len(r) for r in res)
    out.append(f"== DetStage.boxes per {n} pages, ms, median (min .. max) of {RUNS} alternating calls; boxes kept: fast {nbox['fast']}, slow {nbox['slow']} ==")
    for m in ("fast", "slow"):
        out.append(f"   {m}: total {stats(tm[m]['total'])}")
        for k in keys:
            out.append(f"         {k:5s} {stats(tm[m][k])}")
    # ---- the host-only route ---------------------------------------------------------------------------------------------------------------------
    import db_slow_ref as R
    hp = prob[:4].cpu().numpy()
    k4 = int(counts[:4].sum())
    worst = 0.0
    poly()
    torch.cuda.synchronize()
    dev_scores = scores.cpu().numpy()
    t0 = time.perf_counter()
    for j in range(k4):
        s, c = R.box_score_slow(hp[pg[j]], pts[offs[j]:offs[j + 1]])
        worst = max(worst, abs(float(dev_scores[j]) - (s / c if c else 0.0)))
    host4 = time.perf_counter() - t0
    out.append(f"== host-only route (numpy box_score_slow over fill_poly_mask, tests/db_slow_ref.py): {host4 * 1e3:.0f} ms for the {k4} candidates of 4 pages; "
               f"EXTRAPOLATED to {n} pages: {host4 * n / 4 * 1e3:.0f} ms (not measured at 64) ==")
    out.append(f"   the device scores of those {k4} candidates differ from it by at most {worst:.2e}")
    lines = ["how: python tools/det_slow_score_bench.py profiles/r25/det_slow_score.txt -- one process on one MI355X"] + out
    print("\n".join(lines))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
