"""Seeded head maps for the edge cases of the two heat-map decodes (tests/test_decode_edges_host.py, tests/test_gpu_decode_edges.py):
equal scores, the top-K caps really exceeded, more peaks than the candidate buffer holds, peaks on the rim and across the row wrap,
table seams inside a workgroup, corner pixels outside the map, more hits than one 64-lane round.  numpy only.

Every generator returns (heads, facts).  heads is in the layout of lore_synth.synth_lore_heads (NCHW f32: hm 2, st 8, wh 8, ax 256, cr 256,
reg 2) or of centernet_synth.make_case (hm 2, v2c 8, c2v 8, reg 2; the CenterNet ones return ((heads, (crop w, crop h)), facts)); batch
cases return a list of such tables.  facts names what the case relies on -- raw peak counts per class, the pixels that must come first,
hit counts -- and the host test asserts every one of them against the CPU references, so that a case cannot silently stop exercising its edge.
Pixel indices are flat (y * W + x)."""
from __future__ import annotations

import numpy as np

LOW = -8.0            # background logit: sigmoid 3e-4, below every threshold


def _lore_blank(rng, H, W, wh_scale=3.0, st_scale=1.0):
    hm = np.full((1, 2, H, W), LOW, np.float32) - rng.uniform(0.0, 0.5, (1, 2, H, W)).astype(np.float32)
    wh = (np.array([1, 1, -1, 1, -1, -1, 1, -1], np.float32).reshape(1, 8, 1, 1) * wh_scale
          + rng.normal(0, 0.3, (1, 8, H, W)).astype(np.float32))
    st = (np.array([1, 1, -1, 1, -1, -1, 1, -1], np.float32).reshape(1, 8, 1, 1) * st_scale
          + rng.normal(0, 0.2, (1, 8, H, W)).astype(np.float32))
    reg = rng.uniform(0.2, 0.8, (1, 2, H, W)).astype(np.float32)
    ax = rng.standard_normal((1, 256, H, W)).astype(np.float32)
    cr = rng.standard_normal((1, 256, H, W)).astype(np.float32)
    return {"hm": hm, "st": st, "wh": wh, "ax": ax, "cr": cr, "reg": reg}


def _cn_blank(rng, H, W):
    hm = np.full((1, 2, H, W), LOW, np.float32) - rng.uniform(0.0, 0.5, (1, 2, H, W)).astype(np.float32)
    reg = rng.uniform(0.0, 1.0, (1, 2, H, W)).astype(np.float32)
    v2c = rng.normal(0.0, 3.0, (1, 8, H, W)).astype(np.float32)
    c2v = rng.normal(0.0, 3.0, (1, 8, H, W)).astype(np.float32)
    return {"hm": hm, "v2c": v2c, "c2v": c2v, "reg": reg}


def _separated_logits(rng, shape, lo, hi):
    """random logits whose SCORES are a shuffled, jittered ladder over [lo, hi]: continuous random values, but any two at least half a
    rung apart (>= 3e-5 for 5184 values), far above the few 1e-8 by which the device's expf sigmoid and the reference's may differ -- so
    the order of the scores is the same on both sides"""
    n = int(np.prod(shape))
    step = (hi - lo) / n
    s = lo + (np.arange(n) + rng.uniform(0.25, 0.75, n)) * step
    s = s[rng.permutation(n)]
    return np.log(s / (1.0 - s)).astype(np.float32).reshape(shape)


def _flat(ys, xs, W):
    return (np.asarray(ys) * W + np.asarray(xs)).astype(np.int64).reshape(-1)


# ---- a. ties ---------------------------------------------------------------------------------------------------------------------
def _ties_into(rng, hm, W):
    """per class: an 8 x 8 plateau at logit 1.5, a 6 x 6 plateau at logit 20 (score exactly 1.0), isolated peaks in between.
    -> per class the pixels in the documented order (score desc, index asc)"""
    order = []
    for cls, (ay, ax_, by, bx) in enumerate(((4, 5, 30, 20), (20, 30, 5, 3))):
        hm[0, cls, ay:ay + 8, ax_:ax_ + 8] = 1.5
        hm[0, cls, by:by + 6, bx:bx + 6] = 20.0 + cls
        iso_y = np.array([16, 16, 40, 44, 44, 40]) + cls
        iso_x = np.array([3, 40, 40, 3, 12, 30]) + cls
        v = np.sort(rng.uniform(2.0, 6.0, len(iso_y)).astype(np.float32))[::-1]
        hm[0, cls, iso_y, iso_x] = v
        yy, xx = np.meshgrid(np.arange(by, by + 6), np.arange(bx, bx + 6), indexing="ij")
        hi = np.sort(_flat(yy, xx, W))
        yy, xx = np.meshgrid(np.arange(ay, ay + 8), np.arange(ax_, ax_ + 8), indexing="ij")
        lo = np.sort(_flat(yy, xx, W))
        order.append(np.concatenate([hi, _flat(iso_y, iso_x, W), lo]))
    return order


def lore_ties(seed=0, H=80, W=80):
    rng = np.random.default_rng(5000 + seed)
    h = _lore_blank(rng, H, W)
    order = _ties_into(rng, h["hm"], W)
    return h, {"order": order, "peaks": [len(o) for o in order]}


def cn_ties(seed=0, H=48, W=48):
    rng = np.random.default_rng(5100 + seed)
    h = _cn_blank(rng, H, W)
    order = _ties_into(rng, h["hm"], W)
    return (h, (W * 4, H * 4)), {"order": order, "peaks": [len(o) for o in order]}


# ---- b. the K caps exceeded ------------------------------------------------------------------------------------------------------
def lore_cap_cells(seed=0, H=128, W=96):
    """3072 cell peaks (stride-2 lattice, continuous separated scores above every threshold and above 0.5, so that the x0.4 demotion of wiz_rev
    keeps them visible) against K = 3000; no corner at all"""
    rng = np.random.default_rng(5200 + seed)
    h = _lore_blank(rng, H, W, wh_scale=1.0)
    h["hm"][0, 0, 0::2, 0::2] = _separated_logits(rng, (H // 2, W // 2), 0.55, 0.99)
    return h, {"peaks": [(H // 2) * (W // 2), 0], "kept": [3000, 0]}


def lore_cap_corners(seed=0, H=144, W=144, ncell=12):
    """5184 corner peaks (all >= 0.3) against K = 5000; a dozen 30-px cells, each over ~225 lattice points, so corners below the cap
    lie inside cells"""
    rng = np.random.default_rng(5300 + seed)
    h = _lore_blank(rng, H, W, wh_scale=15.0, st_scale=0.5)
    h["hm"][0, 1, 0::2, 0::2] = _separated_logits(rng, (H // 2, W // 2), 0.35, 0.98)
    ys = rng.permutation(np.arange(18, H - 18, 9))[:ncell]
    xs = rng.permutation(np.arange(18, W - 18, 9))[:ncell]
    h["hm"][0, 0, ys, xs] = rng.uniform(1.0, 4.0, ncell).astype(np.float32)
    return h, {"peaks": [ncell, (H // 2) * (W // 2)], "kept": [ncell, 5000], "cells": _flat(ys, xs, W)}


def cn_cap_verts(seed=0, H=128, W=128, ncell=30):
    """4096 vertex peaks against K = 4000, about 30 cells of 8 x 6 px, short random pointers (many vertices claim corners)"""
    rng = np.random.default_rng(5400 + seed)
    h = _cn_blank(rng, H, W)
    h["hm"][0, 1, 0::2, 0::2] = _separated_logits(rng, (H // 2, W // 2), 0.35, 0.98)
    ys = rng.permutation(np.arange(10, H - 10, 3))[:ncell]
    xs = rng.permutation(np.arange(10, W - 10, 3))[:ncell]
    h["hm"][0, 0, ys, xs] = rng.uniform(0.0, 4.0, ncell).astype(np.float32)
    h["c2v"][0, :, ys, xs] = (np.array([4, 3, 4, -3, -4, -3, -4, 3], np.float32)[None] + rng.normal(0, 0.4, (ncell, 8))).astype(np.float32)
    return (h, (W * 3, H * 3)), {"peaks": [ncell, (H // 2) * (W // 2)], "kept": [ncell, 4000]}


# ---- c. more peaks than the candidate buffer (PT_HEAT_CAP = 16384) ---------------------------------------------------------------
OVER_H, OVER_W = 136, 128
OVER_TOP = [(130, 10), (131, 40), (132, 70), (133, 100), (134, 120)]      # (y, x) of the five peaks above the flat class, logits 6..10


def _overflow_into(hm, cls):
    hm[0, cls] = 2.0
    for k, (y, x) in enumerate(OVER_TOP):
        hm[0, cls, y, x] = 6.0 + k
    first = _flat(*zip(*OVER_TOP[::-1]), OVER_W)          # logit 10 first
    return first, OVER_H * OVER_W - 8 * len(OVER_TOP)


def cn_overflow(seed=0):
    rng = np.random.default_rng(5500 + seed)
    h = _cn_blank(rng, OVER_H, OVER_W)
    first, n = _overflow_into(h["hm"], 0)
    vy, vx = rng.permutation(np.arange(3, 60, 3))[:12], rng.permutation(np.arange(3, 120, 3))[:12]
    h["hm"][0, 1, vy, vx] = rng.uniform(0.0, 4.0, 12).astype(np.float32)
    return (h, (OVER_W * 2, OVER_H * 2)), {"peaks": [n, 12], "first": first, "cls": 0}


def lore_overflow(seed=0, corner_class=False):
    """the flat class is the cell class (wiz_rev False) or, with corner_class, the corner class under 10 cells (wiz_rev True)"""
    rng = np.random.default_rng(5600 + seed + int(corner_class))
    h = _lore_blank(rng, OVER_H, OVER_W, wh_scale=12.0 if corner_class else 3.0, st_scale=0.5)
    first, n = _overflow_into(h["hm"], int(corner_class))
    other = 0
    if corner_class:
        # the 5000 kept corners are the five peaks and pixels 0 .. 4994 (rows 0 .. 38): the cells sit among them
        ys, xs = np.array([6, 8, 14, 20, 22, 26, 30, 33, 12, 50]), np.array([10, 40, 70, 100, 20, 55, 85, 110, 118, 60])
        h["hm"][0, 0, ys, xs] = rng.uniform(1.0, 4.0, len(ys)).astype(np.float32)
        other = len(ys)
    return h, {"peaks": [other, n] if corner_class else [n, 0], "first": first, "cls": int(corner_class)}


# ---- d. rim and row wrap ---------------------------------------------------------------------------------------------------------
def _rim_into(rng, hm, H, W):
    """both classes: peaks at the four map corners and on each edge; (6, W-1) a peak below its memory neighbour (7, 0), (12, W-1) a peak
    above its memory neighbour (13, 0): all four stay peaks.  Continuous distinct values.  -> flat indices of the twelve peaks"""
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2 + 3, 0), (H // 2 + 3, W - 1),
           (6, W - 1), (7, 0), (12, W - 1), (13, 0)]
    for cls in range(2):
        v = rng.uniform(0.5, 4.0, len(pts)).astype(np.float32)
        v[8], v[9] = 1.0 + 0.1 * cls, 3.0 + 0.1 * cls
        v[10], v[11] = 3.5 + 0.1 * cls, 1.2 + 0.1 * cls
        for (y, x), val in zip(pts, v):
            hm[0, cls, y, x] = val
    return _flat(*zip(*pts), W)


def lore_rim(seed=0, H=72, W=71):
    """odd W; 72 x 71 = 5112 pixels, the smallest such map the reference's top-5000 accepts"""
    rng = np.random.default_rng(5700 + seed)
    h = _lore_blank(rng, H, W, wh_scale=4.0, st_scale=2.0)
    pts = _rim_into(rng, h["hm"], H, W)
    return h, {"peaks": [12, 12], "pixels": pts}


def cn_rim(seed=0, H=40, W=33):
    rng = np.random.default_rng(5800 + seed)
    h = _cn_blank(rng, H, W)
    pts = _rim_into(rng, h["hm"], H, W)
    return (h, (W * 4, H * 4)), {"peaks": [12, 12], "pixels": pts}


# ---- e. batch seams --------------------------------------------------------------------------------------------------------------
def _seam_tables(rng, blank, H, W, mid_logit):
    """three tables; the middle one empty; table 0 has peaks within its last 64 pixels, table 2 within its first 64"""
    npix = H * W
    tables, facts = [], []
    for t in range(3):
        h = blank(rng, H, W)
        if t == 1:
            h["hm"][:] = mid_logit
            tables.append(h)
            facts.append({"peaks": [0, 0], "seam": np.zeros(0, np.int64)})
            continue
        pix = {}
        for cls in range(2):
            ni = min(8, len(range(3, H - 3, 3)), len(range(3, W - 3, 3)))
            inner = rng.permutation(np.arange(3, H - 3, 3))[:ni] * W + rng.permutation(np.arange(3, W - 3, 3))[:ni]
            seam = (npix - 64 + np.array([5, 25, 41, 63])) if t == 0 else np.array([0, 17, 36, 61])
            seam = seam + 2 * cls * (1 if t == 2 else -1)
            pix[cls] = np.concatenate([inner, seam])
            h["hm"][0, cls].reshape(-1)[pix[cls]] = rng.uniform(0.0, 4.0, len(pix[cls])).astype(np.float32)
        tables.append(h)
        facts.append({"peaks": [len(pix[0]), len(pix[1])], "seam": np.concatenate([pix[0][-4:], pix[1][-4:]])})
    return tables, facts


def lore_seams(seed=0, H=72, W=72):
    rng = np.random.default_rng(5900 + seed)
    tables, facts = _seam_tables(rng, lambda r, h, w: _lore_blank(r, h, w, wh_scale=5.0, st_scale=2.0), H, W, -20.0)
    return tables, {"tables": facts, "npix": H * W}


def cn_seams(seed=0, H=24, W=40):
    rng = np.random.default_rng(6000 + seed)
    tables, facts = _seam_tables(rng, _cn_blank, H, W, -20.0)
    return [(h, (W * 4, H * 4)) for h in tables], {"tables": facts, "npix": H * W}


# ---- f. corner pixels outside the map (Lore) -------------------------------------------------------------------------------------
def lore_outside(seed=0, H=72, W=72):
    """cells whose corner pixels x + W * round(y) fall before pixel 0 (`neg`), at or past H * W (`past`), or inside the map with x outside
    [0, W) -- the reference's wrap into the neighbouring row (`wrap`); a few corners so that wiz_rev has something to snap"""
    rng = np.random.default_rng(6100 + seed)
    h = _lore_blank(rng, H, W, wh_scale=4.0, st_scale=1.0)
    cells = {"neg": [(1, 5), (2, 40), (0, 66)], "past": [(H - 2, 6), (H - 1, 44), (H - 3, 69)],
             "wrap": [(20, 1), (30, 2), (40, W - 2), (50, W - 1)], "plain": [(25, 30), (45, 35)]}
    for kind, pts in cells.items():
        for (y, x) in pts:
            h["hm"][0, 0, y, x] = rng.uniform(1.0, 4.0)
            if kind == "neg":
                h["wh"][0, 1::2, y, x] = np.float32(8.0) + rng.uniform(0, 4, 4).astype(np.float32)      # corner y = centre - wh < -4
            elif kind == "past":
                h["wh"][0, 1::2, y, x] = np.float32(-8.0) - rng.uniform(0, 4, 4).astype(np.float32)
            elif kind == "wrap":
                sgn = 1.0 if x < W // 2 else -1.0
                h["wh"][0, 0::2, y, x] = np.float32(sgn * 9.0) + rng.uniform(-2, 2, 4).astype(np.float32)
    for (y, x) in [(23, 28), (27, 33), (24, 33), (43, 33), (47, 37)]:
        h["hm"][0, 1, y, x] = rng.uniform(1.0, 4.0)
    ncell = sum(len(p) for p in cells.values())
    return h, {"peaks": [ncell, 5], "min_neg": 3, "min_past": 3, "min_wrap": 4}


# ---- g. more than one 64-lane round ----------------------------------------------------------------------------------------------
def lore_rounds(seed=0, H=96, W=112):
    """five 30-px cells, each over a 15 x 15 stride-2 lattice of corner peaks with small `st` (every corner quad lies strictly inside the
    cell: >= 150 hits per cell, three 64-corner rounds and more); a small cell with exactly two corners inside it (score x0.4) and one
    with three (kept)"""
    rng = np.random.default_rng(6200 + seed)
    h = _lore_blank(rng, H, W, wh_scale=15.0, st_scale=0.4)
    big = [(18, 18), (18, 52), (18, 86), (52, 18), (52, 52)]
    ladder = _separated_logits(rng, (5, 15, 15), 0.35, 0.98)
    for k, (cy, cx) in enumerate(big):
        h["hm"][0, 0, cy, cx] = rng.uniform(2.0, 4.0)
        h["hm"][0, 1, cy - 14:cy + 15:2, cx - 14:cx + 15:2] = ladder[k]
    two, three = (60, 86), (82, 86)
    sign = np.array([1, 1, -1, 1, -1, -1, 1, -1], np.float32)
    for (cy, cx), pts in ((two, [(58, 84), (62, 88)]), (three, [(80, 83), (80, 89), (85, 86)])):
        h["hm"][0, 0, cy, cx] = rng.uniform(2.0, 4.0)
        h["wh"][0, :, cy, cx] = sign * 6.0
        for (y, x) in pts:
            h["hm"][0, 1, y, x] = rng.uniform(1.0, 4.0)
    return h, {"peaks": [7, 5 * 225 + 5], "big": _flat(*zip(*big), W), "two": two[0] * W + two[1], "three": three[0] * W + three[1]}


CN_ROUNDS_SIZE = 96


def cn_rounds(seed=0, exact_two=True):
    """One cell Q (corners (30,30) (30,50) (54,50) (54,30) in x,y; crop = map size, so the affine is the identity) whose corners are
    claimed by vertices of ranks 8 (or 10), 70, 130, 200 -- four different 64-vertex rounds.  Top-left is contested: rank 5 points into Q
    from 1.06 px (closer than 2 px: skipped), rank 8 from exactly 2.0 px (not skipped: `< 2`; only with exact_two), rank 10 and rank 100
    from afar; the earliest valid rank wins.  A degenerate cell (c2v = 0: lim = 0) next to a vertex that points at it claims nothing.
    Every other vertex keeps all four pointers within 2 px.  Vertex logits fall linearly with the rank."""
    rng = np.random.default_rng(6300 + seed)
    S = CN_ROUNDS_SIZE
    h = _cn_blank(rng, S, S)
    q = [(30.0, 30.0), (30.0, 50.0), (54.0, 50.0), (54.0, 30.0)]
    cy, cx = 40, 42
    h["hm"][0, 0, cy, cx] = 3.0
    h["reg"][0, :, cy, cx] = 0.25
    for m, (qx, qy) in enumerate(q):
        h["c2v"][0, 2 * m, cy, cx] = cx + 0.25 - qx
        h["c2v"][0, 2 * m + 1, cy, cx] = cy + 0.25 - qy
    dy, dx = 70, 70
    h["hm"][0, 0, dy, dx] = 2.5
    h["reg"][0, :, dy, dx] = 0.25
    h["c2v"][0, :, dy, dx] = 0.0
    centre = (cx + 0.25, cy + 0.25)
    # rank -> (pixel y, pixel x, pointer 0 target (x, y))
    special = {5: (31, 31, (32.0, 32.0)), 10: (29, 29, centre), 20: (72, 71, (dx + 0.25, dy + 0.25)), 70: (50, 29, centre),
               100: (32, 27, centre), 130: (50, 54, centre), 200: (29, 54, centre)}
    if exact_two:
        special[8] = (30, 33, (33.25, 32.25))
    n = 230
    fill = [(y, x) for y in range(2, 27, 3) for x in range(2, 93, 3)]
    fill = [fill[i] for i in rng.permutation(len(fill))[:n - len(special)]]
    logits = np.linspace(5.0, 0.5, n).astype(np.float32)
    order = []
    for r in range(n):
        if r in special:
            y, x, (tx, ty) = special[r]
            h["reg"][0, :, y, x] = 0.25
            h["v2c"][0, :, y, x] = 0.5
            h["v2c"][0, 0, y, x] = x + 0.25 - tx
            h["v2c"][0, 1, y, x] = y + 0.25 - ty
        else:
            y, x = fill.pop()
            h["v2c"][0, :, y, x] = rng.uniform(-1.0, 1.0, 8).astype(np.float32)
        h["hm"][0, 1, y, x] = logits[r]
        order.append(y * S + x)
    win = [special[8 if exact_two else 10], special[70], special[130], special[200]]
    corners = np.array([c for (y, x, _) in win for c in (x + 0.25, y + 0.25)], np.float32)
    return (h, (S, S)), {"peaks": [2, n], "vertex_order": np.array(order), "q_pixel": cy * S + cx, "q_corners": corners,
                         "degenerate_pixel": dy * S + dx, "ranks": sorted(special)}
