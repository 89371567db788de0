"""What score_mode="slow" is held to, stated in Python.  Test infrastructure only: nothing in pdf_table_amd/ imports it.

1. ``box_score_slow``: DBPostProcess.box_score_slow (db_pp/processor_ocr_db_pp.py:270-289) restated over oracle.db_post.fill_poly_mask, returning
   (sum, count) so that a test can hold the mask itself to account; ``score`` is sum / count (0 for an empty mask), what cv2.mean returns.
2. ``row_rule_mask``: the per-row formulation pt_op_det_poly_scores (csrc/det_poly_score.hip) evaluates, in the kernel's own integer arithmetic:
   * an edge's Bresenham pixels on one row are ONE x-interval (``outline_interval``): a run for an x-major edge, one pixel for a y-major one;
   * the sorted, paired scan-line spans equal a histogram rule: with c[x] the number of active crossings whose rounded position is x and B(x) the
     number whose rounded position is < x (those left of the mask included), a pixel is interior iff c[x] > 0 or B(x) is odd.
   tests/test_db_slow_host.py searches seeded polygons for a difference between this and fill_poly_mask.
"""
from __future__ import annotations

import numpy as np

from oracle import db_post as O


def clipped_rect(contour, h, w):
    """(xmin, xmax, ymin, ymax) of box_score_slow: the extent of the points, clipped to the map"""
    c = np.asarray(contour, dtype=np.int64).reshape(-1, 2)
    xmin = int(np.clip(c[:, 0].min(), 0, w - 1))
    xmax = int(np.clip(c[:, 0].max(), 0, w - 1))
    ymin = int(np.clip(c[:, 1].min(), 0, h - 1))
    ymax = int(np.clip(c[:, 1].max(), 0, h - 1))
    return xmin, xmax, ymin, ymax


def slow_mask(contour, h, w):
    """-> (mask uint8 [ymax - ymin + 1, xmax - xmin + 1], (xmin, xmax, ymin, ymax))"""
    c = np.asarray(contour, dtype=np.int64).reshape(-1, 2)
    xmin, xmax, ymin, ymax = clipped_rect(c, h, w)
    shifted = c - np.array([xmin, ymin])
    return O.fill_poly_mask(ymax - ymin + 1, xmax - xmin + 1, shifted), (xmin, xmax, ymin, ymax)


def box_score_slow(prob, contour, mask_fn=None):
    """prob float32 [H, W], contour int [k, 2] (x, y) -> (sum float64, count int); the terms are added in numpy's order"""
    h, w = prob.shape
    mask, (xmin, xmax, ymin, ymax) = (mask_fn or slow_mask)(contour, h, w)
    region = prob[ymin:ymax + 1, xmin:xmax + 1]
    cnt = int(mask.sum())
    return float(region[mask != 0].astype(np.float64).sum()), cnt


def score(s, cnt):
    """the float32 the device returns for (sum, count)"""
    return np.float32(s / cnt) if cnt else np.float32(0)


# ---- the kernel's row formulation ------------------------------------------------------------------------------------------------------------
def _cdiv_trunc(a, b):
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def outline_interval(ax, ay, bx, by, y):
    """the x-interval [lo, hi] that the 8-connected Bresenham line a -> b (iterated left to right, exact halves toward the start) covers on row y,
    or None"""
    if bx < ax:
        ax, ay, bx, by = bx, by, ax, ay
    dx = bx - ax
    dy = abs(by - ay)
    sy = 1 if by >= ay else -1
    u = (y - ay) * sy
    if u < 0 or u > dy:
        return None
    if dy > dx:                                 # y-major: step u sits at minor position floor((2 dx u + dy - 1) / (2 dy))
        x = ax + (2 * dx * u + dy - 1) // (2 * dy)
        return x, x
    if dx == 0:                                 # a single point
        return ax, ax
    if dy == 0:
        return ax, bx
    # x-major: step j sits on minor position floor((2 dy j + dx - 1) / (2 dx)); those equal to u are j in [lo, hi]
    num = 2 * dx * u - dx + 1
    lo = 0 if num <= 0 else (num + 2 * dy - 1) // (2 * dy)
    hi = min(dx, (2 * dx * (u + 1) - dx) // (2 * dy))
    if lo > hi:
        return None
    return ax + lo, ax + hi


def row_rule_mask(contour, h, w):
    """same signature and result as slow_mask, by the per-row rule, in absolute map coordinates like the kernel"""
    c = [(int(x), int(y)) for x, y in np.asarray(contour, dtype=np.int64).reshape(-1, 2)]
    xmin, xmax, ymin, ymax = clipped_rect(c, h, w)
    vymin, vymax = min(p[1] for p in c), max(p[1] for p in c)
    mw = xmax - xmin + 1
    mask = np.zeros((ymax - ymin + 1, mw), dtype=np.uint8)
    k = len(c)
    for y in range(ymin, ymax + 1):
        cross = [0] * mw                        # c[x]
        diff = [0] * (mw + 1)                   # +1 / -1 interval ends
        left = 0                                # crossings whose rounded position is left of the rectangle
        scan = vymin <= y < vymax
        for i in range(k):
            (ax, ay), (bx, by) = c[i - 1], c[i]
            iv = outline_interval(ax, ay, bx, by, y)
            if iv is not None:
                lo, hi = max(iv[0], xmin), min(iv[1], xmax)
                if lo <= hi:
                    diff[lo - xmin] += 1
                    diff[hi - xmin + 1] -= 1
            if not scan or ay == by:
                continue
            dxf = _cdiv_trunc((bx << 16) - (ax << 16), by - ay)
            y0, y1, x0 = (ay, by, ax << 16) if ay < by else (by, ay, bx << 16)
            if y0 <= y < y1:
                r = (x0 + (y - y0) * dxf + 32768) >> 16
                if r < xmin:
                    left += 1
                elif r <= xmax:
                    cross[r - xmin] += 1
        cov, before = 0, left
        for x in range(mw):
            cov += diff[x]
            if cov > 0 or cross[x] > 0 or (before & 1):
                mask[y - ymin, x] = 1
            before += cross[x]
    return mask, (xmin, xmax, ymin, ymax)


def crossings_per_row(contour, h, w):
    """how many edges are active on each row of the scan-line part (every closed polygon gives an even number)"""
    c = [(int(x), int(y)) for x, y in np.asarray(contour, dtype=np.int64).reshape(-1, 2)]
    vymin, vymax = min(p[1] for p in c), max(p[1] for p in c)
    out = []
    for y in range(vymin, vymax):
        out.append(sum(1 for i in range(len(c)) if min(c[i - 1][1], c[i][1]) <= y < max(c[i - 1][1], c[i][1])))
    return out


# ---- seeded 64 x 96 bitmaps the host and the GPU tests share ---------------------------------------------------------------------------------
H, W = 64, 96


def pack_bits(bm):
    """bool [..., h, w] -> uint32 [..., h, w / 32], bit b of word q = column 32 q + b (what pt_det_bitmap writes)"""
    b = np.asarray(bm).reshape(bm.shape[:-1] + (bm.shape[-1] // 32, 32)).astype(np.uint32)
    return (b << np.arange(32, dtype=np.uint32)).sum(axis=-1).astype(np.uint32)


def shape_pages(seed=0):
    """bool [6, 64, 96]: an empty page first and last; seeded blobs; a ring, a plus sign and a 1-pixel diagonal; a checkerboard corner chain
    (pixels that touch by corners only: one 8-connected component, every vertex a turn); components on all four borders"""
    rng = np.random.RandomState(seed)
    p = np.zeros((6, H, W), dtype=bool)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(9):                                                     # page 1: turned blobs
        cx, cy, a, b, th = rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.uniform(3, 20), rng.uniform(1.5, 6), rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        p[1] |= (np.abs(u) < a) & (np.abs(v) < b)
    p[2, 6:24, 8:40] = True                                                # page 2: a ring (outer and hole contour) ...
    p[2, 11:19, 15:33] = False
    p[2, 30:51, 20:25] = True                                              # ... a plus sign ...
    p[2, 38:43, 10:36] = True
    for k in range(22):                                                    # ... and a 1-pixel diagonal: every vertex visited twice
        p[2, 30 + k, 50 + k] = True
    for k in range(20):                                                    # page 3: the corner chain, two pixels wide in places
        p[3, 10 + k, 10 + 2 * k + (k & 1)] = True
        p[3, 11 + k, 11 + 2 * k + (k & 1)] = True
    p[3, 40:60, 30:70] = (xx[40:60, 30:70] + yy[40:60, 30:70]) % 2 == 0    # a checkerboard: ONE component, hundreds of vertices
    p[4, 0:5, 10:40] = True                                                # page 4: all four borders, and a corner
    p[4, H - 4:H, 50:90] = True
    p[4, 20:45, 0:4] = True
    p[4, 15:50, W - 5:W] = True
    p[4, H - 6:H, 0:7] = True
    return p


def kept_contours(bm, max_candidates=1000, min_size=3.0):
    """the contours boxes_from_bitmap scores, in its order: oracle.db_post.candidates_from_bitmap's loop, keeping the contour"""
    out = []
    for c in O.find_contours(bm)[:max_candidates]:
        _, sside = O.get_mini_boxes(c)
        if sside < min_size:
            continue
        out.append(c)
    return out
