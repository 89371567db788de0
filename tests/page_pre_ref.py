"""numpy restatement of the image-page deskew (PdfImageProcessor.rotate_image, utils/table/image_processing.py:500-) for the tests of
csrc/page_pre.hip, the host tracer pt_page_line_angles and PagePreStage.  Test infrastructure only: nothing in pdf_table_amd/ imports it.

The reference delegates every step to OpenCV, which is neither vendored nor installed here, so each restatement below is UNPINNED.  What
it assumes about cv2, for a later check against real OpenCV:

* cvtColor(BGR2GRAY), 8 bit: (B * 1868 + G * 9617 + R * 4899 + 2^13) >> 14 on the reference's BGR page; our pages are RGB, so the same
  weights apply to (channel 2, 1, 0) = (B, G, R).  Then gray = 255 - gray.
* GaussianBlur(15 x 15, sigma 0, BORDER_REPLICATE | BORDER_ISOLATED) on CV_8U takes the bit-exact fixed-point path:
  - taps: getGaussianKernelBitExact (sigma = fma(15, 0.15, 0.35) = 2.6; t_i = exp((x_i^2) * (-0.125 / sigma^2)) with x_i = 2 i - 14,
    normalised by 1 / (2 sum t_i + 1)) turned into ufixedpoint16 (8 fractional bits) by getGaussianKernelFixedPoint_ED: the outer taps
    rounded half-to-even with the rounding error carried to the next tap, the centre tap = 256 - the others (sum exactly 256, symmetric);
  - row pass: uint8 x ufixedpoint16 summed exactly into ufixedpoint16 (max 255 * 256 fits 16 bits, no rounding);
  - column pass: ufixedpoint16 x ufixedpoint16 summed into ufixedpoint32, then (v + 2^15) >> 16 to uint8.
  Because the row pass does not round, the result is (sum_ij k_i k_j g + 2^15) >> 16 in either pass order.
  exp is taken from the C library here; OpenCV's softdouble exp may differ in the last bit of a tap before rounding to 8 bits.
* adaptiveThreshold(255, GAUSSIAN_C, BINARY, 15, C = -2): idelta = ceil(-2); 255 where gray - mean > 2.
* erode then dilate with getStructuringElement(MORPH_RECT, (w // 40, 1)), anchor (L // 2, 0), no kernel reflection for dilate:
  dst(x) = min / max over src(x + i - L // 2), 0 <= i < L; the default border value is 255 for erode and 0 for dilate.
* findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE): OpenCV's scan mode 0 on top of the border follower of oracle/db_post.py (which
  restates icvFetchContour); contours in reverse discovery order.
* calculate_angle: np.arctan(k) * 57.29577; restated with math.atan (the C library's atan, what the host tracer calls).
* getRotationMatrix2D((w // 2, h // 2), angle, 1) with angle * (pi / 180), cos / sin in fp64; warpAffine inverts it in fp64 (D = 1 / det,
  A11 = M4 D, A22 = M0 D, M1 *= -D, M3 *= -D, b = -A M[:, 2]).
* warpAffine INTER_CUBIC, BORDER_REPLICATE: 10-bit fixed-point coordinates, 1/32-pixel positions (as tsr_preprocess_kernel), the 32 x 32
  x 16 table of initInterTab2D (interpolateCubic with A = -0.75 in float32, v * 32768 rounded to int16, each entry adjusted to sum 32768
  on the largest / smallest of its four central taps), taps at sx - 1 .. sx + 2 clamped, (acc + 2^14) >> 15 saturated.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle.db_post import _trace

DIFF_ANGLE = 400
ANGLE_THRESHOLD = 0.2
LINE_SCALE = 40


def gaussian_taps(n: int = 15) -> np.ndarray:
    n2 = n // 2
    # fma(n, 0.15, 0.35): the exact product plus 0.35, rounded once
    sigma = float(Fraction(n) * Fraction(0.15) + Fraction(0.35))
    scale2 = -0.125 / (sigma * sigma)
    v = []
    s = 0.0
    for i in range(n2):
        x = 2 * i + 1 - n
        t = math.exp(float(x * x) * scale2)
        v.append(t)
        s += t
    s *= 2
    s += 1
    mul1 = 1.0 / s
    k = np.zeros(n, np.int64)
    err = 0.0
    tot = 0
    for i in range(n2):
        adj = v[i] * mul1 * 256.0 + err
        v0 = round(adj)               # half to even, as cvRound
        err = adj - v0
        k[i] = k[n - 1 - i] = v0
        tot += v0
    k[n2] = 256 - 2 * tot
    return k


def gray_inv(page: np.ndarray) -> np.ndarray:
    p = page.astype(np.int64)
    return 255 - ((p[..., 0] * 4899 + p[..., 1] * 9617 + p[..., 2] * 1868 + 8192) >> 14)


def blur(g: np.ndarray) -> np.ndarray:
    k = gaussian_taps()
    h, w = g.shape
    ys = np.clip(np.arange(h)[:, None] + np.arange(15)[None] - 7, 0, h - 1)        # [h, 15]
    V = (g[ys] * k[None, :, None]).sum(1)                                           # [h, w]
    xs = np.clip(np.arange(w)[:, None] + np.arange(15)[None] - 7, 0, w - 1)        # [w, 15]
    S = (V[:, xs] * k[None, None, :]).sum(2)
    return (S + (1 << 15)) >> 16


def threshold(page: np.ndarray) -> np.ndarray:
    g = gray_inv(page)
    return (g - blur(g)) > 2


def opening(t: np.ndarray, L: int) -> np.ndarray:
    a = L // 2
    tp = np.pad(t, ((0, 0), (a, L - 1 - a)), constant_values=True)
    e = sliding_window_view(tp, L, axis=1).all(-1)
    ep = np.pad(e, ((0, 0), (a, L - 1 - a)), constant_values=False)
    return sliding_window_view(ep, L, axis=1).any(-1)


def line_mask(page: np.ndarray) -> np.ndarray:
    """bool [h, w]: the opened horizontal-line mask of one RGB page (w >= 40)"""
    return opening(threshold(page), page.shape[1] // LINE_SCALE)


def pack_bits(mask: np.ndarray) -> np.ndarray:
    """bool [..., h, w] -> uint64 [..., h, (w + 63) // 64], bit b of word q = column 64 q + b"""
    w = mask.shape[-1]
    nw = (w + 63) // 64
    m = np.zeros(mask.shape[:-1] + (nw * 64,), np.uint8)
    m[..., :w] = mask
    by = np.packbits(m, axis=-1, bitorder="little")
    return by.reshape(mask.shape[:-1] + (nw, 8)).view("<u8")[..., 0]


def external_contours(mask: np.ndarray):
    """cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) -> list of int [k, 2] (x, y), cv2's order"""
    h, w = mask.shape
    img = np.zeros((h + 2, w + 2), np.int32)
    img[1:-1, 1:-1] = np.asarray(mask) != 0
    found = []
    for y in np.nonzero(img.any(1))[0].tolist():
        row = img[y]
        prev, lnbd, x = 0, 0, 1
        while x <= w:
            d = np.nonzero(row[x:w + 1] != prev)[0]
            if not len(d):
                break
            x += int(d[0])
            p = int(row[x])
            if prev == 0 and p == 1:
                if row[lnbd] <= 0:               # not inside the hole of a traced component
                    found.append(_trace(img, x, y, False))
                    lnbd = x
            elif p == 0 and prev >= 1 and (prev & -2):
                lnbd = x - 1
            prev = int(row[x])
            if prev & -2:
                lnbd = x
            x += 1
    found.reverse()
    return [np.array(c, dtype=np.int64).reshape(-1, 2) - 1 for c in found]


def calculate_angle(p1, p2) -> float:
    dx, dy = float(p2[0]) - float(p1[0]), float(p2[1]) - float(p1[1])
    if dx == 0:
        return 90.0
    if dy == 0:
        return 0.0
    return math.atan(dy / dx) * 57.29577


def get_line_angle(pts: np.ndarray) -> float:
    pts = np.asarray(pts).reshape(-1, 2)
    width = pts[:, 0].max() - pts[:, 0].min()
    height = pts[:, 1].max() - pts[:, 1].min()
    lst = pts.tolist()
    lst = sorted(lst, key=lambda p: p[0]) if width > height else sorted(lst, key=lambda p: p[1])
    return calculate_angle(lst[0], lst[-1])


def line_angles(mask: np.ndarray, min_width: int = DIFF_ANGLE) -> list:
    out = []
    for c in external_contours(mask):
        if c[:, 0].max() - c[:, 0].min() + 1 > min_width:
            out.append(get_line_angle(c))
    return out


def average_angle(angles):
    f = [a for a in angles if a != 0 and a != 90]
    return np.average(f) if len(f) > 0 else None


def rotation_minv(h: int, w: int, angle: float) -> np.ndarray:
    cx, cy = float(w // 2), float(h // 2)
    a = angle * (math.pi / 180)
    al, be = math.cos(a), math.sin(a)
    M = [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return np.array(M, np.float64)


def cubic_table() -> np.ndarray:
    f = np.float32
    A = f(-0.75)
    t1 = np.zeros((32, 4), np.float32)
    for i in range(32):
        x = f(i) * f(1.0 / 32)
        one = f(1)
        c0 = ((A * (x + one) - f(5) * A) * (x + one) + f(8) * A) * (x + one) - f(4) * A
        c1 = ((A + f(2)) * x - (A + f(3))) * x * x + one
        c2 = ((A + f(2)) * (one - x) - (A + f(3))) * (one - x) * (one - x) + one
        c3 = one - c0 - c1 - c2
        t1[i] = [c0, c1, c2, c3]
    tab = np.zeros((1024, 16), np.int64)
    for i in range(32):
        for j in range(32):
            it = tab[i * 32 + j]
            for k1 in range(4):
                for k2 in range(4):
                    v = np.float32(t1[i, k1] * t1[j, k2])
                    it[k1 * 4 + k2] = min(32767, max(-32768, int(np.rint(np.float32(v * np.float32(32768))))))
            diff = int(it.sum()) - 32768
            if diff:
                Mk, mk = (2, 2), (2, 2)
                for k1 in (2, 3):
                    for k2 in (2, 3):
                        if it[k1 * 4 + k2] < it[mk[0] * 4 + mk[1]]:
                            mk = (k1, k2)
                        elif it[k1 * 4 + k2] > it[Mk[0] * 4 + Mk[1]]:
                            Mk = (k1, k2)
                if diff < 0:
                    it[Mk[0] * 4 + Mk[1]] -= diff
                else:
                    it[mk[0] * 4 + mk[1]] -= diff
    return tab


_CUBIC = None


def warp_cubic(page: np.ndarray, minv: np.ndarray) -> np.ndarray:
    """cv2.warpAffine(page, M, (w, h), INTER_CUBIC, BORDER_REPLICATE) given warpAffine's inverse map minv"""
    global _CUBIC
    if _CUBIC is None:
        _CUBIC = cubic_table()
    h, w = page.shape[:2]
    M = np.asarray(minv, np.float64)

    def sat(v):
        return np.clip(np.rint(v), -2147483648.0, 2147483647.0).astype(np.int64)
    xs = np.arange(w, dtype=np.float64)
    ys = np.arange(h, dtype=np.float64)
    adelta, bdelta = sat(M[0] * xs * 1024.0), sat(M[3] * xs * 1024.0)
    X0, Y0 = sat((M[1] * ys + M[2]) * 1024.0) + 16, sat((M[4] * ys + M[5]) * 1024.0) + 16
    X = (X0[:, None] + adelta[None]) >> 5
    Y = (Y0[:, None] + bdelta[None]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    wt = _CUBIC[((Y & 31) << 5) | (X & 31)]                 # [h, w, 16]
    src = page.astype(np.int64)
    acc = np.zeros((h, w, 3), np.int64)
    for k1 in range(4):
        yy = np.clip(sy - 1 + k1, 0, h - 1)
        for k2 in range(4):
            xx = np.clip(sx - 1 + k2, 0, w - 1)
            acc += src[yy, xx] * wt[..., k1 * 4 + k2, None]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def skew_angle(page: np.ndarray) -> float:
    """get_image_rotate_angle_v2's horizontal angle, 0 when there is none"""
    a = average_angle(line_angles(line_mask(page)))
    return 0.0 if a is None else float(a)


def deskew(page: np.ndarray):
    """PdfImageProcessor.rotate_image with pre_rotate_image's arguments -> (page, measured angle)"""
    if page.shape[1] < LINE_SCALE:
        return page, 0.0
    ang = skew_angle(page)
    if abs(ang) < ANGLE_THRESHOLD:
        return page, ang
    return warp_cubic(page, rotation_minv(page.shape[0], page.shape[1], ang)), ang
