"""Seeded head-map cases for DocXLayout's decode (pt_docx_decode, tests/test_gpu_docx_decode.py) and its host chain: one page each, the eight
heads as NCHW float32 arrays [1, C, h, w] at a given map size.  The background is logit -10 (score 4.5e-5); peaks are single pixels with
scores on a grid of 0.004 (so every threshold test, every rank and every NMS score comparison is decided by far more than the sigmoid's
rounding), quads from wh / reg values on a grid of 0.1 px (so that, on a page 4 x the map, no final coordinate falls on a .5).

REF_CASES are compared with the reference's own post-processor (tests/golden/docxlayout_post.*, written by make_golden_docxlayout.py, which
asserts those margins on every case); RULE_CASES hold exact ties -- a plateau, equal scores, equal arg-max maxima, a flat map, the two
logits around 0.3 -- where torch has no rule and the engine's stated rule is tested alone."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

SIZES = [(24, 40), (48, 48)]
REF_CASES = ["few", "many", "borders", "nms", "empty"]
RULE_CASES = ["plateau", "equal_pair", "argmax_tie", "flat", "threshold"]
BG = np.float32(-10.0)
N_MAIN, N_SUB = 11, 2


def page_hw(size) -> Tuple[int, int]:
    """the page the case is decoded for: 4 x the map in both directions"""
    return 4 * size[0], 4 * size[1]


def logit_of(score: float) -> np.float32:
    return np.float32(np.log(score / (1.0 - score)))


def threshold_logits() -> Tuple[np.float32, np.float32]:
    """(the last float32 logit whose torch float32 sigmoid, widened to double, is below 0.3; the next float32: the first at or above it)"""
    import torch
    x = np.float32(np.log(0.3 / 0.7))
    sig = lambda v: float(torch.sigmoid(torch.tensor(v, dtype=torch.float32)))
    while sig(x) >= 0.3:
        x = np.nextafter(x, np.float32(-np.inf))
    while sig(np.nextafter(x, np.float32(np.inf))) < 0.3:
        x = np.nextafter(x, np.float32(np.inf))
    return x, np.nextafter(x, np.float32(np.inf))


def _blank(h: int, w: int, rng) -> Dict[str, np.ndarray]:
    z = {"hm": np.full((1, N_MAIN, h, w), BG, np.float32), "hm_sub": np.full((1, N_SUB, h, w), BG, np.float32)}
    corner = np.array([3.0, 2.0, -3.0, 2.0, -3.0, -2.0, 3.0, -2.0], np.float32)      # TL, TR, BR, BL: corner i = centre - wh[2i:2i+2]
    for k in ("wh", "wh_sub"):
        z[k] = (corner[None, :, None, None] + 0.1 * rng.integers(-3, 4, (1, 8, h, w))).astype(np.float32)
    for k in ("reg", "reg_sub"):
        z[k] = (0.5 + 0.1 * rng.integers(-2, 3, (1, 2, h, w))).astype(np.float32)
    # arg-max inputs: one clear maximum per pixel (0.5 above the rest)
    for k, c in (("cls", 4), ("ftype", 3)):
        v = (0.1 * rng.integers(-5, 6, (1, c, h, w))).astype(np.float32)
        top = rng.integers(0, c, (h, w))
        v[0, top, np.arange(h)[:, None], np.arange(w)[None, :]] = np.float32(1.5)
        z[k] = v
    return z


def _scores(n: int, rng, lo: float = 0.32):
    """n distinct scores on the 0.004 grid, shuffled"""
    s = lo + 0.004 * np.arange(170)
    s = s[s < 0.997]
    assert n <= len(s)
    return rng.permutation(s)[:n]


def _spots(h: int, w: int, n: int, rng, step: int = 2):
    """n distinct pixels on a grid of `step` (never 3x3 neighbours of one another)"""
    ys, xs = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
    pick = rng.permutation(ys.size)[:n]
    assert n <= ys.size
    return ys.reshape(-1)[pick], xs.reshape(-1)[pick]


def _quad(z, key, y, x, half_w, half_h, reg=(0.5, 0.5)):
    z[key][0, :, y, x] = np.array([half_w, half_h, -half_w, half_h, -half_w, -half_h, half_w, -half_h], np.float32)
    z["reg" if key == "wh" else "reg_sub"][0, :, y, x] = np.array(reg, np.float32)


def make_case(name: str, size) -> Dict[str, np.ndarray]:
    h, w = size
    rng = np.random.default_rng(sum(map(ord, name)) * 1000 + h * 64 + w)
    z = _blank(h, w, rng)
    if name == "empty":
        return z
    if name == "few":
        # 30 main peaks over the classes, 6 sub-field peaks; three peaks just below 0.3 (listed by the device, dropped downstream)
        ys, xs = _spots(h, w, 33, rng, 3)
        sc = np.concatenate([_scores(30, rng), [0.2995, 0.2993, 0.2991]])
        for i in range(33):
            z["hm"][0, rng.integers(0, N_MAIN), ys[i], xs[i]] = logit_of(sc[i])
        ys, xs = _spots(h, w, 6, rng, 5)
        for i, s in enumerate(_scores(6, rng)):
            z["hm_sub"][0, i % 2, ys[i], xs[i]] = logit_of(s)
            _quad(z, "wh_sub", ys[i], xs[i], 6.0 + 0.1 * i, 5.0)
        return z
    if name == "many":
        # more than 100 at or above 0.3 in both branches: the rank-100 boundary is a score step of 0.004
        ys, xs = _spots(h, w, 150, rng, 2)
        for i, s in enumerate(_scores(150, rng)):
            z["hm"][0, i % N_MAIN, ys[i], xs[i]] = logit_of(s)
        ys, xs = _spots(h, w, 120, rng, 2)
        for i, s in enumerate(_scores(120, rng)):
            z["hm_sub"][0, i % 2, ys[i], xs[i]] = logit_of(s)
        return z
    if name == "borders":
        # the four corners and the middle of every border; class 10 (last of 11) and sub class 1; the map's first and last pixel
        pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1), (h // 2, w // 2)]
        sc = _scores(2 * len(pts), rng)
        for i, (y, x) in enumerate(pts):
            z["hm"][0, 10 if i % 3 == 0 else i % 10, y, x] = logit_of(sc[i])
            z["hm_sub"][0, 1 if i % 2 == 0 else 0, y, x] = logit_of(sc[len(pts) + i])
        return z
    if name == "nms":
        # corner pixels too (the last page of a batch ends on a peak); then, on integer coordinates (reg 0, integer wh):
        #   a nested pair: A (score .9) holds B's centre -> B goes;
        #   a chain: A2 holds B2's centre, B2 holds C2's, A2 does not hold C2's -> B2 and C2 go (the predicate is order-free);
        #   an edge: E's right edge runs exactly through F's centre -> F stays
        z["hm"][0, 0, 0, 0] = logit_of(0.5)
        z["hm"][0, 10, h - 1, w - 1] = logit_of(0.52)
        z["hm_sub"][0, 1, h - 1, w - 1] = logit_of(0.54)

        def peak(c, y, x, s, hw_, hh_):
            z["hm"][0, c, y, x] = logit_of(s)
            _quad(z, "wh", y, x, hw_, hh_, reg=(0.0, 0.0))

        peak(7, 6, 6, 0.9, 4.0, 3.0)
        peak(2, 7, 8, 0.6, 1.0, 1.0)
        peak(7, 14, 6, 0.92, 3.0, 2.0)
        peak(2, 14, 8, 0.7, 3.0, 1.0)
        peak(3, 14, 10, 0.4, 1.0, 1.0)
        peak(1, 20, 10, 0.8, 4.0, 2.0)      # right edge at x = 14
        peak(4, 20, 14, 0.44, 1.0, 1.0)     # centre (14, 20)
        return z
    if name == "plateau":
        z["hm"][0, 3, 5:7, 9:11] = logit_of(0.7)
        z["hm_sub"][0, 1, 2:4, 2:4] = logit_of(0.6)
        return z
    if name == "equal_pair":
        # two peaks of one score, each holding the other's centre: neither is suppressed
        for x in (8, 11):
            z["hm"][0, 5, 9, x] = logit_of(0.8)
            _quad(z, "wh", 9, x, 5.0, 3.0, reg=(0.0, 0.0))
        return z
    if name == "argmax_tie":
        z["hm"][0, 6, 4, 4] = logit_of(0.75)
        z["cls"][0, :, 4, 4] = np.array([0.2, 1.5, 1.5, 0.1], np.float32)
        z["ftype"][0, :, 4, 4] = np.array([1.5, 1.5, 1.5], np.float32)
        return z
    if name == "flat":
        z["hm"][:] = np.float32(0.0)
        z["hm_sub"][:] = np.float32(0.25)
        return z
    if name == "threshold":
        below, above = threshold_logits()
        z["hm"][0, 1, 3, 3] = above
        z["hm"][0, 1, 3, 9] = below
        z["hm_sub"][0, 0, 3, 3] = below
        z["hm_sub"][0, 0, 3, 9] = above
        return z
    raise KeyError(name)


def stack(cases, size) -> Dict[str, np.ndarray]:
    """several pages' cases as one batch"""
    zs = [make_case(c, size) for c in cases]
    return {k: np.concatenate([z[k] for z in zs], 0) for k in zs[0]}
