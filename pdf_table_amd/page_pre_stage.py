"""Image-page straightening before detection: OcrSystemTask.image_pre_process (ocr_system_task.py:441-491) steps 1 to 3.

* deskew: PdfImageProcessor.rotate_image with pre_rotate_image's arguments (ocr_table_preprocess_task.py:85-114) -- the opened
  horizontal-line mask on the device (pt_page_line_mask), the RETR_EXTERNAL line angles on the host (pt_page_line_angles, 16 threads),
  np.average of those that are neither 0 nor 90, and a cubic warp (pt_page_warp_cubic) of the pages whose |angle| >= 0.2.
* orient: OcrTablePreprocessTask.rotate_image_v2 (ocr_table_preprocess_task.py:116-163) -- the text_image_orientation classifier; a
  page it calls "90", "180" or "270" with a score above 0.6 (ImagePreProcessOutput.check_rotate, entity/table_entity.py:711-727) is
  turned by that label (rotate_image_angle_v2: ROTATE_90_CLOCKWISE / ROTATE_180 / ROTATE_90_COUNTERCLOCKWISE) and classified again; the
  turn is kept only when the second label is "0" or "180".  table_attribute, when asked, runs on the first pass.
* sideways: TableProcessUtils.check_pdf_text_need_rotate90 (table_common.py:1617-1640) on the detected boxes; such a page is turned
  with ROTATE_90_COUNTERCLOCKWISE (pt_page_quarter_turn) and detected again by the caller.

Deviations: nothing is written back to a file and re-read; a page without boxes is not turned (the reference divides
0 by 0); pages narrower than 40 pixels are not deskewed (cv2 rejects the zero-width structuring element), nor pages wider than the mask
kernel takes (mask_fits).
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import engine as E
from . import lib as L
from .rec_stage import order_points

DIFF_ANGLE = 400          # pre_rotate_image: diff_angle
ANGLE_THRESHOLD = 0.2     # pre_rotate_image: angle_threshold
LINE_SCALE = 40           # line_scale_horizontal
ORIENT_SCORE = 0.6        # ImagePreProcessOutput.check_rotate
ORIENT_CODES = {"90": L.PT_ROTATE_90_CLOCKWISE, "180": L.PT_ROTATE_180, "270": L.PT_ROTATE_90_COUNTERCLOCKWISE}


def mask_fits(w: int) -> bool:
    """pt_page_line_mask accepts the width: >= 40 (cv2's structuring element) and a band of >= 2 rows within 64 KiB of LDS (page_pre.hip
    mask_lds<2>: about 14 500 pixels); wider pages are not deskewed"""
    nw = (w + 63) // 64
    return w >= LINE_SCALE and 2 * nw * 8 * 2 + 2 * w * 2 <= 65536


def orientation_turn(first: dict):
    """check_rotate on the first classification -> the label to turn by ("90" / "180" / "270"), or None"""
    label, score = first["label_names"][0], first["scores"][0]
    return label if score > ORIENT_SCORE and label != "0" and label in ORIENT_CODES else None


def orientation_keep(second: dict) -> bool:
    """rotate_image_v2: the turned page is kept when its own classification says "0" or "180" """
    return second["label_names"][0] in ("0", "180")


def rotation_minv(h: int, w: int, angle: float) -> np.ndarray:
    """the inverse map cv2.warpAffine computes in fp64 from cv2.getRotationMatrix2D((w // 2, h // 2), angle, 1.0)"""
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


def average_angle(angles) -> float:
    """PdfImageProcessor.average_angle, then get_image_rotate_angle_v2's `angle = 0` when there is none"""
    f = [a for a in angles if a != 0 and a != 90]
    return float(np.average(f)) if len(f) > 0 else 0.0


def sideways_ratio(boxes: np.ndarray):
    """sum |p0.x - p2.x| / sum |p0.y - p2.y| over the boxes after order_point; None without boxes (the reference divides 0 by 0)"""
    b = np.asarray(boxes).reshape(-1, 4, 2)
    if not len(b):
        return None
    p = order_points(b)
    w = float(np.abs(p[:, 0, 0] - p[:, 2, 0]).sum())
    h = float(np.abs(p[:, 0, 1] - p[:, 2, 1]).sum())
    return w / h if h > 0 else math.inf


def needs_turn(boxes: np.ndarray) -> bool:
    """check_pdf_text_need_rotate90: the page is turned when its boxes are, in sum, taller than wide (ratio < 1)"""
    r = sideways_ratio(boxes)
    return r is not None and r < 1


class PagePreStage:
    def __init__(self, engine, n_threads: int = 16):
        self.engine = engine
        self.n_threads = max(1, min(16, int(n_threads)))

    def measure(self, pages: torch.Tensor) -> List[float]:
        """the deskew angle of every page of a same-shape batch (0 for pages the mask kernel does not take: mask_fits)"""
        n, h, w, _ = pages.shape
        if not mask_fits(w):
            return [0.0] * n
        bits = self.engine.page_line_mask(pages).cpu().numpy()          # one copy of the bits
        return [average_angle(a) for a in E.page_line_angles(bits, w, DIFF_ANGLE, self.n_threads)]

    def deskew(self, pages: torch.Tensor) -> Tuple[torch.Tensor, List[float]]:
        """same-shape uint8 RGB pages [n, h, w, 3] -> (pages with the skewed ones warped back, measured angles).  The input is not changed."""
        n, h, w, _ = pages.shape
        angles = self.measure(pages)
        idx = [i for i, a in enumerate(angles) if abs(a) >= ANGLE_THRESHOLD]
        if not idx:
            return pages, angles
        warped = self.engine.page_warp_cubic(pages, np.stack([rotation_minv(h, w, angles[i]) for i in idx]), idx)
        if len(idx) == n:
            return warped, angles
        out = pages.clone()
        out[torch.tensor(idx, device=pages.device)] = warped
        return out, angles

    def turn(self, pages: torch.Tensor, code: int) -> torch.Tensor:
        """cv2.rotate of every page (L.PT_ROTATE_90_CLOCKWISE / _180 / _90_COUNTERCLOCKWISE)"""
        return self.engine.page_quarter_turn(pages, code)

    def orient(self, pages: torch.Tensor, orientation, attribute=None):
        """same-shape pages [n, h, w, 3] -> (groups, metrics, attributes).  orientation / attribute: ClsStage of text_image_orientation /
        table_attribute (or None).  groups: [(page indices, uint8 tensor [k, h', w', 3])] by final shape; metrics per page: {"angle",
        "score"} plus {"angle2", "score2"} when a second pass ran (rotate_image_v2's metric); attributes: table_attribute_postprocess of
        the first pass per page, or None.  One classification of the batch, one turn per label, one classification per turned shape."""
        n = pages.shape[0]
        first = orientation.pages(pages)
        attrs = attribute.pages(pages) if attribute is not None else None
        metrics = [{"angle": r["label_names"][0], "score": r["scores"][0]} for r in first]
        by_label: dict = {}
        for i, r in enumerate(first):
            lab = orientation_turn(r)
            if lab is not None:
                by_label.setdefault(lab, []).append(i)
        turned = {}                                  # page -> its turned tensor
        for lab, idx in by_label.items():
            t = self.turn(pages[torch.tensor(idx, device=pages.device)].contiguous(), ORIENT_CODES[lab])
            for k, i in enumerate(idx):
                turned[i] = t[k]
        by_shape: dict = {}
        for i in sorted(turned):
            by_shape.setdefault(tuple(turned[i].shape), []).append(i)
        keep = set()
        for shape, idx in by_shape.items():
            second = orientation.pages(torch.stack([turned[i] for i in idx]))
            for i, r in zip(idx, second):
                metrics[i]["angle2"], metrics[i]["score2"] = r["label_names"][0], r["scores"][0]
                if orientation_keep(r):
                    keep.add(i)
        final: dict = {}
        for i in range(n):
            t = turned[i] if i in keep else pages[i]
            final.setdefault(tuple(t.shape), []).append((i, t))
        groups = []
        for shape, items in final.items():
            idx = [i for i, _ in items]
            if len(idx) == n and all(i not in keep for i in idx):
                groups.append((idx, pages))
            else:
                groups.append((idx, torch.stack([t for _, t in items])))
        return groups, metrics, attrs

    @staticmethod
    def sideways(boxes_per_page: Sequence[np.ndarray]) -> np.ndarray:
        """bool [n]: the pages to turn by ROTATE_90_COUNTERCLOCKWISE and detect again"""
        return np.array([needs_turn(b) for b in boxes_per_page], dtype=bool)

    def straighten(self, pages: Sequence[np.ndarray], deskew: bool = True, orientation=None, attribute=None):
        """host pages of any shapes -> (device pages [h, w, 3] per page, deskew angles or None, orientation metrics or None, table attributes
        or None).  Each shape group is uploaded once; deskew then orient on the device, nothing comes back to the host but the mask bits."""
        n = len(pages)
        dev: List[torch.Tensor] = [None] * n
        angles = [None] * n
        metrics = [None] * n
        attrs = [None] * n
        groups: dict = {}
        for i, p in enumerate(pages):
            groups.setdefault(p.shape, []).append(i)
        for shape, idxs in groups.items():
            batch = torch.from_numpy(np.stack([pages[i] for i in idxs])).to(self.engine._tdev)
            if deskew:
                batch, ang = self.deskew(batch)
                for i, a in zip(idxs, ang):
                    angles[i] = a
            if orientation is None:
                for k, i in enumerate(idxs):
                    dev[i] = batch[k]
                continue
            parts, met, att = self.orient(batch, orientation, attribute)
            for k, i in enumerate(idxs):
                metrics[i] = met[k]
                if att is not None:
                    attrs[i] = att[k]
            for sub, t in parts:
                for k, j in enumerate(sub):
                    dev[idxs[j]] = t[k]
        return dev, angles, metrics, attrs
