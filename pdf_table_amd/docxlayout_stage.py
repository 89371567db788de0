"""Batched layout detection with DocXLayout (DLA-34 + DLAUp + eight heads): warp, network, peaks, top-K and polygon NMS on the GPU, the
ordering of the few dozen regions of a page on the host.

Replaces, for a batch of equally sized resident pages, the reference's per-page chain ``DocXLayoutPreProcessor.do_preprocess``
(docx_layout/image_processing_docxlayout.py:124-164) -> ``DocXLayoutModel.forward`` (modeling_docxlayout.py:75-93: DLASeg) ->
``DocXLayoutImagePostProcessor.post_process`` (:223-459).  The device half ends in ``pt_docx_decode``: per page and branch (main: 11
classes, sub-fields: 2) the first ``top_k`` peaks at or above a threshold just below ``scores_thresh`` in (score, index) order, their quads
in head-map pixels, the ``cls`` / ``ftype`` arg-max columns and the keep flags of ``pnms``.  The host half maps the kept quads to page
pixels, applies the reference's exact threshold rules, and orders the regions with its comparator sort.  ``DocXLayoutStage(device_order=True)``
moves that half into one more launch (``pt_op_docx_order``, csrc/docx_order.hip); the host code here stays its specification and its fallback.

Deviations, both in code the reference cannot run here (``shapely`` is not installed) or would raise in:
  * ``quad_intersection_rate`` restates ``pts_intersection_rate`` for convex quads (Sutherland-Hodgman clipping, shoelace areas, float64).
    A zero-area source gives rate 0 (the reference divides by zero); when either quad is not convex the rate is computed on the two
    bounding boxes.  The reference's own polygon library is not pinned by a fixture: tests/golden/make_golden_docxlayout.py injects this same
    function as its ``shapely.geometry.Polygon`` stand-in.
  * the comparator's last rule divides by the taller block's height; two blocks of height 0 compare by their centres instead of raising.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from functools import cmp_to_key
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from .centernet_stage import centernet_decode_affine
from .engine import TSR_TABLE_DTYPE, HipEngine
from .layout_stage import LayoutStage
from .tsr_stage import lore_geometry

__all__ = ["DocXLayoutConfig", "DocXLayoutStage", "load_checkpoint", "quad_intersection_rate", "sort_blocks", "docx_page_result",
           "DOCX_LABELS", "DOCX_MEAN", "DOCX_STD"]

DOCX_LABELS = ["title", "figure", "text", "header", "page_number", "footnote", "footer", "table", "table_caption", "figure_caption", "equation",
               "full_column", "sub_column"]                  # configuration_docxlayout.py:57-72
DOCX_MEAN = (0.40789655, 0.44719303, 0.47026116)             # image_processing_docxlayout.py:110-111, applied to B, G, R
DOCX_STD = (0.2886383, 0.27408165, 0.27809834)
N_MAIN = 11                                                  # classes of the hm head; the sub-field classes follow


@dataclass
class DocXLayoutConfig:
    """configuration_docxlayout.py:20-72 (inference fields) and the pre-processor's fixed input size (image_processing_docxlayout.py:114-119)"""
    model_name: str = "DocXLayout"
    backbone: str = "dla34"
    task_type: str = "general"
    top_k: int = 100
    scores_thresh: float = 0.3
    num_classes: int = 13
    use_nms: bool = True
    model_path: str = ""
    resolution: Tuple[int, int] = (768, 768)                 # (input_h, input_w)
    labels: List[str] = field(default_factory=lambda: list(DOCX_LABELS))

    def __post_init__(self):
        self.label2id = {name: i for i, name in enumerate(self.labels)}
        self.id2label = dict(enumerate(self.labels))


def load_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """What ``DocXLayoutModel.load_model`` -> ``load_checkpoint`` (modeling_docxlayout.py:72-73, table/lgpma/checkpoint.py) would read: a ``.pth`` /
    ``.bin`` / ``.pt`` file, or a directory holding ``pytorch_model.bin`` (else the single ``*.pth`` in it); its ``state_dict`` entry if present;
    a leading ``module.`` stripped from every key.  A state dict without one of the eight heads raises ``KeyError`` naming the key.

    The reference's task builds ``DocXLayoutConfig()`` with an empty ``model_path`` and only then assigns the path (ocr_layout_task.py:46-53 sets it
    after the config, but ``DocXLayoutModel.__init__`` tests ``config.model_path`` of the config it is given), so whether its own door ever loads a
    file depends on that order; this loader is what ``load_model`` does once it runs."""
    f = str(path)
    if os.path.isdir(f):
        cand = os.path.join(f, "pytorch_model.bin")
        if not os.path.isfile(cand):
            pths = sorted(p for p in os.listdir(f) if p.endswith(".pth"))
            if len(pths) != 1:
                raise RuntimeError(f"no DocXLayout checkpoint under {f}: expected pytorch_model.bin or a single *.pth file, found {pths or 'none'}")
            cand = os.path.join(f, pths[0])
        f = cand
    elif not (os.path.isfile(f) and f.endswith((".pth", ".bin", ".pt"))):
        raise RuntimeError(f"no DocXLayout checkpoint at {f}: pass a .pth / .bin / .pt file or a directory holding pytorch_model.bin")
    ck = torch.load(f, map_location="cpu", weights_only=True)
    if isinstance(ck, dict) and "state_dict" in ck:
        ck = ck["state_dict"]
    sd = {(str(k)[len("module."):] if str(k).startswith("module.") else str(k)): v for k, v in ck.items()}
    from .weights import DOCX_HEADS
    for h, _ in DOCX_HEADS:
        for k in (f"{h}.0.weight", f"{h}.0.bias", f"{h}.2.weight", f"{h}.2.bias"):
            if k not in sd:
                raise KeyError(f"DocXLayout checkpoint {f} lacks '{k}'")
    return sd


# ---- polygon overlap (pts_intersection_rate, processor_utils.py:421-430) ---------------------------------------------------------------------
def _shoelace(poly: Sequence[Tuple[float, float]]) -> float:
    """signed area: positive when the vertices run counter-clockwise in a y-up frame"""
    s = 0.0
    for i in range(len(poly)):
        x0, y0 = poly[i]
        x1, y1 = poly[(i + 1) % len(poly)]
        s += x0 * y1 - x1 * y0
    return 0.5 * s


def _is_convex(poly) -> bool:
    sign = 0
    n = len(poly)
    for i in range(n):
        ax, ay = poly[i]
        bx, by = poly[(i + 1) % n]
        cx, cy = poly[(i + 2) % n]
        cr = (bx - ax) * (cy - by) - (by - ay) * (cx - bx)
        if cr != 0:
            if sign and (cr > 0) != (sign > 0):
                return False
            sign = 1 if cr > 0 else -1
    return True


def _clip(subject, clip):
    """Sutherland-Hodgman: `subject` cut by every edge of the convex, counter-clockwise `clip`"""
    out = list(subject)
    n = len(clip)
    for i in range(n):
        if not out:
            break
        ax, ay = clip[i]
        bx, by = clip[(i + 1) % n]
        ex, ey = bx - ax, by - ay
        inp, out = out, []
        side = [ex * (py - ay) - ey * (px - ax) for px, py in inp]
        for k in range(len(inp)):
            p, q = inp[k], inp[(k + 1) % len(inp)]
            sp, sq = side[k], side[(k + 1) % len(inp)]
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def quad_intersection_rate(src: Sequence[float], tgt: Sequence[float]) -> float:
    """area(src & tgt) / area(src) for two quads given as 8 coordinates each (module docstring: convex quads are clipped, anything else is
    compared by bounding box; a zero-area source gives 0)"""
    a = [(float(src[k]), float(src[k + 1])) for k in range(0, 8, 2)]
    b = [(float(tgt[k]), float(tgt[k + 1])) for k in range(0, 8, 2)]
    if not (_is_convex(a) and _is_convex(b)):
        a = _bbox_quad(a)
        b = _bbox_quad(b)
    area_a, area_b = _shoelace(a), _shoelace(b)
    if area_a == 0.0 or area_b == 0.0:
        return 0.0
    if area_a < 0:
        a = a[::-1]
    if area_b < 0:
        b = b[::-1]
    inter = _clip(a, b)
    return abs(_shoelace(inter)) / abs(area_a) if len(inter) >= 3 else 0.0


def _bbox_quad(poly):
    xs, ys = [p[0] for p in poly], [p[1] for p in poly]
    return [(min(xs), min(ys)), (max(xs), min(ys)), (max(xs), max(ys)), (min(xs), max(ys))]


# ---- reading order (sort_pts, processor_utils.py:246-418) ---------------------------------------------------------------------------------------
def _main_angle(pts_list) -> float:
    """the median direction of the first edge: of the blocks more than three times as wide as high if there are any, else of all"""
    wide, rest = [], []
    for p in pts_list:
        ex, ey = p[2] - p[0], p[3] - p[1]
        fx, fy = p[4] - p[2], p[5] - p[3]
        (wide if math.sqrt(ex ** 2 + ey ** 2) > math.sqrt(fx ** 2 + fy ** 2) * 3 else rest).append(math.atan2(ey, ex))
    pick = wide or rest
    if not pick:
        return 0
    pick.sort()
    return pick[len(pick) // 2]


def _relation(lo_a, len_a, lo_b, len_b) -> int:
    """how interval a lies to interval b on one axis (calc_x_type / calc_y_type are this one rule): 1 before, 2 after, 3 overlapping from before,
    4 overlapping from after, 5 a contains b, 6 a inside b"""
    hi_a, hi_b = lo_a + len_a, lo_b + len_b
    start = 1 if lo_a < lo_b else (-1 if lo_a > lo_b else 0)
    end = 1 if hi_a > hi_b else (-1 if hi_a < hi_b else 0)
    if hi_a < lo_b + 1e-4 and hi_a < hi_b - 1e-4:
        return 1
    if lo_a > hi_b - 1e-4 and lo_a > lo_b + 1e-4:
        return 2
    if start == 1 and end == -1:
        return 3
    if start == -1 and end == 1:
        return 4
    if start >= 0 and end >= 0:
        return 5
    if start <= 0 and end <= 0:
        return 6
    return 0


def _compare_rects(ra, rb, thres: float = 0.5) -> int:
    """cmp_pts_udlr on two rotated rectangles (min x, min y, width, height): rows first, columns inside a row.  NOT a total order."""
    lx_a, ly_a, hx_a, hy_a = ra[0], ra[1], ra[0] + ra[2], ra[1] + ra[3]
    lx_b, ly_b, hx_b, hy_b = rb[0], rb[1], rb[0] + rb[2], rb[1] + rb[3]
    xt, yt = _relation(ra[0], ra[2], rb[0], rb[2]), _relation(ra[1], ra[3], rb[1], rb[3])
    if yt == 1:
        return -1
    if yt == 2:
        return 1
    if yt == 3:
        near = (hy_a - ly_b) / min(hy_a - ly_a, hy_b - ly_b)
        return (-1 if near < thres else 1) if xt in (2, 4) else -1
    if yt == 4:
        near = (hy_b - ly_a) / min(hy_a - ly_a, hy_b - ly_b)
        return (1 if near < thres else -1) if xt in (1, 3) else 1
    if xt in (1, 3):
        return -1
    if xt in (2, 4):
        return 1
    diff = abs(0.5 * (ly_a + hy_a) - 0.5 * (ly_b + hy_b))
    tall = max(hy_a - ly_a, hy_b - ly_b)
    same_row = (diff == 0) if tall == 0 else (diff / tall < 0.1)
    ka, kb = ((lx_a + hx_a), (lx_b + hx_b)) if same_row else ((ly_a + hy_a), (ly_b + hy_b))
    return -1 if ka < kb else (1 if ka > kb else 0)


def sort_blocks(blocks: List[Dict]) -> None:
    """sort_pts: in place, by the comparator above on every block's bounding rectangle in the frame turned by the main angle.  The comparator
    is not a total order, so the result depends on the algorithm and on the initial order: ``list.sort`` over the caller's order, as in the
    reference.  The rectangle of a block is computed once, not per comparison (same values)."""
    ang = _main_angle([b["pts"] for b in blocks])
    sn, cs = math.sin(ang), math.cos(ang)

    def rect(pts):
        xs = [pts[k] * cs + pts[k + 1] * sn for k in range(0, len(pts), 2)]
        ys = [pts[k + 1] * cs - pts[k] * sn for k in range(0, len(pts), 2)]
        return (min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys))

    rects = {id(b): rect(b["pts"]) for b in blocks}
    blocks.sort(key=cmp_to_key(lambda a, b: _compare_rects(rects[id(a)], rects[id(b)])))


# ---- the host half (post_process_bbox .. post_process, image_processing_docxlayout.py:223-459) ----------------------------------------------
def _to_page(rows: np.ndarray, inv: np.ndarray) -> np.ndarray:
    """ctdet_4ps_post_process: every vertex (float32) through the float64 inverse map, the row stored as float32"""
    out = np.asarray(rows, np.float32).copy()
    p = out[:, :8].astype(np.float64).reshape(-1, 4, 2)
    q = np.empty_like(p)
    q[..., 0] = inv[0, 0] * p[..., 0] + inv[0, 1] * p[..., 1] + inv[0, 2]
    q[..., 1] = inv[1, 0] * p[..., 0] + inv[1, 1] * p[..., 1] + inv[1, 2]
    out[:, :8] = q.reshape(-1, 8).astype(np.float32)
    return out


def _per_class(rows: np.ndarray, num_classes: int, thresh: float) -> Dict[int, np.ndarray]:
    """the per-class split (1-based keys) and duplicate_removal: rows with float32 score > thresh, or ONE all-zero placeholder row"""
    t = np.float32(thresh)
    out = {}
    for j in range(num_classes):
        r = rows[(rows[:, 9] == j) & (rows[:, 8] > t)]
        out[j + 1] = r if len(r) else np.zeros((1, 12), np.float32)
    return out


def docx_page_result(main_rows: np.ndarray, sub_rows: np.ndarray, page_hw: Tuple[int, int], map_hw: Tuple[int, int],
                     cfg: Optional[DocXLayoutConfig] = None) -> List[Dict]:
    """One page's records behind pnms -- ``main_rows`` / ``sub_rows`` float32 [m, 12] in list order (8 head-map coordinates, score, 0-based
    class of the branch, two arg-max columns) -- -> the reference's unified list ``{"bbox": array([x0, y0, x2, y2]), "label", "score",
    "category_id"}`` in its reading order."""
    cfg = cfg or DocXLayoutConfig()
    inv = centernet_decode_affine(int(page_hw[0]), int(page_hw[1]), int(map_hw[0]), int(map_hw[1]))
    main = _to_page(np.asarray(main_rows, np.float32).reshape(-1, 12), inv)
    sub = _to_page(np.asarray(sub_rows, np.float32).reshape(-1, 12), inv)
    sub[:, 9] += np.float32(N_MAIN)
    dets = _per_class(main, cfg.num_classes, cfg.scores_thresh)
    dets_sub = _per_class(sub, cfg.num_classes, cfg.scores_thresh)
    for j in range(N_MAIN + 1, cfg.num_classes + 1):
        dets[j] = dets_sub[j]
    # merge_outputs: at most top_k rows over all classes, placeholders counted, ties at the cut all kept
    scores = np.hstack([dets[j][:, 8] for j in range(1, cfg.num_classes + 1)])
    if len(scores) > cfg.top_k:
        kth = len(scores) - cfg.top_k
        cut = np.partition(scores, kth)[kth]
        dets = {j: r[r[:, 8] >= cut] for j, r in dets.items()}
    # convert_eval_format: rounded vertices, two-decimal scores; classes ascending, list order inside a class
    layouts, subfields = [], []
    t = np.float32(cfg.scores_thresh)
    for j in range(1, cfg.num_classes + 1):
        for box in dets[j]:
            if box[8] < t:
                continue
            item = {"category": cfg.id2label[int(box[9])], "pts": np.round(box).tolist()[:8], "confidence": float("{:.2f}".format(box[8]))}
            (subfields if j > N_MAIN else layouts).append(item)
    ordered = _reading_order(layouts, subfields)
    return [{"bbox": np.array([it["pts"][0], it["pts"][1], it["pts"][4], it["pts"][5]]), "label": it["category"], "score": it["confidence"],
             "category_id": cfg.label2id[it["category"]]} for it in ordered]


def _reading_order(layouts: List[Dict], subfields: List[Dict]) -> List[Dict]:
    """wrap_result: regions are assigned to the sub-field that covers most of them (more than a tenth), sub-fields and the regions inside each
    are put in reading order, regions outside every sub-field take part in the order of the sub-fields as blocks of their own"""
    fields = [dict(f, layouts=[]) for f in subfields]
    sort_blocks(fields)
    loose = []
    for it in layouts:
        best, where = 0.0, -1
        for k, f in enumerate(fields):
            rate = quad_intersection_rate(it["pts"], f["pts"])
            if rate > best:
                best, where = rate, k
        (fields[where]["layouts"] if where >= 0 and best > 0.1 else loose).append(it)
    sort_blocks(loose)
    for f in fields:
        sort_blocks(f["layouts"])
    blocks = fields + [dict(it, layouts=[it]) for it in loose]
    sort_blocks(blocks)
    return [it for b in blocks for it in b["layouts"]]


class DocXLayoutStage(LayoutStage):
    """``LayoutStage``'s contract -- ``forward(pages, landing=None) -> (n, ticket)``, ``finish(n, ticket, org)``, ``__call__`` -- for DocXLayout, so that
    ``OcrTablePipeline.predict_stream()`` pipelines it like PicoDet.  forward(): per micro-batch of pages the warp (``pt_docx_preprocess``: the whole
    page is the crop) and the network (``pt_docx_forward_net``) into one set of head maps, then ONE ``pt_docx_decode`` launch for the batch; counts,
    records and keep flags (about 10 KB a page) land through the parent's alternating pinned buffers.  No host synchronisation of its own.

    ``device_order=True`` (off by default): forward() queues one ``pt_op_docx_order`` launch (csrc/docx_order.hip: docx_page_result on the device,
    a workgroup per page) behind the decode on the same stream and lands its (n_out, flag, rows) together with the three tensors above (about
    16 KB a page); finish() only builds the dicts from the rows.  A page the kernel flags (a list of 64 or more blocks in one of the sorts) goes
    through docx_page_result on its landed records as without the knob; ``last_fallback`` lists the pages of the last finish() that did.  Integers,
    labels and scores equal the host route's for an axis-aligned page with no condition; for turned quads the main angle's atan2 / sin / cos are
    the device library's (tests/docx_order_ref.py states the stability rule the tests use)."""

    def __init__(self, eng: HipEngine, config: Optional[DocXLayoutConfig] = None, micro_batch: Optional[int] = None, bgr: bool = True,
                 precision: Optional[int] = None, device_order: bool = False):
        self.device_order = bool(device_order)
        self.last_fallback: List[int] = []
        self.eng = eng
        self.precision = precision
        self.config = config or DocXLayoutConfig()
        if not 1 <= int(self.config.top_k) <= L.PT_DOCX_MAX_K:
            raise ValueError(f"DocXLayout: top_k={self.config.top_k} outside 1 .. {L.PT_DOCX_MAX_K}")
        self.micro_batch = int(micro_batch if micro_batch is not None else os.environ.get("PT_LAYOUT_MICROBATCH", "16"))
        self.bgr = bgr
        self.device_decode = False
        self._copy_stream = None
        self._pinned = [None, None]
        self._turn = 0

    def _tables(self, n: int, ph: int, pw: int) -> np.ndarray:
        inp_h, inp_w = self.config.resolution
        minv, _ = lore_geometry(ph, pw, inp_h, inp_w)      # c = (w / 2, h / 2), s = max(h, w): do_preprocess at scale 1
        tb = np.zeros(n, dtype=TSR_TABLE_DTYPE)
        tb["minv"], tb["page"], tb["crop_w"], tb["crop_h"] = minv.reshape(1, 6), np.arange(n), pw, ph
        return tb

    def forward(self, pages: torch.Tensor, landing=None):
        cfg = self.config
        n, ph, pw, _ = pages.shape
        inp_h, inp_w = cfg.resolution
        tb = self._tables(n, ph, pw)
        dev = pages.device
        heads = {k: torch.empty((n, inp_h // 4, inp_w // 4, 16 if k == "hm" else 8), dtype=torch.float32, device=dev) for k in HipEngine.DOCX_HEADS}
        with self.eng.precision_scope(self.precision):
            for i in range(0, n, self.micro_batch):
                x = self.eng.docx_preprocess(pages, tb[i:i + self.micro_batch], inp_h, inp_w, bgr=self.bgr, mean=DOCX_MEAN, std=DOCX_STD)
                self.eng.docx_forward_net(x, out={k: v[i:i + self.micro_batch] for k, v in heads.items()})
            counts, recs, _, keep = self.eng.docx_decode(heads, top_k=cfg.top_k, thr_lo=cfg.scores_thresh - 1e-3, ncls_main=N_MAIN,
                                                         ncls_sub=cfg.num_classes - N_MAIN, with_inds=False)
            if self.device_order:
                return self._land_tensors((counts, recs, keep) + self._order_launch(counts, recs, keep, (ph, pw)), landing)
        return self._land_tensors((counts, recs, keep), landing)

    def _order_launch(self, counts: torch.Tensor, recs: torch.Tensor, keep: torch.Tensor, page_hw):
        """one pt_op_docx_order launch on the current stream behind whatever wrote the records -> (n_out, flag, rows) on the device"""
        cfg = self.config
        inp_h, inp_w = cfg.resolution
        inv = centernet_decode_affine(int(page_hw[0]), int(page_hw[1]), inp_h // 4, inp_w // 4)
        return self.eng.op_docx_order(counts, recs, keep, inv, scores_thresh=cfg.scores_thresh, top_k=cfg.top_k, num_classes=cfg.num_classes,
                                      n_main=N_MAIN, use_nms=cfg.use_nms)

    def order_records(self, counts, recs, keep, page_hw) -> List[List[Dict]]:
        """the device half of ``device_order=True`` on given records (counts int32 [B,2], recs float32 [B,2,K,12], keep uint8 [B,2,K]; tensors or
        arrays) of pages of ``page_hw`` pixels: the launch, a blocking copy, the dict lists -- flagged pages through the host route, as finish()
        does (``last_fallback``).  For records that come from no network."""
        dev = self.eng._tdev
        c, r, k = (torch.as_tensor(np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v).to(dev).contiguous() for v in (counts, recs, keep))
        host = tuple(t.cpu() for t in (c, r, k) + self._order_launch(c, r, k, page_hw))
        return self._finish_ordered(c.shape[0], host, page_hw)

    def _page_host(self, counts, recs, keep, i: int, org) -> List[Dict]:
        """page i's landed records -> docx_page_result on the kept rows of both lists"""
        inp_h, inp_w = self.config.resolution
        rows = []
        for b in range(2):
            m = int(counts[i, b])
            r = recs[i, b, :m]
            rows.append(r[keep[i, b, :m] != 0] if self.config.use_nms else r)
        return docx_page_result(rows[0], rows[1], (int(org[0]), int(org[1])), (inp_h // 4, inp_w // 4), self.config)

    def _finish_ordered(self, n: int, host, org) -> List[List[Dict]]:
        """device_order=True: the landed (counts, recs, keep, n_out, flag, rows) -> the dict lists; only the two-decimal score is computed here"""
        cfg = self.config
        counts, recs, keep, n_out, flag, rows = (h[:n].numpy() for h in host)
        self.last_fallback = [i for i in range(n) if flag[i] != 0]
        out = []
        for i in range(n):
            if flag[i] != 0:
                out.append(self._page_host(counts, recs, keep, i, org))
                continue
            m = int(n_out[i])
            box = rows[i, :m, :4].astype(np.float64)
            page = []
            for k in range(m):
                label = cfg.id2label[int(rows[i, k, 5])]
                page.append({"bbox": box[k].copy(), "label": label, "score": float("{:.2f}".format(rows[i, k, 4])), "category_id": cfg.label2id[label]})
            out.append(page)
        return out

    def finish(self, n: int, ticket, org) -> List[List[Dict]]:
        """host half: wait for that forward()'s copy, then per page the kept rows of both lists -> docx_page_result"""
        done, host = ticket
        done.synchronize()
        if len(host) == 6:      # a forward() with device_order=True
            return self._finish_ordered(n, host, org)
        counts, recs, keep = (h[:n].numpy() for h in host)
        return [self._page_host(counts, recs, keep, i, org) for i in range(n)]

    def __call__(self, pages: torch.Tensor) -> List[List[Dict]]:
        n, ticket = self.forward(pages)
        return self.finish(n, ticket, tuple(pages.shape[1:3]))
