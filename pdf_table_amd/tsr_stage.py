"""Batched table-structure recognition stage (Lore): geometry and result shaping on the host, everything else on the GPU.

Replaces, for a batch of table crops of resident pages, the reference's per-table chain
``TableLorePreProcessor.process`` (lore/processer_lore.py:66-109) -> ``LoreModel.forward`` (lore/modeling_lore.py:125-194:
DLASeg detector, ``process_detect_output``, ``LoreProcessModel``) -> ``TableLorePostProcessor.__call__``
(processer_lore.py:163-188).  The host computes one 2x3 affine map per table (float64, like cv2.getAffineTransform)
and, after the device decode, maps the cell quads back to source pixels and rounds the logical locations.
"""
from __future__ import annotations

import os
import time

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from .streams import shared_stream

from . import lib as L
from .engine import TSR_TABLE_DTYPE, HipEngine
from .table_html import structure_html

__all__ = ["LoreConfig", "TsrStage", "lore_geometry", "affine_from_center_scale", "affine_upper_left", "invert_affine",
           "quad_inverse_map", "transform_quads", "process_logic_output"]


@dataclass
class LoreConfig:
    """The fields of lore/configuration_lore.py:29-116 that the inference path reads."""
    task_type: str = "wtw"
    model_name: str = "Lore"
    model_path: str = ""
    backbone: str = "DLA-34"
    resolution: Tuple[int, int] = (1024, 1024)
    stacking_layers: int = 4
    tsfm_layers: int = 4
    upper_left: bool = False
    wiz_2dpe: bool = False
    wiz_stacking: bool = True
    wiz_rev: bool = True
    vis_thresh: float = 0.2

    def __post_init__(self):
        if self.task_type == "wireless":                  # configuration_lore.py:66-78
            self.backbone, self.resolution = "ResNet-18", (768, 768)
            self.stacking_layers = self.tsfm_layers = 4
            self.upper_left, self.wiz_2dpe, self.wiz_rev, self.vis_thresh = True, True, False, 0.2
        elif self.task_type == "wtw":                     # configuration_lore.py:79-92
            self.backbone, self.resolution = "DLA-34", (1024, 1024)
            self.stacking_layers = self.tsfm_layers = 4
            self.upper_left, self.wiz_2dpe, self.wiz_rev, self.vis_thresh = False, False, True, 0.2
        else:                                             # "ptn" and anything else (:94-108)
            self.backbone, self.resolution = "DLA-34", (512, 512)
            self.stacking_layers = self.tsfm_layers = 3
            self.upper_left, self.wiz_2dpe, self.wiz_rev, self.vis_thresh = False, True, False, 0.35


def _affine_3pt(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """the 2x3 map through three point pairs (what cv2.getAffineTransform solves), float64"""
    a = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        a[2 * i, 0:3] = (src[i, 0], src[i, 1], 1.0)
        a[2 * i + 1, 3:6] = (src[i, 0], src[i, 1], 1.0)
        b[2 * i], b[2 * i + 1] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def affine_from_center_scale(center, scale, out_size, inv: bool = False) -> np.ndarray:
    """get_affine_transform(center, scale, 0, out_size, inv) of lineless_table_process.py:403-438 (rot = 0, no shift):
    three float32 anchor points on each side -- centre, centre + (0, -scale/2), and their perpendicular third."""
    s = np.float32(scale)
    dst_w, dst_h = out_size
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = center
    src[1] = np.asarray(center) + np.asarray([0.0, s * -0.5])
    dst[0] = (dst_w * 0.5, dst_h * 0.5)
    dst[1] = np.array([dst_w * 0.5, dst_h * 0.5], np.float32) + np.array([0, dst_w * -0.5], np.float32)
    for p in (src, dst):
        d = p[0] - p[1]
        p[2] = p[1] + np.array([-d[1], d[0]], np.float32)
    return _affine_3pt(dst, src) if inv else _affine_3pt(src, dst)


def affine_upper_left(center, scale, out_size, inv: bool = False) -> np.ndarray:
    """get_affine_transform_upper_left (lineless_table_process.py:441-468): the origin stays at the top-left corner;
    (cx, scale) -> (0, out_w) when cx >= cy, else (scale, cy) -> (out_w, 0); third point perpendicular."""
    s = np.float32(scale)
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = center
    if center[0] < center[1]:
        src[1] = (s, center[1])
        dst[1] = (out_size[0], 0)
    else:
        src[1] = (center[0], s)
        dst[1] = (0, out_size[0])
    for p in (src, dst):
        d = p[0] - p[1]
        p[2] = p[1] + np.array([-d[1], d[0]], np.float32)
    return _affine_3pt(dst, src) if inv else _affine_3pt(src, dst)


def invert_affine(m: np.ndarray) -> np.ndarray:
    """the inverse map cv2.warpAffine derives from M (float64, same operation order)"""
    m = np.asarray(m, np.float64).reshape(6).copy()
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0] = a11
    m[1] *= -d
    m[3] *= -d
    m[4] = a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m.reshape(2, 3)


def lore_geometry(crop_h: int, crop_w: int, inp_h: int, inp_w: int, upper_left: bool = False):
    """-> (minv 2x3 for pt_tsr_table, meta int64 [cx, cy, s, in_h, in_w, out_h, out_w]) -- processer_lore.py:74-126:
    c = (w/2, h/2) float32 (or (0, 0) with upper_left), s = max(h, w); meta is cast to int64 (fractions of c are
    dropped, as in the reference)."""
    s = max(crop_h, crop_w) * 1.0
    if upper_left:
        c = np.array([0, 0], dtype=np.float32)
        trans = affine_upper_left(c, s, (inp_w, inp_h))
    else:
        c = np.array([crop_w / 2.0, crop_h / 2.0], dtype=np.float32)
        trans = affine_from_center_scale(c, s, (inp_w, inp_h))
    meta = np.array([c[0], c[1], s, inp_h, inp_w, inp_h // 4, inp_w // 4]).astype(np.int64)
    return invert_affine(trans), meta


def quad_inverse_map(meta: np.ndarray, upper_left: bool = False) -> np.ndarray:
    """the float64 2x3 map transform_quads sends every vertex through (what pt_op_lore_match takes per table)"""
    return (affine_upper_left if upper_left else affine_from_center_scale)(meta[:2], meta[2], (meta[6], meta[5]), inv=True)


def transform_quads(quads: np.ndarray, meta: np.ndarray, upper_left: bool = False) -> np.ndarray:
    """ctdet_4ps_post_process[_upper_left] (lineless_table_process.py:489-533): the four vertices of every quad through
    the inverse map built from the int64 meta; float64 matrix x float32 point, stored back as float32."""
    t = quad_inverse_map(meta, upper_left)
    p = quads.astype(np.float32).astype(np.float64).reshape(-1, 4, 2)
    out = np.empty_like(p)
    out[..., 0] = t[0, 0] * p[..., 0] + t[0, 1] * p[..., 1] + t[0, 2]
    out[..., 1] = t[1, 0] * p[..., 0] + t[1, 1] * p[..., 1] + t[1, 2]
    return out.reshape(-1, 8).astype(np.float32)


def process_logic_output(logi: np.ndarray) -> np.ndarray:
    """lineless_table_process.py:658-663: fractional part > 0.5 rounds up, otherwise down."""
    fl = np.floor(logi)
    return np.where(logi - fl > 0.5, fl + 1, fl).astype(np.float32)


class TsrStage:
    def __init__(self, eng: HipEngine, config: Optional[LoreConfig] = None, micro_batch: int = 8, bgr: bool = True,
                 with_html: bool = True):
        self.eng = eng
        self.config = config or LoreConfig()
        self.micro_batch = micro_batch
        self.bgr = bgr
        self.with_html = with_html      # also emit 'structure_str_list' (show_results :292-303)
        self._copy_stream = None
        self.wait_s = 0.0
        self.fused_decode = os.environ.get("PT_TSR_FUSED", "1") != "0"     # pt_tsr_forward_decode vs the two-call path

    def tables(self, page_shape: Tuple[int, int], boxes_per_page: Sequence[np.ndarray]):
        """integer table boxes [k,4] (x1,y1,x2,y2) per page, cropped like crop_image_by_box
        (utils/ocr/ocr_common_utils.py:269-284: img[y1:y2, x1:x2]) -> (pt_tsr_table records, metas)."""
        ph, pw = page_shape
        inp_h, inp_w = self.config.resolution
        recs, metas = [], []
        for pi, boxes in enumerate(boxes_per_page):
            for b in np.asarray(boxes).reshape(-1, 4):
                x1, y1, x2, y2 = (int(v) for v in b)
                x1, y1 = max(x1, 0), max(y1, 0)
                x2, y2 = min(x2, pw), min(y2, ph)
                cw, ch = x2 - x1, y2 - y1
                if cw <= 0 or ch <= 0:
                    raise ValueError(f"empty table crop {b.tolist()} on a {ph}x{pw} page")
                minv, meta = lore_geometry(ch, cw, inp_h, inp_w, self.config.upper_left)
                r = np.zeros((), dtype=TSR_TABLE_DTYPE)
                r["minv"], r["page"], r["x0"], r["y0"], r["crop_w"], r["crop_h"] = minv.reshape(6), pi, x1, y1, cw, ch
                recs.append(r)
                metas.append(meta)
        return (np.array(recs, dtype=TSR_TABLE_DTYPE) if recs else np.zeros(0, dtype=TSR_TABLE_DTYPE)), metas

    def start(self, pages: torch.Tensor, tables: np.ndarray):
        """device half 1, nothing synchronises: per micro-batch warp -> DLA-34+DCN -> decode; returns the pending state"""
        cfg = self.config
        inp_h, inp_w = cfg.resolution
        pending = []
        # balanced micro-batches (87 tables at micro_batch 80 -> 44 + 43, not 80 + 7: a 7-table launch leaves most CUs idle)
        nmb = max(1, -(-len(tables) // self.micro_batch))
        size = -(-len(tables) // nmb) if len(tables) else 1
        fused = cfg.backbone != "ResNet-18" and self.fused_decode
        if fused and nmb > 1:
            # all micro-batches decode into slices of one allocation, so that the processor (a chain of ~60 small launches)
            # runs ONCE over all tables of the call instead of once per micro-batch
            nt = len(tables)
            dev = pages.device
            counts_all = torch.zeros((nt,), dtype=torch.int32, device=dev)
            dets_all = torch.empty((nt, L.PT_TSR_MAX_CELLS, 9), dtype=torch.float32, device=dev)
            logi_all = torch.empty((nt, L.PT_TSR_MAX_CELLS, 256), dtype=torch.float32, device=dev)
        for i in range(0, len(tables), size):
            tb = tables[i:i + size]
            out = (counts_all[i:i + len(tb)], dets_all[i:i + len(tb)], logi_all[i:i + len(tb)]) if fused and nmb > 1 else None
            if fused and os.environ.get("PT_TSR_BANDS", "1") != "0":
                # warp + net + decode in one call with the tables known to the library: the detector's front segment skips the letterbox rows of
                # crops wider than high (PT_TSR_BANDS=0, read per call: the two calls below, A/B switch)
                counts, dets, logi = self.eng.tsr_warp_forward_decode(pages, tb, inp_h, inp_w, bgr=self.bgr, wiz_rev=cfg.wiz_rev,
                                                                      vis_thresh=cfg.vis_thresh, sync=False, out=out)
                pending.append((i, len(tb), counts, dets, logi))
                continue
            x = self.eng.tsr_preprocess(pages, tb, inp_h, inp_w, bgr=self.bgr)
            if fused:      # one call, ax / cr heads only where the decode reads them
                counts, dets, logi = self.eng.tsr_forward_decode(x, wiz_rev=cfg.wiz_rev, vis_thresh=cfg.vis_thresh, sync=False, out=out)
            else:
                heads = self.eng.tsr_forward_net(x, wireless=cfg.backbone == "ResNet-18")
                counts, dets, logi = self.eng.tsr_decode(heads, wiz_rev=cfg.wiz_rev, vis_thresh=cfg.vis_thresh, sync=False)
            pending.append((i, len(tb), counts, dets, logi))
        if fused and nmb > 1:
            pending = [(0, len(tables), counts_all, dets_all, logi_all)]
        # the cell counts go to pinned host memory right behind the decode, with an event of their own: process() then waits
        # for THESE tables' decode only -- a `.cpu()` there would wait for everything queued on the stream since (a pipelined
        # caller has queued the next batch by then)
        out = []
        for (i, nt, counts, dets, logi) in pending:
            host = torch.empty(counts.shape, dtype=counts.dtype, pin_memory=True)
            host.copy_(counts, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            out.append((i, nt, counts, dets, logi, host, ev))
        return out

    def match_input(self, tables: np.ndarray, metas: List[np.ndarray], boxes_per_page: Sequence[np.ndarray],
                    text_boxes: Sequence[np.ndarray]) -> Dict:
        """What process(match=...) needs to assign text lines to cells on the device (pt_op_lore_match): per table its candidate lines -- the
        page's lines whose centre lies in the layout box the crop was cut from, grown by 2 (texts_in_table: what page_table_html chooses) --
        with their float32 boxes, the inverse map transform_quads builds and the crop's corner.  ``tables`` / ``metas``: tables()'s;
        ``boxes_per_page``: what tables() was given; ``text_boxes``: per page [t, 4] = (min x, min y, max x, max y) in page pixels
        (table_text_match.text_boxes).  Host arithmetic only."""
        from .table_text_match import texts_in_table
        flat = [b for boxes in boxes_per_page for b in np.asarray(boxes).reshape(-1, 4)]
        if len(flat) != len(tables):
            raise ValueError(f"match_input: {len(flat)} table boxes for {len(tables)} table records")
        per_page: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}
        lines, boxes = [], []
        for r, box in zip(tables, flat):
            pi = int(r["page"])
            if pi not in per_page:
                tb64 = np.asarray(text_boxes[pi], np.float64).reshape(-1, 4)
                tb32 = tb64.astype(np.float32)
                if not np.array_equal(tb32.astype(np.float64), tb64):
                    raise ValueError("match_input: the text boxes must be exact in float32 (the device matches float32 boxes widened to double)")
                per_page[pi] = (np.asarray(text_boxes[pi]).reshape(-1, 4), tb32)
            tbx, tb32 = per_page[pi]
            inside = texts_in_table([float(v) for v in box], tbx, diff=2) if len(tbx) else np.zeros(0, np.int64)
            lines.append(inside)
            boxes.append(tb32[inside])
        affine = np.stack([quad_inverse_map(m, self.config.upper_left).reshape(6) for m in metas]) if len(metas) else np.zeros((0, 6))
        offset = np.stack([tables["x0"], tables["y0"]], 1).astype(np.float64)
        return {"lines": lines, "boxes": boxes, "affine": np.ascontiguousarray(affine, np.float64), "offset": offset}

    def _queue_match(self, match: Dict, i: int, nt: int, counts_d, dets, axes):
        """one pinned non-blocking upload (maps, corners, line boxes, per-table line offsets) and one pt_op_lore_match launch on the current stream for
        tables i .. i + nt - 1 -> (candidate lines per table, int32 [lines] on the device or None without lines, what must stay alive)"""
        lines_of = match["lines"][i:i + nt]
        offs = np.zeros(nt + 1, np.int32)
        offs[1:] = np.cumsum([len(c) for c in lines_of])
        m = int(offs[-1])
        if m == 0:
            return lines_of, None, None
        boxes = np.concatenate(match["boxes"][i:i + nt]).astype(np.float32).reshape(-1)
        geom = np.concatenate([match["affine"][i:i + nt].reshape(-1), match["offset"][i:i + nt].reshape(-1)])
        # float64 first, then the 16-byte boxes (nt * 64 bytes in), then the int32 offsets: every view below is aligned
        buf = np.concatenate([geom.view(np.uint8), boxes.view(np.uint8), offs.view(np.uint8)])
        up = torch.from_numpy(buf).pin_memory().to(self.eng._tdev, non_blocking=True)
        a, b, c = nt * 48, nt * 64, nt * 64 + 16 * m
        out = self.eng.op_lore_match(dets, axes, counts_d, up[:a].view(torch.float64).reshape(nt, 6), up[a:b].view(torch.float64).reshape(nt, 2),
                                     up[b:c].view(torch.float32).reshape(m, 4), up[c:].view(torch.int32))
        return lines_of, out, up

    def process(self, pending, match: Optional[Dict] = None):
        """device half 2: cell counts from their pinned copy (waits for half 1 of these tables only when it is still running), the
        processor over all cells of each micro-batch, then the valid rows to pinned host memory on a copy stream behind
        an event -- nothing here waits for work queued after start().  ``match`` (match_input()): behind the processor of every entry one
        pt_op_lore_match launch assigns the tables' candidate lines to cells; its [lines] int32 rides on the same copy back and collect()
        attaches it.  Without it: no new launch, copy or key."""
        cfg = self.config
        staged = []
        for (i, nt, counts_d, dets, logi, counts_h, counts_ev) in pending:
            t0 = time.perf_counter()
            counts_ev.synchronize()
            self.wait_s += time.perf_counter() - t0      # host seconds spent waiting for the decode (diagnostics: pipeline.metric)
            counts = counts_h.numpy().copy()
            logic, stacked = self.eng.tsr_process(logi, dets, counts, use_2dpe=cfg.wiz_2dpe)
            mt = self._queue_match(match, i, nt, counts_d, dets, stacked if cfg.wiz_stacking else logic) if match is not None else None
            staged.append((i, nt, counts, dets, logic, stacked, mt))
        if not staged:
            return [], None
        if self._copy_stream is None:
            self._copy_stream = shared_stream(staged[0][3].device, "tsr_copy")
        ready = torch.cuda.Event()
        ready.record()
        host = []
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(ready)
            for (i, nt, counts, dets, logic, stacked, mt) in staged:
                nmax = max(1, int(counts.max()) if len(counts) else 1)
                bufs = []
                for src in (dets, logic, stacked):
                    dst = torch.empty((src.shape[0], nmax, src.shape[2]), dtype=torch.float32, pin_memory=True)
                    dst.copy_(src[:, :nmax], non_blocking=True)
                    src.record_stream(self._copy_stream)
                    bufs.append(dst)
                if mt is None:
                    host.append((i, nt, counts, bufs))
                    continue
                lines_of, rows_d, up = mt
                rows_h = None
                if rows_d is not None:
                    rows_h = torch.empty(rows_d.shape, dtype=torch.int32, pin_memory=True)
                    rows_h.copy_(rows_d, non_blocking=True)
                    rows_d.record_stream(self._copy_stream)
                host.append((i, nt, counts, bufs, (lines_of, rows_h, up)))      # up: alive until collect() has seen the copy
            done = torch.cuda.Event()
            done.record(self._copy_stream)
        return host, done

    def collect(self, processed, metas: List[np.ndarray], offsets: Optional[np.ndarray] = None) -> List[Dict]:
        """host half: quads back to source pixels, logical rounding -> per table {'polygons' f32 [n,8], 'logi' f32 [n,4]
        (integer valued), 'logic_axis', 'stacked_axis' (unrounded), 'scores'} like TableLorePostProcessor's result dict.
        ``offsets`` int [tables, 2]: the crop's (x0, y0) on its page, added to every vertex so that the quads are in page
        pixels -- what the reference's system path does after the per-crop call (convert_table_sep_to_merge ->
        box_list_move_point, pdf_table/table_common.py:1811-1825); None keeps them relative to the crop (the task's own
        result, processer_lore.py:175-182)."""
        cfg = self.config
        host, done = processed
        if done is not None:
            done.synchronize()
        out: List[Dict] = []
        for ent in host:
            i, nt, counts, bufs = ent[:4]
            dets_h, logic_h, stacked_h = (b.numpy() for b in bufs)
            # process(match=...): per table its candidate lines (page indices) and, per line, the input row of its cell
            lines_of, rows_h = ent[4][:2] if len(ent) > 4 else (None, None)
            rows = rows_h.numpy() if rows_h is not None else np.zeros(0, np.int32)
            m0 = 0
            for k in range(nt):
                n = int(counts[k])
                if lines_of is not None:
                    mk = len(lines_of[k])
                    matched = {"matched_lines": np.asarray(lines_of[k], np.int64) if n else np.zeros(0, np.int64),
                               "matched": rows[m0:m0 + mk].astype(np.int64) if n else np.zeros(0, np.int64)}
                    m0 += mk
                if n == 0:       # LoreModel.forward's empty case (modeling_lore.py:171-173)
                    out.append({"polygons": np.zeros((1, 8), np.float32), "logi": np.zeros((1, 4), np.float32),
                                "logic_axis": np.zeros((1, 4), np.float32), "stacked_axis": np.zeros((1, 4), np.float32),
                                "scores": np.zeros((0,), np.float32)})
                    if lines_of is not None:
                        out[-1].update(matched)
                    continue
                final = stacked_h[k, :n] if cfg.wiz_stacking else logic_h[k, :n]
                polys = transform_quads(dets_h[k, :n, :8], metas[i + k], cfg.upper_left)
                if offsets is not None:
                    # box_list_move_point works on .tolist() values: python floats + the rounded int corner -> float64
                    polys = polys.astype(np.float64) + np.tile(np.asarray(offsets[i + k], np.float64), 4)[None]
                r = {"polygons": polys,
                     "logi": process_logic_output(final), "logic_axis": logic_h[k, :n].copy(),
                     "stacked_axis": stacked_h[k, :n].copy(), "scores": dets_h[k, :n, 8].copy()}
                if self.with_html:       # table_html.table_cells_from_logits(polygons, logi) gives the cell objects on demand
                    r["structure_str_list"] = [structure_html(r["polygons"], r["logi"])]
                if lines_of is not None:
                    r.update(matched)
                out.append(r)
        return out

    def finish(self, pending, metas: List[np.ndarray], offsets: Optional[np.ndarray] = None, match: Optional[Dict] = None) -> List[Dict]:
        return self.collect(self.process(pending, match) if match is not None else self.process(pending), metas, offsets)

    def run(self, pages: torch.Tensor, tables: np.ndarray, metas: List[np.ndarray], offsets: Optional[np.ndarray] = None,
            match: Optional[Dict] = None) -> List[Dict]:
        return self.finish(self.start(pages, tables), metas, offsets, match)

    def regroup(self, flat: List[Dict], boxes_per_page: Sequence[np.ndarray]) -> List[List[Dict]]:
        res, o = [], 0
        for b in boxes_per_page:
            k = len(np.asarray(b).reshape(-1, 4))
            res.append(flat[o:o + k])
            o += k
        return res

    def __call__(self, pages: torch.Tensor, boxes_per_page: Sequence[np.ndarray], page_frame: bool = False,
                 text_boxes: Optional[Sequence[np.ndarray]] = None) -> List[List[Dict]]:
        """page_frame=True: quads in page pixels (the crop's clamped x0, y0 added), like the reference's merged result.  text_boxes (per page
        [t, 4], table_text_match.text_boxes; needs page_frame=True): every table's candidate lines are assigned to its cells on the device ->
        'matched_lines' / 'matched' in every table (process(match=...))"""
        if text_boxes is not None and not page_frame:
            raise ValueError("TsrStage: text lines are matched in page pixels: text_boxes needs page_frame=True")
        tables, metas = self.tables(tuple(pages.shape[1:3]), boxes_per_page)
        offs = np.stack([tables["x0"], tables["y0"]], 1).astype(np.float32) if page_frame and len(tables) else None
        match = self.match_input(tables, metas, boxes_per_page, text_boxes) if text_boxes is not None and len(tables) else None
        flat = self.run(pages, tables, metas, offs, match) if len(tables) else []
        return self.regroup(flat, boxes_per_page)
