"""Batched layout-detection stage (PicoDet): pre-process + network + candidate compaction on the GPU, the per-class hard
NMS on the host over the few candidates that can pass the score threshold.

Replaces the reference's per-page chain ``OCRPicodetPreProcessor.__call__`` -> ONNX run -> ``OCRPicodetPostProcessor.__call__``
(picodet/processor_picodet.py:72-113, 184-298; ocr_layout_task.py:70-157).  The device hands back, per page, only the
anchors whose best class score exceeds a threshold just below ``score_threshold`` (the reference's post-processor drops
everything else in ``probs > self.score_threshold``, :252); their box distributions are decoded here with the
reference's numpy arithmetic (float32 soft-max, float64 boxes), so the result equals the oracle's on the same head values.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Dict, List, Sequence

import numpy as np
import torch
from .streams import shared_stream

from . import lib as L
from .engine import HipEngine

__all__ = ["PicodetConfig", "LayoutStage", "OnnxLayoutStage", "hard_nms", "layout_tables", "LAYOUT_LABELS"]

LAYOUT_LABELS = {   # configuration_picodet.py:66-104
    "ch": ["text", "title", "figure", "figure_caption", "table", "table_caption", "header", "footer", "reference", "equation"],
    "en": ["text", "title", "list", "table", "figure"],
    "table": ["table"],
}


@dataclass
class PicodetConfig:
    """configuration_picodet.py:41-113 (inference fields)"""
    task_type: str = "en"
    model_name: str = "picodet"
    model_path: str = ""
    backbone: str = "LCNet"
    img_height: int = 800
    img_width: int = 608
    score_threshold: float = 0.5
    nms_threshold: float = 0.5
    strides: Sequence[int] = (8, 16, 32, 64)
    nms_top_k: int = 1000
    keep_top_k: int = 100
    labels: List[str] = field(default_factory=list)

    def __post_init__(self):
        self.labels = list(LAYOUT_LABELS.get(self.task_type, LAYOUT_LABELS["ch"]))
        self.id2label = dict(enumerate(self.labels))


def _iou_of(b0, b1, eps=1e-5):
    lt = np.maximum(b0[..., :2], b1[..., :2])
    rb = np.minimum(b0[..., 2:], b1[..., 2:])
    hw = np.clip(rb - lt, 0.0, None)
    inter = hw[..., 0] * hw[..., 1]
    a0 = np.clip(b0[..., 2:] - b0[..., :2], 0.0, None)
    a1 = np.clip(b1[..., 2:] - b1[..., :2], 0.0, None)
    return inter / (a0[..., 0] * a0[..., 1] + a1[..., 0] * a1[..., 1] - inter + eps)


def hard_nms(box_scores: np.ndarray, iou_threshold: float, top_k: int = -1, candidate_size: int = 200) -> np.ndarray:
    """processor_picodet.py:301-330: greedy NMS over the candidate_size best boxes, at most top_k kept"""
    scores, boxes = box_scores[:, -1], box_scores[:, :-1]
    picked = []
    idx = np.argsort(scores)[-candidate_size:]
    while len(idx) > 0:
        cur = idx[-1]
        picked.append(cur)
        if 0 < top_k == len(picked) or len(idx) == 1:
            break
        idx = idx[:-1]
        idx = idx[_iou_of(boxes[idx, :], boxes[cur:cur + 1, :]) <= iou_threshold]
    return box_scores[picked, :]


def _softmax_f32(x: np.ndarray) -> np.ndarray:
    """scipy.special.softmax(x, axis=1) on float32 input: exp(x - max) / sum, in float32"""
    e = np.exp(x - np.max(x, axis=1, keepdims=True))
    return e / np.sum(e, axis=1, keepdims=True)


def layout_tables(layout_result: List[Dict], label: str = "table", score_threshold: float = 0.2) -> List[Dict]:
    """TableProcessUtils.get_layout_by_type (pdf_table/table_common.py:1287-1300): regions of one label, top to bottom"""
    res = [it for it in layout_result if it["label"].lower() == label.lower() and it["score"] >= score_threshold]
    res.sort(key=lambda x: x["bbox"][1])
    return res


class LayoutStage:
    CANDIDATE_SIZE = 200      # hard_nms's candidate_size (processor_picodet.py:301), the [-200:] of decode_page

    def __init__(self, eng: HipEngine, config: PicodetConfig = None, max_cands: int = 2048, precision: Optional[int] = None,
                 device_decode: bool = False):
        """``device_decode=True``: forward() queues pt_op_layout_decode (csrc/layout_decode.hip) behind the candidate compaction on the same stream
        and lands (counts, detection counts, detections [n, ncls * min(keep_top_k, 200), 6] float64) instead of the records; finish() only
        checks the counts and builds the dict lists.  Equal scores are ordered by (level, anchor) there -- decode_page's arg-sorts have no tie
        rule -- and exp is the device's, so boxes and scores agree with decode_page to float32 rounding, not bit for bit.  Off by default.

        ``precision``: an L.PT_PRECISION_* for THIS stage's network, whatever the engine's is (None: the engine's).  The layout net is the
        pipeline's smallest (3 % of a step) and its output is a DECISION the table stage inherits -- the crop of every table at the box's ROUNDED
        coordinates (ocr_system_task.py:184-198): in a 16-bit mode an edge that rounds one pixel differently is a different input to the table
        net.  ``precision=L.PT_PRECISION_BF16X3`` runs just this stage in the pair mode (its blob must then be a bf16 blob with the pair tiles,
        also on an engine that otherwise computes in PT_PRECISION_F16: blobs carry their format per model)."""
        self.eng = eng
        self.precision = precision
        self.config = config or PicodetConfig()
        self.max_cands = max_cands
        self._copy_stream = None
        self._pinned = [None, None]          # two host landing buffers: a forward() may be queued while the previous finish() still reads
        self._turn = 0
        self.device_decode = bool(device_decode)

    PROBS = False      # the in-tree head hands back class LOGITS

    def _max_dets(self) -> int:
        cfg = self.config
        return len(cfg.labels) * (min(int(cfg.keep_top_k), self.CANDIDATE_SIZE) if cfg.keep_top_k > 0 else self.CANDIDATE_SIZE)

    def _decode_on_device(self, counts: torch.Tensor, cands: torch.Tensor, org, landing=None):
        """device_decode=True: one pt_op_layout_decode launch on the current stream behind the kernels that wrote counts / cands, then the copy of
        (counts, detection counts, detections) instead of the records"""
        cfg = self.config
        ndet, dets = self.eng.op_layout_decode(counts, cands, len(cfg.labels), cfg.strides, cfg.img_height, cfg.img_width, int(org[0]), int(org[1]),
                                               probs=self.PROBS, score_threshold=cfg.score_threshold, nms_threshold=cfg.nms_threshold,
                                               nms_top_k=cfg.nms_top_k, candidate_size=self.CANDIDATE_SIZE, keep_top_k=cfg.keep_top_k,
                                               max_dets=self._max_dets())
        return self._land_tensors((counts, ndet, dets), landing)

    def forward(self, pages: torch.Tensor, landing=None):
        """device half (asynchronous): network + candidate compaction on the current stream, then the D2H of the
        records on a copy stream behind an event -- finish() waits for that copy only, not for whatever else has
        been queued on the compute stream meanwhile.  ``landing``: a key of its own host landing buffer, outside the two
        that alternate (predict_stream's second layout pass over pages rotated by the orientation vote)"""
        cfg = self.config
        # the stage's precision is host state read when a call is QUEUED: the launches below carry it, later calls do not; the scope holds the
        # engine's lock, so no other host thread can queue a call in this stage's precision meanwhile
        with self.eng.precision_scope(self.precision):
            counts, cands = self.eng.layout_forward(pages, cfg.img_height, cfg.img_width, len(cfg.labels),
                                                    thr_lo=cfg.score_threshold - 1e-3, max_cands=self.max_cands)
        if getattr(self, "device_decode", False):
            return self._decode_on_device(counts, cands, pages.shape[1:3], landing)
        return self._land(counts, cands, landing)

    def _land(self, counts: torch.Tensor, cands: torch.Tensor, landing=None):
        """counts / records written on the current stream -> their copy into a pinned landing buffer on the copy stream behind an event: (n, ticket)"""
        return self._land_tensors((counts, cands), landing)

    def _land_tensors(self, dev, landing=None):
        """device tensors [n, ...] written on the current stream (a stage always lands the same kinds) -> pinned copies, as _land()"""
        counts = dev[0]
        n = counts.shape[0]
        if self._copy_stream is None:
            self._copy_stream = shared_stream(counts.device, "layout_copy")
        if landing is None:
            slot = self._turn
            self._turn ^= 1
            pinned = self._pinned
        else:
            slot = landing
            pinned = self.__dict__.setdefault("_pinned_extra", {})
        host = pinned.get(slot) if isinstance(pinned, dict) else pinned[slot]
        if host is None or host[0].shape[0] < n or len(host) != len(dev):
            host = tuple(torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype).pin_memory() for t in dev)
            pinned[slot] = host
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(ready)
            for h, t in zip(host, dev):
                h[:n].copy_(t, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._copy_stream)
        for t in dev:
            t.record_stream(self._copy_stream)
        return n, (done, host)

    def decode_outputs(self, scores: Sequence[np.ndarray], dists: Sequence[np.ndarray], org_shape) -> List[Dict]:
        """One page's outputs of a PicoDet ONNX export -- per level class PROBABILITIES [A_l, ncls] and box-distribution logits [A_l, 32], the
        two halves ``OcrLayoutTask.get_onnx_output_dict`` splits (ocr_layout_task.py:159-175) -- -> the same result list: anchors that can pass
        the score threshold become the candidate records decode_page() reads from the engine's own graph"""
        cfg = self.config
        ncls = len(cfg.labels)
        recs = []
        for l, (sc, bd) in enumerate(zip(scores, dists)):
            sc, bd = np.asarray(sc, np.float32).reshape(-1, ncls), np.asarray(bd, np.float32).reshape(-1, 32)
            keep = np.nonzero(sc.max(1) > cfg.score_threshold - 1e-3)[0]
            r = np.zeros((len(keep), 2 + ncls + 32), np.float32)
            r[:, 0] = np.full(len(keep), l, np.int32).view(np.float32)
            r[:, 1] = keep.astype(np.int32).view(np.float32)
            r[:, 2:2 + ncls], r[:, 2 + ncls:] = sc[keep], bd[keep]
            recs.append(r)
        return self.decode_page(np.concatenate(recs, 0) if recs else np.zeros((0, 2 + ncls + 32), np.float32), org_shape, probs=True)

    def decode_page(self, rec: np.ndarray, org_shape, probs: bool = False) -> List[Dict]:
        """candidate records [k, 48] of one page -> the `bboxs` list of OCRPicodetPostProcessor.__call__ (probs: the class columns already
        went through the sigmoid, as in an ONNX export's outputs)"""
        cfg = self.config
        ncls = len(cfg.labels)
        if len(rec) == 0:
            return []
        # the device appends candidates with an atomic counter: put them in the reference's dense order (level, anchor) so that
        # ties in the argsorts below break as they do there and the result does not depend on the order of arrival
        rec = rec[np.lexsort((rec[:, 1].view(np.int32), rec[:, 0].view(np.int32)))]
        level = rec[:, 0].view(np.int32)
        anchor = rec[:, 1].view(np.int32)
        logits = rec[:, 2:2 + ncls]
        scores = np.ascontiguousarray(logits, dtype=np.float32) if probs else \
            torch.sigmoid(torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32))).numpy()   # F.sigmoid of forward_eval
        reg = rec[:, 2 + ncls:2 + ncls + 32].astype(np.float32)
        reg_max = 7
        th, tw = cfg.img_height, cfg.img_width
        boxes_l, scores_l = [], []
        for l, stride in enumerate(cfg.strides):
            m = level == l
            if not m.any():
                continue
            a, sc, bd = anchor[m], scores[m], reg[m]
            fm_w = int(np.arange(tw / stride).shape[0])                      # np.arange(fm_w) of a float count (:213-215)
            ct_row = (a // fm_w + 0.5) * stride
            ct_col = (a % fm_w + 0.5) * stride
            center = np.stack((ct_col, ct_row, ct_col, ct_row), axis=1)
            dist = _softmax_f32(bd.reshape(-1, reg_max + 1)) * np.expand_dims(np.arange(reg_max + 1), 0)
            dist = np.sum(dist, axis=1).reshape(-1, 4) * stride
            order = np.argsort(sc.max(axis=1))[::-1][:cfg.nms_top_k]         # the level's top-K rule (:225-229)
            boxes_l.append(center[order] + [-1, -1, 1, 1] * dist[order])
            scores_l.append(sc[order])
        bboxes = np.concatenate(boxes_l, 0)
        conf = np.concatenate(scores_l, 0)
        # per-class greedy NMS: candidate order by numpy (its tie order), the greedy loop on the host in C++ (pt_hard_nms)
        groups, orders, labels_c = [], [], []
        base = 0
        for c in range(ncls):
            probs = conf[:, c]
            mask = probs > cfg.score_threshold
            if not mask.any():
                continue
            bs = np.concatenate([bboxes[mask], probs[mask].reshape(-1, 1)], axis=1)
            groups.append(bs)
            orders.append(np.argsort(bs[:, -1])[-200:] + base)
            labels_c.append(c)
            base += len(bs)
        picked, labels = [], []
        if groups:
            allb = np.ascontiguousarray(np.concatenate(groups, 0), dtype=np.float64)
            order = np.ascontiguousarray(np.concatenate(orders), dtype=np.int64)
            goff = np.zeros(len(groups) + 1, np.int64)
            goff[1:] = np.cumsum([len(o) for o in orders])
            out = np.empty(len(order), np.int64)
            npk = np.zeros(len(groups), np.int32)
            L.check(L.load().pt_hard_nms(allb.ctypes.data, order.ctypes.data, goff.ctypes.data, len(groups),
                                             float(cfg.nms_threshold), int(cfg.keep_top_k), out.ctypes.data, npk.ctypes.data),
                    "pt_hard_nms")
            for g, c in enumerate(labels_c):
                sel = out[goff[g]:goff[g] + npk[g]]
                picked.append(allb[sel])
                labels.extend([c] * len(sel))
        if not picked:
            return []
        pb = np.concatenate(picked)
        oh, ow = np.float32(org_shape[0]), np.float32(org_shape[1])
        b = pb[:, :4]
        x = b[:, [0, 2, 0, 2]]
        y = b[:, [1, 3, 3, 1]]
        xy = np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], 1)
        xy[:, [0, 2]] = xy[:, [0, 2]].clip(0, ow)        # warp_boxes clips to the ORIGINAL size in the resized frame (:158-159)
        xy[:, [1, 3]] = xy[:, [1, 3]].clip(0, oh)
        pb[:, :4] = xy.astype(np.float32)
        sf = np.array([float(th) / org_shape[0], float(tw) / org_shape[1]], dtype=np.float32)
        pb[:, :4] /= np.concatenate([sf[::-1], sf[::-1]])
        return [{"bbox": pb[i, :4].copy(), "label": cfg.id2label[int(c)], "score": pb[i, 4], "category_id": int(c)}
                for i, c in enumerate(labels)]

    def __call__(self, pages: torch.Tensor) -> List[List[Dict]]:
        n, ticket = self.forward(pages)
        return self.finish(n, ticket, tuple(pages.shape[1:3]))

    def finish(self, n: int, ticket, org) -> List[List[Dict]]:
        """host half: wait for the candidate copy of that forward(), decode + NMS per page.  At most one newer forward() may
        have been issued in between (two landing buffers)."""
        done, host = ticket
        done.synchronize()
        counts = host[0][:n].numpy().copy()
        if (counts > self.max_cands).any():
            raise RuntimeError(f"layout: {int(counts.max())} candidate anchors on a page exceed max_cands={self.max_cands}")
        if getattr(self, "device_decode", False):
            return self._finish_decoded(n, host)
        kmax = int(counts.max()) if len(counts) else 0
        rec = host[1][:n, :max(kmax, 1)].numpy()
        return [self._decode_record_page(rec[i, :counts[i]], org) for i in range(len(counts))]

    def _finish_decoded(self, n: int, host) -> List[List[Dict]]:
        """device_decode=True: the landed (counts, detection counts, detections) -> the dict lists; nothing is computed here"""
        cfg = self.config
        ndet = host[1][:n].numpy().copy()
        if (ndet > host[2].shape[1]).any():
            raise RuntimeError(f"layout: {int(ndet.max())} detections on a page exceed max_dets={host[2].shape[1]}")
        dets = host[2][:n].numpy()
        return [[{"bbox": dets[i, k, :4].copy(), "label": cfg.id2label[int(dets[i, k, 5])], "score": dets[i, k, 4], "category_id": int(dets[i, k, 5])}
                 for k in range(int(ndet[i]))] for i in range(n)]

    def _decode_record_page(self, rec: np.ndarray, org) -> List[Dict]:
        """one page's landed records -> its result list (the in-tree head hands back class LOGITS)"""
        return self.decode_page(rec, org)


class OnnxLayoutStage(LayoutStage):
    """A LayoutStage whose device half is a PicoDet ONNX export walked by ``HipGraphExecutor`` (the reference's layout stage is ONNX-only,
    ocr_layout_task.py:82-123): same contract -- ``forward(pages, landing=None) -> (n, ticket)``, ``finish(n, ticket, org)``, ``__call__`` -- so
    ``OcrTablePipeline.predict_stream()`` pipelines it like the in-tree net.  forward(): the engine's pre-processing kernel, the layer walk
    replayed from the executor's captured HIP graph, ONE pt_op_pico_candidates launch on the graph's 2 L output activations right behind the
    replay on the same stream (they are the graph's own buffers: stream order is what protects them from the next replay), then the parent's
    copy of counts and records into the alternating pinned landing buffers.  No host synchronisation of its own.  finish(): the parent's decode
    with ``probs=True`` (an export's class rows went through the Sigmoid already).  The kernel converts and copies only, so the results equal
    ``detect_host()`` -- every anchor copied to the host, filtered by numpy -- bit for bit.

    The graph's outputs are checked from their host-known shapes once per input shape (2 L token-row outputs, ncls and 32 real channels; the
    texts of ``UnsupportedOnnxGraph`` are those the synchronous route raised).  A graph whose outputs are not 16-bit activations, or that has
    more levels or classes than a candidate record holds, is served by ``detect_host()`` inside forward(): slower, never refused."""

    MAX_LEVELS = 4
    MAX_CLASSES = L.PT_LAYOUT_CAND_FLOATS - 2 - 32

    PROBS = True      # an export's class rows went through the Sigmoid already

    def __init__(self, eng: HipEngine, executor, config: PicodetConfig = None, max_cands: int = 2048, device_decode: bool = False):
        # the executor computes in the engine's arithmetic; device_decode as in LayoutStage (the host fallback for outputs the tail cannot read is unchanged)
        super().__init__(eng, config, max_cands=max_cands, precision=None, device_decode=device_decode)
        self.exec = executor
        self._tail_ok: Dict[tuple, bool] = {}       # pre-processed input shape -> True: device tail, False: host route

    def _graph_outputs(self, pages: torch.Tensor):
        cfg = self.config
        x = self.eng.layout_preprocess(pages, cfg.img_height, cfg.img_width)
        return x, self.exec.run_device_graphed(x, 3)      # the layer walk replayed from a captured HIP graph per batch shape

    def _check_outputs(self, acts) -> bool:
        """the shape check of the synchronous route, from what the host knows of the activations -> True when the device tail can read them"""
        from .onnx_import import UnsupportedOnnxGraph
        cfg = self.config
        ncls = len(cfg.labels)
        for a in acts:
            if not getattr(a, "seq", False):
                raise UnsupportedOnnxGraph(f"layout graph output of shape {a.shape()}: [B, anchors, channels] tensors are expected")
        half = len(acts) // 2
        if len(acts) % 2 or not acts:
            raise UnsupportedOnnxGraph(f"a PicoDet export returns 2 L tensors (L score maps, then L box distributions), this graph returns {len(acts)}")
        if any(a.c != ncls for a in acts[:half]) or any(a.c != 32 for a in acts[half:2 * half]):
            raise UnsupportedOnnxGraph(f"layout graph outputs {[tuple(a.shape()) for a in acts]}: {ncls} class scores and 32 distribution bins per anchor "
                                       f"are expected for task_type '{cfg.task_type}'")
        if any(s_.shape()[:2] != d_.shape()[:2] for s_, d_ in zip(acts[:half], acts[half:])):
            return False
        return half <= self.MAX_LEVELS and ncls <= self.MAX_CLASSES and all(a.t.dtype == self.exec.adt and a.t.is_contiguous() for a in acts)

    def _decode_host(self, acts, org) -> List[List[Dict]]:
        """every anchor of every level to the host (2 L blocking copies), numpy filters them (decode_outputs)"""
        self._check_outputs(acts)
        outs = [self.exec.values(a)[:, 0].cpu().numpy() for a in acts]
        half = len(outs) // 2
        return [self.decode_outputs([s_[i] for s_ in outs[:half]], [b_[i] for b_ in outs[half:half * 2]], org) for i in range(outs[0].shape[0])]

    def detect_host(self, pages: torch.Tensor) -> List[List[Dict]]:
        """the synchronous route: what the device tail is compared against, and the fallback for outputs it cannot read"""
        _, acts = self._graph_outputs(pages)
        return self._decode_host(acts, tuple(pages.shape[1:3]))

    def forward(self, pages: torch.Tensor, landing=None):
        cfg = self.config
        x, acts = self._graph_outputs(pages)
        key = tuple(x.shape)
        ok = self._tail_ok.get(key)
        if ok is None:
            ok = self._tail_ok[key] = self._check_outputs(acts)
        if not ok:
            return pages.shape[0], ("host", self._decode_host(acts, tuple(pages.shape[1:3])))
        half = len(acts) // 2
        counts, cands = self.eng.op_pico_candidates([a.t for a in acts[:half]], [a.t for a in acts[half:]], len(cfg.labels),
                                                    thr_lo=cfg.score_threshold - 1e-3, max_cands=self.max_cands, split=self.exec.split)
        if getattr(self, "device_decode", False):
            return self._decode_on_device(counts, cands, pages.shape[1:3], landing)
        return self._land(counts, cands, landing)

    def finish(self, n: int, ticket, org) -> List[List[Dict]]:
        if ticket[0] == "host":
            return ticket[1]
        return super().finish(n, ticket, org)

    def _decode_record_page(self, rec: np.ndarray, org) -> List[Dict]:
        return self.decode_page(rec, org, probs=True)
