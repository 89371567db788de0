"""Batched table-structure recognition with SLANet (PaddleOCR ``{ch,en}_ppstructure_mobile_v2.0_SLANet_infer``, the reference's ONNX-only
structure model): crop geometry and the label decode on the host, everything else on the GPU.

Replaces, for a batch of table crops of resident pages, the reference's per-table chain ``SLANetPreprocessor.__call__``
(model/slanet/processor_slanet.py:66-108) -> onnxruntime (``BaseInferTask.infer``; the head is an ONNX ``Loop`` of 501 steps) ->
``SLANetPostProcessor.__call__`` (:123-148):

  * ``pt_slanet_preprocess``: the crop as BGR, ratio = 488 / max(h, w), cv2.resize bilinear to (int(w ratio), int(h ratio)), DB's mean / std in
    that BGR order, zero padding to 488 x 488 at the top-left -- one launch per micro-batch of tables;
  * the feed-forward part of the graph (``onnx_import.split_sla_head``'s prefix) on the generic executor, eager once then replayed;
  * the whole greedy walk of the head as ONE ``pt_op_sla_decode`` launch with ``eos_id`` set (csrc/sla_head.hip): a table stops behind its first
    ``eos`` at a step > 0, exactly where ``TableLabelDecode.decode`` stops reading;
  * ONE non-blocking copy per micro-batch of ids, the probabilities of the chosen ids, boxes and step counts to pinned memory, an event behind it;
  * host: ``TableLabelDecode.decode_ids`` and ``slanet_shape_result`` (pdf_table_amd/rec_postprocess.py).

Stage contract as ``CenterNetStage``: ``stage(pages, boxes_per_page, page_frame=...)`` -> per page, per table the reference's dict
(``polygons``, ``structure_str_list``, plus ``score``).  With ``text_boxes=`` (the pages' recognised lines, page pixels) every table also gets
``"matched"``: {cell ordinal: [indices of the page's lines, in page order]} -- ``TableMatch(filter_ocr_result=True)``'s filter and ``match_result`` over
the table's candidate lines, computed by ONE ``pt_op_table_match`` launch per micro-batch on the head's outputs while they are still on the device
(csrc/table_match.hip; pdf_table_amd/table_structure_match.py is the same arithmetic in numpy and what the tests compare with)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import TSR_TABLE_DTYPE, HipEngine
from .onnx_import import SlaHeadParams, UnsupportedOnnxGraph
from .rec_postprocess import TableLabelDecode, slanet_shape_result
from .table_text_match import texts_in_table
from .weights import pack_sla_head

__all__ = ["SlaNetStage", "slanet_resized_size", "slanet_shape_list"]


def slanet_resized_size(h: int, w: int, max_len: int = 488) -> Tuple[int, int, float]:
    """ResizeTableImage (db_pp/table_ops.py:196-201): -> (resize_h, resize_w, ratio); ``int()`` truncates"""
    ratio = max_len / (max(h, w) * 1.0)
    return int(h * ratio), int(w * ratio), ratio


def slanet_shape_list(h: int, w: int, max_len: int = 488) -> np.ndarray:
    """the ``shape`` the pre-processor hands to the decode: [h, w, ratio, ratio, pad_h, pad_w]"""
    ratio = slanet_resized_size(h, w, max_len)[2]
    return np.array([h, w, ratio, ratio, max_len, max_len])


class SlaNetStage:
    def __init__(self, eng: HipEngine, executor, head: SlaHeadParams, decode: TableLabelDecode, size: int = 488, micro_batch: int = 16):
        """executor: a HipGraphExecutor on ``eng`` over split_sla_head's prefix model; head: its SlaHeadParams; size: the side of the network
        input (the reference's table_max_len, 488; tests use smaller ones)"""
        if executor.eng is not eng:
            raise ValueError("SlaNetStage: the executor must run on the stage's engine")
        if head.n_cls != len(decode.character):
            raise UnsupportedOnnxGraph(f"SLANet head of {head.n_cls} classes, the dictionary has {len(decode.character)} (sos + lines + eos)")
        self.eng, self.exec, self.head, self.decode = eng, executor, head, decode
        self.size, self.micro_batch = int(size), max(1, int(micro_batch))
        w16, vec = pack_sla_head(head.weights, fmt=executor.fmt, split=executor.split)
        self._w16 = torch.from_numpy(w16.view(np.int16)).to(eng._tdev)
        self._f32 = torch.from_numpy(vec).to(eng._tdev)
        # 1 at the tokens that own a box (TableLabelDecode.td_token): what pt_op_table_match calls a cell row
        self._cell_flags_host = np.zeros(len(decode.character), np.uint8)
        self._cell_flags_host[[decode.dict[t] for t in decode.td_token if t in decode.dict]] = 1
        self._cell_flags = torch.from_numpy(self._cell_flags_host).to(eng._tdev)

    def tables(self, page_shape: Tuple[int, int], boxes_per_page: Sequence[np.ndarray]) -> np.ndarray:
        """integer table boxes [k, 4] (x1, y1, x2, y2) per page, cropped like crop_image_by_box (img[y1:y2, x1:x2]) -> pt_tsr_table records"""
        ph, pw = page_shape
        recs = []
        for pi, boxes in enumerate(boxes_per_page):
            for b in np.asarray(boxes).reshape(-1, 4):
                x1, y1, x2, y2 = (int(v) for v in b)
                x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, pw), min(y2, ph)
                if x2 - x1 <= 0 or y2 - y1 <= 0:
                    raise ValueError(f"empty table crop {b.tolist()} on a {ph}x{pw} page")
                r = np.zeros((), dtype=TSR_TABLE_DTYPE)
                r["page"], r["x0"], r["y0"], r["crop_w"], r["crop_h"] = pi, x1, y1, x2 - x1, y2 - y1
                recs.append(r)
        return np.array(recs, dtype=TSR_TABLE_DTYPE) if recs else np.zeros(0, dtype=TSR_TABLE_DTYPE)

    def candidate_lines(self, tables: np.ndarray, text_boxes: Sequence[np.ndarray]) -> List[np.ndarray]:
        """per table the indices (ascending = page order) of its page's text lines whose rounded centre lies in the crop grown by 2 pixels
        (get_text_in_table_bbox, diff = 2): the lines the reference hands to TableMatch"""
        out = []
        for r in tables:
            tb = np.asarray(text_boxes[int(r["page"])], np.float64).reshape(-1, 4)
            x0, y0 = float(r["x0"]), float(r["y0"])
            out.append(texts_in_table((x0, y0, x0 + float(r["crop_w"]), y0 + float(r["crop_h"])), tb, diff=2) if len(tb) else np.zeros(0, np.int64))
        return out

    def start(self, pages: torch.Tensor, tables: np.ndarray, text_boxes: Optional[Sequence[np.ndarray]] = None):
        """device half, nothing synchronises: per micro-batch pre-process -> prefix graph -> one head launch -> one copy to pinned memory.
        text_boxes (per page [t, 4] = (min x, min y, max x, max y) in page pixels, table_text_match.text_boxes): the lines of every table are
        matched to its cells on the device as well -- candidates chosen here on the host, their boxes, the per-table offsets and frames uploaded in ONE
        pinned non-blocking copy, one pt_op_table_match launch behind the head, its [lines] int32 riding on the same copy back"""
        hd, ex = self.head, self.exec
        T, L = hd.steps, hd.n_loc
        cand = self.candidate_lines(tables, text_boxes) if text_boxes is not None else None
        pending = []
        for i in range(0, len(tables), self.micro_batch):
            tb = tables[i:i + self.micro_batch]
            n = len(tb)
            x = self.eng.slanet_preprocess(pages, tb, self.size)
            if not ex.split:                                  # the tolerance mode takes the fp32 image and splits it into (hi, lo) itself
                x = x.to(ex.adt)
            a = ex.run_device_graphed(x, 3)[0]
            if a.flat or a.seq or a.c != hd.channels:
                raise UnsupportedOnnxGraph(f"SLANet prefix returned a tensor of shape {a.shape()}: a [B, {hd.channels}, h, w] map is expected")
            fea = a.t.reshape(n, a.t.shape[1] * a.t.shape[2], a.t.shape[3])
            probs, loc, ids, steps = self.eng.op_sla_decode(fea, hd.channels, self._w16, self._f32, hd.hidden, hd.n_cls, hd.n_loc, T,
                                                            eos_id=self.decode.end_idx, split=ex.split)
            chosen = probs.gather(2, ids.long().unsqueeze(-1)).squeeze(-1)
            parts = [ids.reshape(-1), steps, chosen.reshape(-1).view(torch.int32), loc.reshape(-1).view(torch.int32)]
            lines_of = up = None
            if cand is not None:
                lines_of = cand[i:i + n]
                offs = np.zeros(n + 1, np.int32)
                offs[1:] = np.cumsum([len(c) for c in lines_of])
                m = int(offs[-1])
                # the decode's scaling (x times the crop's width, y times its height) and the page-frame shift, per table
                frames = np.stack([tb["crop_w"], tb["crop_h"], tb["x0"], tb["y0"]], 1).astype(np.float32)
                boxes = [np.asarray(text_boxes[int(r["page"])], np.float64).reshape(-1, 4)[c] for r, c in zip(tb, lines_of)]
                buf = np.concatenate([np.concatenate(boxes).astype(np.float32).reshape(-1).view(np.int32), offs, frames.reshape(-1).view(np.int32)])
                up = torch.from_numpy(buf).pin_memory().to(self.eng._tdev, non_blocking=True)
                parts.append(self.eng.op_table_match(loc, ids, steps, self._cell_flags, up[4 * m + n + 1:].view(torch.float32).reshape(n, 4),
                                                     up[:4 * m].view(torch.float32).reshape(m, 4), up[4 * m:4 * m + n + 1]))
            dev = torch.cat(parts)
            host = torch.empty(dev.shape, dtype=torch.int32, pin_memory=True)
            host.copy_(dev, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            pending.append((i, n, host, done, (dev, up), lines_of))      # dev, up: alive until finish() has seen the copy
        return pending

    def finish(self, pending, tables: np.ndarray, page_frame: bool = False) -> List[Dict]:
        T, L = self.head.steps, self.head.n_loc
        out: List[Dict] = []
        for (i, n, host, done, _dev, lines_of) in pending:
            if lines_of is not None and not page_frame:
                raise ValueError("SlaNetStage: text lines are matched in page pixels: text_boxes needs page_frame=True")
            done.synchronize()                                 # THAT copy, not whatever has been queued on the stream since
            h = host.numpy()
            ids, steps = h[:n * T].reshape(n, T), h[n * T:n * T + n]
            o = n * T + n
            chosen = h[o:o + n * T].view(np.float32).reshape(n, T)
            loc = h[o + n * T:o + n * T + n * T * L].view(np.float32).reshape(n, T, L)
            match = h[o + n * T + n * T * L:]
            tb = tables[i:i + n]
            shapes = np.stack([slanet_shape_list(int(r["crop_h"]), int(r["crop_w"]), self.size) for r in tb])
            res = self.decode.decode_ids(ids, chosen, loc, shapes, steps)
            m0 = 0
            for k in range(n):
                toks, score = res["structure_batch_list"][k]
                d = slanet_shape_result(toks, res["bbox_batch_list"][k])
                del d["inputs"]
                d["score"] = float(score)
                if page_frame and len(d["polygons"]):
                    off = np.tile(np.array([tb[k]["x0"], tb[k]["y0"]], d["polygons"].dtype), d["polygons"].shape[1] // 2)
                    d["polygons"] = d["polygons"] + off[None]
                if lines_of is not None:
                    # step index -> cell ordinal (the k-th cell row is the k-th polygon), line position -> index of the line on its page
                    ordinal = np.cumsum(self._cell_flags_host[ids[k, :int(steps[k])]]) - 1
                    matched: Dict[int, List[int]] = {}
                    for line, t in zip(lines_of[k].tolist(), match[m0:m0 + len(lines_of[k])].tolist()):
                        if t >= 0:
                            matched.setdefault(int(ordinal[t]), []).append(line)
                    m0 += len(lines_of[k])
                    d["matched"] = matched
                out.append(d)
        self.eng.check()                                       # the batch has executed: surface device-side failures of it
        return out

    def __call__(self, pages: torch.Tensor, boxes_per_page: Sequence[np.ndarray], page_frame: bool = False,
                 text_boxes: Optional[Sequence[np.ndarray]] = None) -> List[List[Dict]]:
        tables = self.tables(tuple(pages.shape[1:3]), boxes_per_page)
        flat = self.finish(self.start(pages, tables, text_boxes), tables, page_frame) if len(tables) else []
        res, o = [], 0
        for b in boxes_per_page:
            k = len(np.asarray(b).reshape(-1, 4))
            res.append(flat[o:o + k])
            o += k
        return res
