"""Batched recognition stage of the PP-OCR ONNX recognisers ("PP-OCRv4" / "PP-OCRv3" / "PP-Table": what ``fix_model_names()`` selects for
every language, model/ocr_pdf/configuration_ocr_document.py:128-141) with ``RecStage``'s contract -- ``start`` / ``finish`` / ``__call__`` -- so
that ``OcrTablePipeline.predict()`` and ``predict_stream()`` serve them like the in-tree recognisers.

Device half (``start``, asynchronous on the current stream, no host synchronisation of its own): quad geometry on the host,
``PPOcrRecPreProcessor.lines`` over the resident pages (48-px, width-sorted mini-batches), one walk of the generic graph executor per
mini-batch through its eager-then-replay policy (``run_device_graphed``; ``run_lines_graphed`` for exports with the batch size baked in as 1),
ending in ``pt_op_ctc_greedy`` (executor built with ``ctc_tail=True``: class id and probability per token, csrc/ctc_ops.hip) -- and the ids and
probabilities of ALL mini-batches on their way to one pinned host buffer, an event behind the copy.  Host half (``finish``): waits for that
event only, ``CTCLabelDecode.decode_ids`` per mini-batch, texts and scores scattered through ``indices`` back to line order.

Where the executor planned no CTC tail (a graph that returns logits, has a second output, or whose Softmax something else reads) the stage
takes the maximum and the lowest arg-max of the executor's output on the device itself: slower, still served.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from .engine import HipEngine
from .onnx_import import UnsupportedOnnxGraph
from .rec_postprocess import CTCLabelDecode
from .rec_pp_stage import PPOcrRecPreProcessor

__all__ = ["PPRecStage", "pprec_decode_host"]


def pprec_decode_host(ctc: CTCLabelDecode, ids: np.ndarray, conf: np.ndarray, spans: Sequence[Tuple[int, int, int, int]], indices: np.ndarray,
                      kept: np.ndarray, per_page: Sequence[int]):
    """The stage's host half without the device: flat ``ids`` / ``conf`` (all mini-batches back to back), ``spans`` = per mini-batch
    (batch_beg_img_no, lines, tokens per line, offset into the flat arrays), ``indices`` = the pre-processor's width-sorted order over the KEPT
    lines, ``kept`` bool per line of the page batch (False: the quad has no crop), ``per_page`` = lines per page
    -> (texts per page, scores per page), in page and line order; a dropped line is '' with score 0."""
    kept = np.asarray(kept, dtype=bool)
    n = len(kept)
    if n != sum(per_page):
        raise ValueError(f"{n} lines for pages of {list(per_page)} lines")
    texts, scores = [""] * n, [0.0] * n
    pos = np.nonzero(kept)[0]
    for beg, nb, T, off in spans:
        res = ctc.decode_ids(np.asarray(ids[off:off + nb * T]).reshape(nb, T), np.asarray(conf[off:off + nb * T]).reshape(nb, T))
        for i, (text, sc) in enumerate(res):
            k = int(pos[int(indices[beg + i])])
            texts[k], scores[k] = text, float(sc)
    out_t, out_s, o = [], [], 0
    for k in per_page:
        out_t.append(texts[o:o + k])
        out_s.append(scores[o:o + k])
        o += k
    return out_t, out_s


class PPRecStage:
    def __init__(self, eng: HipEngine, pp: PPOcrRecPreProcessor, executor, ctc: CTCLabelDecode, batch1: bool = False):
        """executor: a HipGraphExecutor on ``eng`` (built with ctc_tail=True for the one-pass tail); batch1: the export has its batch size baked
        in as 1 -- the lines of a mini-batch are walked one by one inside one captured graph"""
        if executor.eng is not eng or pp.engine is not eng:
            raise ValueError("PPRecStage: the pre-processor and the executor must run on the stage's engine")
        self.eng, self.pp, self.exec, self.ctc, self.batch1 = eng, pp, executor, ctc, bool(batch1)
        self.last_scores: List[List[float]] = []          # per page, per line: set by finish()
        self.last_widths: List[int] = []                  # img_w of the mini-batches of the last start()

    def _tokens(self, a):
        """one executor output -> (ids int32 [b, T], conf float32 [b, T])"""
        ncls = len(self.ctc.character)
        if hasattr(a, "ids"):                             # the planned CTC tail
            if a.c != ncls:
                raise UnsupportedOnnxGraph(f"recogniser output of {a.c} classes: {ncls} (blank + dictionary + space) are expected")
            return a.ids, a.conf
        if not a.seq or a.tm or a.c != ncls:
            raise UnsupportedOnnxGraph(f"recogniser output of shape {a.shape()}: [B, T, {ncls}] (blank + dictionary + space) is expected")
        v = self.exec.values(a)                           # fp32 [b, 1, T, classes]
        v = v.reshape(v.shape[0], v.shape[-2], v.shape[-1])
        conf = v.max(-1).values
        # the LOWEST index of the maximum (numpy's argmax, what the reference decodes with); torch's arg-max promises no order among equal values
        cls = torch.arange(v.shape[-1], device=v.device, dtype=torch.int32)
        ids = torch.where(v == conf.unsqueeze(-1), cls, torch.full_like(cls, v.shape[-1])).min(-1).values
        return ids.to(torch.int32), conf.to(torch.float32)

    def start(self, pages: torch.Tensor, boxes_per_page: Sequence[np.ndarray]):
        per_page = [len(b) for b in boxes_per_page]
        batches, kept = self.pp.lines_kept(pages, boxes_per_page)
        self.last_widths = [int(b["image"].shape[-1]) for b in batches]
        if not batches:
            return per_page, kept, [], None, None, 0, None, None
        ex = self.exec
        parts_i, parts_c, spans, off = [], [], [], 0
        for b in batches:
            img = b["image"]                              # f32 [n, 3, 48, img_w], a view of the pre-processor's buffer
            n = int(img.shape[0])
            x = img.permute(0, 2, 3, 1).contiguous()
            if not ex.split:                              # the tolerance mode takes the fp32 image and splits it into (hi, lo) itself
                x = x.to(ex.adt)
            if self.batch1:
                toks = [self._tokens(o[0]) for o in ex.run_lines_graphed(x, 3)]
                ids, conf = torch.cat([t[0] for t in toks]), torch.cat([t[1] for t in toks])
            else:
                ids, conf = self._tokens(ex.run_device_graphed(x, 3)[0])
            T = int(ids.shape[-1])
            if tuple(ids.shape) != (n, T) or tuple(conf.shape) != (n, T):
                raise UnsupportedOnnxGraph(f"recogniser returned {tuple(ids.shape)} tokens for {n} lines")
            # a replayed graph returns its own buffers, which the next mini-batch of the same shape overwrites: out of them now, in stream order
            parts_i.append(ids.reshape(-1).clone())
            parts_c.append(conf.reshape(-1).view(torch.int32).clone())
            spans.append((int(b["batch_beg_img_no"]), n, T, off))
            off += n * T
        dev = torch.cat(parts_i + parts_c)                # [ids of every mini-batch | the bits of their probabilities]: one copy to the host
        host = torch.empty((2 * off,), dtype=torch.int32, pin_memory=True)
        host.copy_(dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return per_page, kept, spans, batches[0]["indices"], host, off, done, dev      # dev: alive until finish() has seen the copy

    def finish(self, state) -> List[List[str]]:
        per_page, kept, spans, indices, host, total, done, _ = state
        ids = conf = np.zeros(0, np.int32)
        if host is not None:
            done.synchronize()                            # THAT copy, not whatever has been queued on the stream since
            h = host.numpy()
            ids, conf = h[:total], h[total:].view(np.float32)
        self.eng.check()                                  # the batch has executed: surface device-side failures of it
        texts, self.last_scores = pprec_decode_host(self.ctc, ids, conf, spans, indices, kept, per_page)
        return texts

    def __call__(self, pages: torch.Tensor, boxes_per_page: Sequence[np.ndarray]) -> List[List[str]]:
        return self.finish(self.start(pages, boxes_per_page))
