"""PP-OCR flavour of the recognition post-process: ``CTCLabelDecode`` (reference:
src/pdftable/model/ocr_rec_pp/rec_postprocess.py:17-195) over the engine's fused arg-max output.

The reference takes the full ``[batch, T, classes]`` probability tensor, does ``argmax(axis=2)`` / ``max(axis=2)`` on the
host and decodes.  The engine never materialises that tensor: the classifier GEMM's epilogue already yields, per time
step, the winning class id and its value, so this class starts from ``(ids int [B,T], probs float [B,T])``.
Character table: ``['blank'] + dict lines (+ ' ' if use_space_char)``; blank (0) and repeats are dropped; confidence is
the mean of the kept per-step maxima (``[0]`` -> 0.0 for an empty string); Arabic dictionaries reverse the text while
keeping latin/digit runs in order (``pred_reverse``).

``TableLabelDecode`` is SLANet's (reference: src/pdftable/model/slanet/table_postprocess.py:172-290) over the head kernel's output -- class id and its
probability per step, one box per step -- and ``slanet_shape_result`` the shaping of ``SLANetPostProcessor.__call__`` (processor_slanet.py:123-148).
"""
from __future__ import annotations

import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["CTCLabelDecode", "TableLabelDecode", "slanet_shape_result"]

_LATIN_RUN = re.compile("[a-zA-Z0-9 :*./%+-]")


class CTCLabelDecode:
    def __init__(self, character_dict_path: Optional[str] = None, use_space_char: bool = False,
                 characters: Optional[Sequence[str]] = None):
        self.reverse = False
        if characters is not None:
            chars = list(characters)
        elif character_dict_path is None:
            chars = list("0123456789abcdefghijklmnopqrstuvwxyz")
        else:
            with open(character_dict_path, "rb") as fin:
                chars = [ln.decode("utf-8").strip("\n").strip("\r\n") for ln in fin.readlines()]
            if use_space_char:
                chars.append(" ")
            self.reverse = "arabic" in character_dict_path
        self.character = ["blank"] + chars
        self.dict = {c: i for i, c in enumerate(self.character)}

    @staticmethod
    def pred_reverse(pred: str) -> str:
        out, run = [], ""
        for c in pred:
            if _LATIN_RUN.search(c):
                run += c
            else:
                if run:
                    out.append(run)
                out.append(c)
                run = ""
        if run:
            out.append(run)
        return "".join(out[::-1])

    def decode_ids(self, ids: np.ndarray, probs: Optional[np.ndarray] = None) -> List[Tuple[str, float]]:
        ids = np.asarray(ids)
        res = []
        for b in range(ids.shape[0]):
            row = ids[b]
            keep = np.ones(len(row), dtype=bool)
            keep[1:] = row[1:] != row[:-1]
            keep &= row != 0
            text = "".join(self.character[int(t)] for t in row[keep])
            conf = probs[b][keep] if probs is not None else np.ones(len(row))      # reference: [1] * len(selection), never empty
            if len(conf) == 0:
                conf = [0]
            if self.reverse:
                text = self.pred_reverse(text)
            res.append((text, np.mean(conf).tolist()))
        return res

    def __call__(self, preds, **kwargs):
        """Reference call shape: preds float [B, T, classes] (kept for drop-in use and for the golden test)."""
        if isinstance(preds, (tuple, list)):
            preds = preds[-1]
        preds = np.asarray(preds)
        return self.decode_ids(preds.argmax(axis=2), preds.max(axis=2))


class TableLabelDecode:
    """Structure tokens and cell boxes of one SLANet walk.  Character table: ``['sos'] + dict lines + ['eos']``; with ``merge_no_span_structure`` the
    dictionary first gains ``<td></td>`` (if absent) and loses ``<td>``.  Per table: steps are read until the first ``eos`` at a step > 0; ``sos`` and
    ``eos`` themselves are skipped; every ``<td>`` / ``<td`` / ``<td></td>`` token takes that step's box, x values times the crop's width and y values times
    its height; the score is the mean probability of the kept tokens (NaN for an empty table, as ``np.mean([])`` gives the reference)."""
    beg_str, end_str = "sos", "eos"
    td_token = ("<td>", "<td", "<td></td>")

    def __init__(self, character_dict_path: Optional[str] = None, merge_no_span_structure: bool = False, characters: Optional[Sequence[str]] = None):
        if characters is not None:
            chars = list(characters)
        else:
            with open(character_dict_path, "rb") as fin:
                chars = [ln.decode("utf-8").strip("\n").strip("\r\n") for ln in fin.readlines()]
        if merge_no_span_structure:
            if "<td></td>" not in chars:
                chars.append("<td></td>")
            if "<td>" in chars:
                chars.remove("<td>")
        self.character = [self.beg_str] + chars + [self.end_str]
        self.dict = {c: i for i, c in enumerate(self.character)}
        self.beg_idx, self.end_idx = self.dict[self.beg_str], self.dict[self.end_str]

    def decode_ids(self, ids: np.ndarray, probs: np.ndarray, boxes: np.ndarray, shape_list: np.ndarray, steps: Optional[np.ndarray] = None):
        """ids int [B, T], probs float [B, T] (probability of the chosen id), boxes float [B, T, L], shape_list [B, 6] = (h, w, ratio_h, ratio_w, pad_h,
        pad_w); steps int [B]: rows of each table the head wrote (it stops behind the first eos at a step > 0; None: all T) ->
        {"bbox_batch_list": [float array [cells, L]], "structure_batch_list": [[tokens, score]]}"""
        ids, probs, boxes = np.asarray(ids), np.asarray(probs), np.asarray(boxes)
        out_s, out_b = [], []
        for b in range(ids.shape[0]):
            toks, bbs, scores = [], [], []
            n = ids.shape[1] if steps is None else int(steps[b])
            h, w = float(shape_list[b][0]), float(shape_list[b][1])
            for t in range(n):
                k = int(ids[b, t])
                if t > 0 and k == self.end_idx:
                    break
                if k in (self.beg_idx, self.end_idx):
                    continue
                text = self.character[k]
                if text in self.td_token:
                    bb = np.array(boxes[b, t], dtype=boxes.dtype)
                    bb[0::2] *= w
                    bb[1::2] *= h
                    bbs.append(bb)
                toks.append(text)
                scores.append(probs[b, t])
            out_s.append([toks, np.mean(scores) if scores else np.float64("nan")])       # np.mean([]) is NaN in the reference too (with a warning)
            out_b.append(np.array(bbs))
        return {"bbox_batch_list": out_b, "structure_batch_list": out_s}

    def __call__(self, preds, batch=None):
        """Reference call shape: preds {"structure_probs" [B, T, V], "loc_preds" [B, T, L]}, batch[-1] the shape list"""
        sp, lp = np.asarray(preds["structure_probs"]), np.asarray(preds["loc_preds"])
        return self.decode_ids(sp.argmax(axis=2), sp.max(axis=2), lp, batch[-1])


def slanet_shape_result(tokens: List[str], boxes: np.ndarray, inputs=None) -> dict:
    """SLANetPostProcessor's result of one table: the tokens wrapped in the html / body / table tags, 4-value boxes (x1, y1, x2, y2) expanded to 8-value
    polygons (x1, y1, x2, y1, x2, y2, x1, y2), 8-value boxes passed through"""
    tokens = ["<html>", "<body>", "<table>"] + list(tokens) + ["</table>", "</body>", "</html>"]
    boxes = np.asarray(boxes)
    if len(boxes) > 0 and len(boxes[0]) == 4:
        boxes = np.array([[x1, y1, x2, y1, x2, y2, x1, y2] for (x1, y1, x2, y2) in boxes])
    return {"polygons": boxes, "structure_str_list": tokens, "inputs": inputs}
