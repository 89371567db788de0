"""Structure tokens + one box per cell + recognised text lines -> table HTML on the host: the reference's TOKEN route.

The reference's system path has two routes from a table-structure result to HTML (ocr_table_to_html_task.py:139-156).  Cells with logical
locations (Lore) go through ``match_table_cell_and_text_cell`` (pdf_table_amd/table_text_match.py).  Structure models that return a token
sequence plus one box per cell -- SLANet, MtlTabNet, TableMaster -- are marked ``"not_spit_text"`` by ``convert_table_sep_to_merge``
(pdf_table/table_common.py:1852-1867) and go through ``match_table_structure_and_text_cell`` (:245-277), i.e. PP-Structure's
``TableMatch(filter_ocr_result=True)`` (ocr_pdf/table/matcher.py) with ``use_master = config.tsr_match_need_use_master()``.  This module
restates that route:

  * ``filter_lines``  = ``_filter_ocr_result``: a line is dropped when max(y1, y2) is strictly below the smallest cell y;
  * ``match_result``  = ``match_result``: per line the cell with the smallest (1 - iou, distance), the lowest index among equal keys; the
    reference's Python double loop as numpy passes over [lines, cells];
  * ``pred_html`` / ``pred_html_master`` = ``get_pred_html`` / ``get_pred_html_master``;
  * ``structure_table_html`` = the one-element list of ``match_table_structure_and_text_cell`` (:272-277), ``.replace`` chain included.

Arithmetic of ``match_result`` (what matcher.py computes with numpy 2 scalars on float32 cell polygons and integer or float64 text boxes;
tests/golden/table_match.json holds recorded results, one case where the float32 rounding decides the winner):
  * ``distance`` is float64: the float32 cell values are widened, the four absolute differences are added left to right;
  * the cell's own area (x2 - x1) * (y2 - y1) is float32: both differences and the product are rounded to float32;
  * the builtin max / min return one of their operands (the text box's on equality), so an edge pair of the intersection that comes from
    the cell alone is subtracted in float32, and an intersection whose two extents are both float32 is a float32 product;
  * everything else is float64.
Integer cells (MtlTabNet / TableMaster: int32 polygons) are exact in float64 whatever the order.

Reference behaviours kept on purpose: ``rec_res`` entries are ``(text, 1)`` tuples, so ``'<b>' in ocr_contents[i]`` is a tuple-membership test
(true only for a line whose whole text is ``'<b>'``); the ``ocr_post_process`` argument is unused on this route; a table without cells gets
no HTML (``[]``: the reference's ``.min()`` of an empty array raises and the table is skipped)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

# table_master_match.py's deal_eb_token and one-argument deal_bb (the <thead> section only) are, replacement for replacement and pattern for
# pattern, what mtl_stage restates from master_post_processor.py (deal_bb with its default tag): shared, not copied
from .mtl_stage import deal_bb, deal_eb_token

__all__ = ["cell_boxes", "filter_lines", "match_keys", "match_result", "pred_html", "pred_html_master", "structure_table_html",
           "use_master_for"]


def use_master_for(model: str) -> bool:
    """OCRDocumentConfig.tsr_match_need_use_master (configuration_ocr_document.py:160-164)"""
    return model in ("Lgpma", "MtlTabNet", "TableMaster")


def cell_boxes(cells: np.ndarray) -> np.ndarray:
    """[n, 8] polygons -> (min x, min y, max x, max y) in the polygons' own dtype; [n, 4] boxes pass through AS THEY ARE (match_result :84-88)"""
    c = np.asarray(cells)
    if c.ndim != 2 or c.shape[1] not in (4, 8):
        raise ValueError(f"cell boxes must be [n, 4] or [n, 8], got {c.shape}")
    if c.shape[1] == 4:
        return c
    return np.stack([c[:, 0::2].min(1), c[:, 1::2].min(1), c[:, 0::2].max(1), c[:, 1::2].max(1)], 1)


def filter_lines(cells: np.ndarray, line_boxes: np.ndarray) -> np.ndarray:
    """indices of the lines ``_filter_ocr_result`` keeps: max(y1, y2) >= the smallest y of any cell"""
    c = np.asarray(cells)
    lb = np.asarray(line_boxes, np.float64).reshape(-1, 4)
    y_min = c[:, 1::2].min()
    return np.flatnonzero(~(np.maximum(lb[:, 1], lb[:, 3]) < y_min))


def match_keys(line_boxes: np.ndarray, cells: np.ndarray):
    """-> (1 - iou, distance), float64 [lines, cells] each: the two sort keys of ``match_result``"""
    t = np.asarray(line_boxes, np.float64).reshape(-1, 4)[:, None, :]      # [T, 1, 4]
    cb = cell_boxes(cells)
    f32 = cb.dtype == np.float32
    c = cb.astype(np.float64)[None, :, :]                                   # [1, C, 4]
    a0, a1, a2, a3 = (np.abs(c[..., k] - t[..., k]) for k in range(4))
    d2, d3 = a0 + a1, a2 + a3
    dist = (((a0 + a1) + a2) + a3) + np.minimum(d2, d3)
    s1 = (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1])
    if f32:
        w32, h32 = cb[:, 2] - cb[:, 0], cb[:, 3] - cb[:, 1]                 # float32 differences
        s2 = (w32 * h32).astype(np.float64)[None, :]                        # float32 product
    else:
        w32 = h32 = None
        s2 = (c[..., 2] - c[..., 0]) * (c[..., 3] - c[..., 1])
    total = s1 + s2
    # max(rec1[k], rec2[k]) is the cell's value only where it is strictly larger, min(..) only where it is strictly smaller
    lo1_c, hi1_c = c[..., 1] > t[..., 1], c[..., 3] < t[..., 3]
    lo0_c, hi0_c = c[..., 0] > t[..., 0], c[..., 2] < t[..., 2]
    left, right = np.where(lo1_c, c[..., 1], t[..., 1]), np.where(hi1_c, c[..., 3], t[..., 3])
    top, bottom = np.where(lo0_c, c[..., 0], t[..., 0]), np.where(hi0_c, c[..., 2], t[..., 2])
    e1, e0 = right - left, bottom - top
    inter = e1 * e0
    if f32:
        both1, both0 = lo1_c & hi1_c, lo0_c & hi0_c
        e1 = np.where(both1, h32.astype(np.float64)[None, :], e1)
        e0 = np.where(both0, w32.astype(np.float64)[None, :], e0)
        inter = np.where(both1 & both0, (w32 * h32).astype(np.float64)[None, :], e1 * e0)
    apart = (left >= right) | (top >= bottom)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(apart, 0.0, inter / (total - inter))
    return 1.0 - iou, dist


def match_result(line_boxes: np.ndarray, cells: np.ndarray) -> Dict[int, List[int]]:
    """``TableMatch.match_result``: {cell index: [line indices, ascending]}, keys in the order of their first line"""
    matched: Dict[int, List[int]] = {}
    if len(line_boxes) == 0:
        return matched
    k1, dist = match_keys(line_boxes, cells)
    for i in range(k1.shape[0]):
        m = np.flatnonzero(k1[i] == k1[i].min())                  # lexicographic minimum, first index among equal keys
        j = int(m[np.argmin(dist[i][m])])
        matched.setdefault(j, []).append(i)
    return matched


def _cell_texts(matched: Dict[int, List[int]], td_index: int, ocr_contents):
    """the inner loop both HTML builders share (matcher.py:115-131 / :155-171): the cell's contents in order, trimmed when there are several"""
    idxs = matched[td_index]
    out = []
    for i, k in enumerate(idxs):
        content = ocr_contents[k][0]
        if len(idxs) > 1:
            if len(content) == 0:
                continue
            if content[0] == " ":
                content = content[1:]
            if "<b>" in content:
                content = content[3:]
            if "</b>" in content:
                content = content[:-4]
            if len(content) == 0:
                continue
            if i != len(idxs) - 1 and " " != content[-1]:
                content += " "
        out.append(content)
    return out


def pred_html(tokens: Sequence[str], matched: Dict[int, List[int]], ocr_contents) -> str:
    """``get_pred_html``; ocr_contents: the (text, 1) tuples"""
    end_html: List[str] = []
    td_index = 0
    for tag in tokens:
        if "</td>" not in tag:
            end_html.append(tag)
            continue
        if "<td></td>" == tag:
            end_html.append("<td>")
        if td_index in matched:
            b_with = "<b>" in ocr_contents[matched[td_index][0]] and len(matched[td_index]) > 1      # tuple membership, as in the reference
            if b_with:
                end_html.append("<b>")
            end_html.extend(_cell_texts(matched, td_index, ocr_contents))
            if b_with:
                end_html.append("</b>")
        end_html.append("</td>" if "<td></td>" == tag else tag)
        td_index += 1
    return "".join(end_html)


def pred_html_master(tokens: Sequence[str], matched: Dict[int, List[int]], ocr_contents) -> str:
    """``get_pred_html_master``: the text goes inside the token, every token through deal_eb_token, the joined string through deal_bb"""
    end_html: List[str] = []
    td_index = 0
    for token in tokens:
        if "</td>" in token:
            txt, b_with = "", False
            if td_index in matched:
                b_with = "<b>" in ocr_contents[matched[td_index][0]] and len(matched[td_index]) > 1
                txt = "".join(_cell_texts(matched, td_index, ocr_contents))
            if b_with:
                txt = "<b>{}</b>".format(txt)
            token = "<td>{}</td>".format(txt) if "<td></td>" == token else "{}</td>".format(txt)
            td_index += 1
        end_html.append(deal_eb_token(token))
    return deal_bb("".join(end_html))


def structure_table_html(tokens: Sequence[str], cells: np.ndarray, line_boxes: np.ndarray, texts: Sequence[str], use_master: bool,
                         matched: Optional[Dict[int, List[int]]] = None) -> List[str]:
    """One table -> ``table_html`` (``db_table_html`` is the same list): ``match_table_structure_and_text_cell``.  tokens: the structure
    model's ``structure_str_list``; cells: its polygons [n, 4 | 8]; line_boxes [t, 4] (min x, min y, max x, max y) and ``texts``: the
    candidate lines of the table (``texts_in_table``).  ``matched``: a match map computed elsewhere (the device's, SlaNetStage), its line
    indices pointing into ``texts``; then nothing is filtered or matched here."""
    cells = np.asarray(cells)
    if cells.ndim != 2 or len(cells) == 0:
        return []
    if matched is None:
        lb = np.asarray(line_boxes, np.float64).reshape(-1, 4)
        keep = filter_lines(cells, lb)
        matched = match_result(lb[keep], cells)
        rec_res = [(texts[i], 1) for i in keep.tolist()]
    else:
        rec_res = [(t, 1) for t in texts]
    html = pred_html_master(tokens, matched, rec_res) if use_master else pred_html(tokens, matched, rec_res)
    return [html.replace("<html><body>", "").replace("</body></html>", "").replace("<tbody>", "").replace("</tbody>", "")
            .replace("</tr>", "</tr>\n").replace("<table>", "<table class='pdf-table' border='1'>")]
