"""References for the Lore line -> cell match (csrc/lore_match.hip), shared by test_lore_match_host.py and the GPU tests.

``host_chain`` is what the pipeline computes on the host without device_match: transform_quads + the crop offset +
process_logic_output + table_cells_from_logits + find_top1_match, mapped back to INPUT rows through the sort order.
``key_rule`` restates the kernel: no sort, one key per cell in input order, the smallest key wins."""
import numpy as np

from pdf_table_amd.table_html import table_cells_from_logits
from pdf_table_amd.table_text_match import find_top1_match
from pdf_table_amd.tsr_stage import process_logic_output, transform_quads


def sorted_match_to_rows(polys, logi, lines):
    """find_top1_match over the cells in the reference's sorted order -> input rows; polys [n,8], logi [n,4] rounded"""
    cells, order = table_cells_from_logits(polys, logi, return_order=True)
    if len(lines) == 0:
        return np.zeros(0, np.int64)
    cb = np.array([[c.x1, c.y1, c.x2, c.y2] for c in cells], np.float64)
    return np.asarray(order, np.int64)[find_top1_match(lines, cb)]


def page_polygons(dets, meta, upper_left, offset):
    """quads of the decode [n, >= 8] -> page pixels as TsrStage.collect(offsets=...) delivers them (float64)"""
    polys = transform_quads(np.asarray(dets)[:, :8], meta, upper_left)
    return polys.astype(np.float64) + np.tile(np.asarray(offset, np.float64), 4)[None]


def host_chain(dets, axes, meta, upper_left, offset, lines):
    """dets [n, 9] / axes [n, 4] unrounded (the valid rows of one table), lines [m, 4] -> int64 [m] input rows"""
    return sorted_match_to_rows(page_polygons(dets, meta, upper_left, offset), process_logic_output(np.asarray(axes, np.float32)), lines)


def key_rule(polys, logi, lines, diff=2):
    """The kernel's rule in numpy: per line the input row with the smallest (k1, dist, top, left, bottom, right, row), a containing
    cell counting as (-inf, 0).  polys [n,8] page pixels, logi [n,4] = [left, right, top, bottom] rounded, lines [m,4]."""
    p = np.asarray(polys, np.float64)
    lg = np.asarray(logi)
    n = len(p)
    c0, c1, c2, c3 = p[:, 6], p[:, 7], p[:, 2], p[:, 3]          # bottom-left, top-right
    out = np.empty(len(lines), np.int64)
    rows = np.arange(n)
    for i, t in enumerate(np.asarray(lines, np.float64)):
        inside = (t[0] >= c0 - diff) & (t[2] <= c2 + diff) & (np.minimum(c1, c3) - diff <= min(t[1], t[3])) & (max(t[1], t[3]) <= np.maximum(c1, c3) + diff)
        d1 = np.abs(c0 - t[0]) + np.abs(c1 - t[1])
        d2 = np.abs(c2 - t[2]) + np.abs(c3 - t[3])
        dist = (d1 + d2) + np.minimum(d1, d2)
        ix = np.maximum(np.minimum(t[2], c2) - np.maximum(t[0], c0), 0)
        iy = np.maximum(np.minimum(t[3], c3) - np.maximum(t[1], c1), 0)
        inter = ix * iy
        a_t = abs((t[2] - t[0]) * (t[3] - t[1]))
        a_c = np.abs((c2 - c0) * (c3 - c1))
        k1 = 1.0 - inter / (a_t + a_c - inter + 1e-6)
        k1 = np.where(inside, -np.inf, k1)
        dist = np.where(inside, 0.0, dist)
        out[i] = np.lexsort((rows, lg[:, 1], lg[:, 3], lg[:, 0], lg[:, 2], dist, k1))[0]
    return out
