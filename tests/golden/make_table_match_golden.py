"""Record tests/golden/table_match.json from the reference's own TableMatch (model/ocr_pdf/table/matcher.py and table_master_match.py, loaded by
file path; table_master_match imports two shapely names that neither function under test uses: they are stubbed in sys.modules).

    python tests/golden/make_table_match_golden.py /path/to/reference/src/pdftable/model/ocr_pdf/table

Every case holds the inputs (cells with their dtype, integer text boxes as the reference's ``np.array(dt_boxes)``, texts, structure tokens) and what
``TableMatch(filter_ocr_result=True)`` gives: the lines ``_filter_ocr_result`` keeps, ``match_result`` on them (pairs in dict order) and the HTML string
of ``__call__`` with use_master False and True.  Cases:
  f32_4 / f32_8         4-value and 8-value float32 fractional cells
  i32_8_mtl             int32 polygons and merged master tokens (MtlTabNet / TableMaster)
  iou0_equal_distance   every pair at IoU 0, cells 1 and 2 at the same distance from the line (the lower index wins), cell 0 further away
  iou0_distance_decides equal 1 - iou (IoU 0), the distance decides
  equal_iou_mirror      two cells overlapping the line as mirror images: equal IoU and equal distance
  identical_cells       the same cell at two indices
  y_filter              a line whose ymax equals the smallest cell y (kept) and one a pixel above (dropped)
  html_lines            several lines in one cell: leading and trailing spaces, empty strings, <b>..</b> content, a text equal to '<b>'; <td></td>,
                        <td .. > with spans, thead / tbody
  html_master_tokens    merged span tokens and <eb..> variants
  no_lines              a table without candidate lines
  random_f32_dense      40 lines x 30 fractional cells that overlap a lot: every branch of the mixed float32 / float64 intersection arithmetic
  f32_area_decides      two cells that both contain the line, so the IoU order is the order of the cells' own areas: found by a seeded search
                        (SEARCH_SEED, the trial is recorded) such that the float32-rounded areas order the cells differently from the exact ones;
                        ``float64_winner`` is what match_result gives on the same cells cast to float64"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEARCH_SEED = 20


def load_reference(table_dir):
    shapely, geometry = types.ModuleType("shapely"), types.ModuleType("shapely.geometry")
    geometry.Polygon = geometry.MultiPoint = object
    shapely.geometry = geometry
    sys.modules.setdefault("shapely", shapely)
    sys.modules.setdefault("shapely.geometry", geometry)
    pkg = types.ModuleType("ref_table")
    pkg.__path__ = [table_dir]
    sys.modules["ref_table"] = pkg
    mods = {}
    for name in ("table_master_match", "matcher"):
        spec = importlib.util.spec_from_file_location("ref_table." + name, os.path.join(table_dir, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_table." + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["matcher"]


SLA_TOKENS = ["<html>", "<body>", "<table>", "<thead>", "<tr>", "<td></td>", "<td", ' colspan="2"', ">", "</td>", "</tr>", "</thead>", "<tbody>", "<tr>",
              "<td></td>", "<td></td>", "<td", ' rowspan="2"', ' colspan="3"', ">", "</td>", "</tr>", "</tbody>", "</table>", "</body>", "</html>"]
MASTER_TOKENS = ["<html>", "<body>", "<table>", "<thead>", "<tr>", "<td></td>", '<td colspan="2"></td>', "<eb5></eb5>", "</tr>", "</thead>", "<tbody>", "<tr>",
                 "<td></td>", "<eb></eb>", "<eb2></eb2>", '<td rowspan="2"></td>', "<eb10></eb10>", "<td></td>", "</tr>", "</tbody>", "</table>", "</body>",
                 "</html>"]


def plain_tokens(n):
    return ["<html>", "<body>", "<table>", "<tr>"] + ["<td></td>"] * n + ["</tr>", "</table>", "</body>", "</html>"]


def grid(dtype, frac):
    """5 cells: a head row of two, a body row of three"""
    c = np.array([[10, 10, 100, 30], [100, 10, 300, 30], [10, 30, 100, 60], [100, 30, 200, 60], [200, 30, 300, 60]], np.float64)
    return (c + frac).astype(dtype)


def poly8(c4, skew):
    x1, y1, x2, y2 = c4.T
    return np.stack([x1, y1, x2, y1 + skew, x2, y2, x1, y2 - skew], 1).astype(c4.dtype)


def cases():
    out = []
    g = np.random.default_rng(5)
    lines = np.array([[12, 12, 60, 26], [110, 11, 220, 29], [14, 34, 90, 44], [14, 46, 80, 58], [120, 35, 190, 55], [205, 33, 290, 57], [150, 62, 260, 75]])
    texts = ["Name", "Total amount", "first", "second", "12.5", "ok", "below the table"]
    out.append(dict(name="f32_4", cells=grid(np.float32, 0.37), lines=lines, texts=texts, tokens=SLA_TOKENS))
    out.append(dict(name="f32_8", cells=poly8(grid(np.float32, 0.61), np.float32(1.75)), lines=lines, texts=texts, tokens=SLA_TOKENS))
    out.append(dict(name="i32_8_mtl", cells=poly8(grid(np.int32, 0), 0), lines=lines, texts=texts, tokens=MASTER_TOKENS))
    out.append(dict(name="iou0_equal_distance", cells=np.array([[300, 100, 320, 110], [50, 100, 70, 110], [150, 100, 170, 110]], np.float32),
                    lines=np.array([[100, 100, 120, 110]]), texts=["x"], tokens=plain_tokens(3)))
    out.append(dict(name="iou0_distance_decides", cells=np.array([[50, 100, 70, 110], [130, 100, 150, 110], [300, 100, 320, 110]], np.float32),
                    lines=np.array([[100, 100, 120, 110], [290, 112, 310, 120]]), texts=["x", "y"], tokens=plain_tokens(3)))
    out.append(dict(name="equal_iou_mirror", cells=np.array([[400, 100, 440, 120], [90, 100, 130, 120], [110, 100, 150, 120]], np.float32),
                    lines=np.array([[100, 100, 140, 120]]), texts=["x"], tokens=plain_tokens(3)))
    out.append(dict(name="identical_cells", cells=np.array([[10, 10, 50, 30], [60.5, 10.25, 120.5, 30.75], [60.5, 10.25, 120.5, 30.75]], np.float32),
                    lines=np.array([[62, 12, 118, 29], [12, 12, 48, 28]]), texts=["twice", "once"], tokens=plain_tokens(3)))
    out.append(dict(name="y_filter", cells=np.array([[10, 50, 100, 70], [100, 52.5, 200, 70]], np.float32),
                    lines=np.array([[12, 40, 90, 50], [12, 39, 90, 49], [110, 30, 190, 49], [110, 55, 190, 68], [12, 50, 90, 41]]),
                    texts=["touches", "above", "above too", "inside", "upside"], tokens=plain_tokens(2)))
    many = np.array([[12, 11, 40, 19], [42, 11, 70, 19], [12, 20, 40, 28], [44, 20, 90, 28], [110, 11, 160, 19], [165, 11, 220, 19], [110, 20, 200, 28],
                     [14, 34, 90, 44], [14, 46, 80, 58], [120, 35, 190, 55], [205, 33, 240, 43], [245, 33, 290, 43], [205, 45, 290, 57]])
    many_texts = [" lead", "trail ", "", "<b>bold</b>", "<b>", "head", "<b>x</b> ", "solo ", "", "<b>one</b>", "", " ", "a"]
    out.append(dict(name="html_lines", cells=grid(np.float32, 0.37), lines=many, texts=many_texts, tokens=SLA_TOKENS))
    out.append(dict(name="html_master_tokens", cells=grid(np.int32, 0), lines=many, texts=many_texts, tokens=MASTER_TOKENS))
    out.append(dict(name="no_lines", cells=grid(np.float32, 0.37), lines=np.zeros((0, 4), np.int64), texts=[], tokens=SLA_TOKENS))
    xy = g.uniform(0, 400, (30, 2))
    wh = g.uniform(20, 300, (30, 2))
    dense = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    lxy = g.integers(0, 500, (40, 2))
    lwh = g.integers(5, 250, (40, 2))
    out.append(dict(name="random_f32_dense", cells=dense, lines=np.concatenate([lxy, lxy + lwh], 1), texts=[f"t{i}" for i in range(40)],
                    tokens=plain_tokens(30)))
    return out


def area_case(ref):
    """two cells around one line; cell 1 is cell 0 moved by a fraction of a pixel: equal areas in real numbers, unequal once rounded"""
    tm = ref.TableMatch(filter_ocr_result=True)
    g = np.random.default_rng(SEARCH_SEED)
    for trial in range(100000):
        line = np.array([[1500, 900, 1700, 940]])
        x1, y1 = g.uniform(1000, 1400), g.uniform(500, 800)
        w, h = g.uniform(800, 1500), g.uniform(500, 900)
        dx, dy = g.uniform(0.1, 0.9, 2)
        cells = np.array([[x1, y1, x1 + w, y1 + h], [x1 + dx, y1 + dy, x1 + dx + w, y1 + dy + h]]).astype(np.float32)
        a32 = (cells[:, 2] - cells[:, 0]) * (cells[:, 3] - cells[:, 1])
        c64 = cells.astype(np.float64)
        a64 = (c64[:, 2] - c64[:, 0]) * (c64[:, 3] - c64[:, 1])
        if a32[0] == a32[1] or a64[0] == a64[1] or (a32[0] < a32[1]) == (a64[0] < a64[1]):
            continue
        w32 = list(tm.match_result(list(line), cells))[0]
        w64 = list(tm.match_result(list(line), c64))[0]
        if w32 != w64:
            return dict(name="f32_area_decides", cells=cells, lines=line, texts=["x"], tokens=plain_tokens(2), search_seed=SEARCH_SEED, trial=trial,
                        float64_winner=int(w64))
    raise SystemExit("no float32-area case found")


def record(ref, case):
    tm = ref.TableMatch(filter_ocr_result=True)
    cells, lines = case["cells"], np.asarray(case["lines"], np.int64)
    rec_res = [(t, 1) for t in case["texts"]]
    kept_boxes, kept_idx = tm._filter_ocr_result(cells, lines, [(i, 1) for i in range(len(lines))])
    matched = tm.match_result(kept_boxes, cells)
    res = {k: v for k, v in case.items() if k not in ("cells", "lines")}
    res.update(cells=[[float(v) for v in row] for row in cells], cell_dtype=str(cells.dtype), lines=lines.tolist(),
               kept=[int(i) for i, _ in kept_idx], matched=[[int(k), [int(i) for i in v]] for k, v in matched.items()],
               html=tm((case["tokens"], cells), lines, rec_res, use_master=False), html_master=tm((case["tokens"], cells), lines, rec_res, use_master=True))
    return res


def main(table_dir):
    ref = load_reference(table_dir)
    out = [record(ref, c) for c in cases() + [area_case(ref)]]
    with open(os.path.join(HERE, "table_match.json"), "w") as f:
        json.dump({"numpy": np.__version__, "cases": out}, f, indent=1, ensure_ascii=True)
    for c in out:
        print(c["name"], "kept", c["kept"], "matched", c["matched"][:6])


if __name__ == "__main__":
    main(sys.argv[1])
