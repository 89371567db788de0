"""The Lore line -> cell match without a GPU: the rule csrc/lore_match.hip implements (a key reduction over the cells in INPUT order, no
sort) equals find_top1_match over the sorted cells mapped back through the sort order, and page_table_html(matched=...) gives the HTML
of the host route."""
import json
import os
import types

import numpy as np
import pytest

from lore_match_ref import key_rule, sorted_match_to_rows
from lore_synth import synth_table_grids, synth_table_texts
from pdf_table_amd import table_text_match as M
from pdf_table_amd.table_html import table_cells_from_logits


def _golden_cases(golden_dir):
    with open(os.path.join(golden_dir, "table_text_match.json")) as f:
        gold = json.load(f)
    grids = synth_table_grids(gold["seed"])
    for g in gold["cases"]:
        polys, logi = grids[g["case"]]
        boxes, texts = synth_table_texts(g["case"], polys)
        yield g, polys, logi, boxes, texts


def test_key_rule_equals_sorted_match_on_golden_cases(golden_dir):
    n = 0
    for g, polys, logi, boxes, _ in _golden_cases(golden_dir):
        tb = M.text_boxes(boxes)
        inside = M.texts_in_table(g["bbox"], tb, diff=2)
        _, order = table_cells_from_logits(polys, logi, return_order=True)
        want = np.asarray(order)[np.asarray(g["top1"], np.int64)]          # the reference's recorded answer, as input rows
        assert sorted_match_to_rows(polys, logi, tb[inside]).tolist() == want.tolist()
        assert key_rule(polys, logi, tb[inside]).tolist() == want.tolist()
        n += len(inside)
    assert n > 50


def _seeded_table(seed):
    """an R x C grid (page pixels, y grows downwards) in a random input order, three duplicated cells appended (ties in every key but
    the row), lines inside cells, across borders and outside the table; integer line boxes like the detector's"""
    rng = np.random.default_rng(seed)
    R, C = int(rng.integers(2, 9)), int(rng.integers(2, 8))
    xs = np.cumsum(np.concatenate([[30.0], rng.uniform(30, 90, C)]))
    ys = np.cumsum(np.concatenate([[50.0], rng.uniform(14, 40, R)]))
    polys, logi = [], []
    for r in range(R):
        for c in range(C):
            j = rng.uniform(-1.0, 1.0, 8)
            polys.append(np.array([xs[c], ys[r], xs[c + 1], ys[r], xs[c + 1], ys[r + 1], xs[c], ys[r + 1]]) + j)
            logi.append([c, c, r, r])
    polys, logi = np.array(polys, np.float32), np.array(logi, np.float32)
    dup = rng.choice(len(polys), 3, replace=False)
    polys, logi = np.concatenate([polys, polys[dup]]), np.concatenate([logi, logi[dup]])
    perm = rng.permutation(len(polys))                                   # logical order against input order
    polys, logi = polys[perm], logi[perm]
    lines = []
    for _ in range(40):
        k = int(rng.integers(len(polys)))
        x1, y1, x2, y2 = polys[k, 0], polys[k, 1], polys[k, 4], polys[k, 5]
        a = rng.uniform(-6, 0.4 * (x2 - x1))
        b = rng.uniform(-6, 0.4 * (x2 - x1))
        c = rng.uniform(-4, 0.3 * (y2 - y1))
        d = rng.uniform(-4, 0.3 * (y2 - y1))
        lines.append([x1 + a, y1 + c, x2 - b, y2 - d])
    lines = np.trunc(np.array(lines)).astype(np.float64)
    return polys.astype(np.float64), logi, lines


@pytest.mark.parametrize("seed", range(8))
def test_key_rule_equals_sorted_match_on_permuted_tables(seed):
    polys, logi, lines = _seeded_table(seed)
    want = sorted_match_to_rows(polys, logi, lines)
    got = key_rule(polys, logi, lines)
    assert got.tolist() == want.tolist()
    _, order = table_cells_from_logits(polys, logi, return_order=True)
    assert list(order) != sorted(order)                                  # the sort does move cells


def test_page_table_html_with_matched_equals_host_route(golden_dir):
    for g, polys, logi, boxes, texts in _golden_cases(golden_dir):
        tb = M.text_boxes(boxes)
        inside = M.texts_in_table(g["bbox"], tb, diff=2)
        rows = key_rule(polys, logi, tb[inside])
        want = M.page_table_html(polys, logi, g["bbox"], boxes, texts, post_process=g["ocr_post_process"])
        assert want == (g["html"], g["db_html"])
        assert M.page_table_html(polys, logi, g["bbox"], boxes, texts, post_process=g["ocr_post_process"], matched=rows) == want
        assert M.page_table_html(polys, logi, g["bbox"], boxes, texts, post_process=g["ocr_post_process"], matched=rows,
                                 matched_lines=inside) == want


def test_page_table_html_refuses_a_map_of_the_wrong_size(golden_dir):
    g, polys, logi, boxes, texts = next(_golden_cases(golden_dir))
    with pytest.raises(ValueError):
        M.page_table_html(polys, logi, g["bbox"], boxes, texts, matched=np.zeros(1000, np.int64))
    with pytest.raises(ValueError):
        M.page_table_html(polys, logi, g["bbox"], boxes, texts, matched=np.array([len(polys)]), matched_lines=np.array([0]))


def test_attach_html_uses_the_stage_map_and_gives_nothing_for_an_empty_table(golden_dir):
    """_attach_html with the keys TsrStage.collect(match) attaches: the HTML of the host route for a table with cells, [] for a table
    whose count is 0 (empty maps, no scores)"""
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.tsr_stage import TsrStage
    pipe = OcrTablePipeline.__new__(OcrTablePipeline)
    pipe.table_html, pipe.device_match, pipe.table_structure_model = True, True, None
    pipe.table_structure_task = types.SimpleNamespace(_stage=TsrStage.__new__(TsrStage))
    g, polys, logi, boxes, texts = next(_golden_cases(golden_dir))
    boxes = np.asarray(boxes, np.float64).reshape(-1, 8)
    tb = M.text_boxes(boxes)
    inside = M.texts_in_table(g["bbox"], tb, diff=2)
    full = {"polygons": polys, "logi": logi, "scores": np.ones(len(polys), np.float32), "matched_lines": inside,
            "matched": key_rule(polys, logi, tb[inside])}
    empty = {"polygons": np.zeros((1, 8), np.float32), "logi": np.zeros((1, 4), np.float32), "scores": np.zeros(0, np.float32),
             "matched_lines": np.zeros(0, np.int64), "matched": np.zeros(0, np.int64)}
    tsr = [[full, empty]]
    pipe._attach_html(tsr, [np.array([g["bbox"], g["bbox"]])], [boxes], [texts])
    assert (full["table_html"], full["db_table_html"]) == M.page_table_html(polys, logi, g["bbox"], boxes, texts)
    assert empty["table_html"] == [] and empty["db_table_html"] == []
    # the knob is on but the stage gave no map: an error, not the host route in silence
    del full["matched"], full["matched_lines"]
    with pytest.raises(RuntimeError):
        pipe._attach_html(tsr, [np.array([g["bbox"], g["bbox"]])], [boxes], [texts])
