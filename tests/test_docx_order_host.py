"""device_order without a GPU: the Python restatement of the sort replay (tests/docx_order_ref.py, the kernel's specification) against ``sorted`` of
the running interpreter, the stability checker on an axis-aligned and on a crafted borderline page, the knob's refusals."""
import math
import os
import random
import sys
from functools import cmp_to_key

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docx_order_ref as O  # noqa: E402
from pdf_table_amd.docxlayout_stage import DocXLayoutConfig, _compare_rects, docx_page_result, sort_blocks  # noqa: E402

SIZES = (0, 1, 2, 3, 17, 62, 63)


def _replayed(items, cmp):
    return [items[i] for i in O.replay_sort(len(items), lambda i, j: cmp(items[i], items[j]) < 0)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_replay_equals_the_interpreter_with_an_inconsistent_comparator(n, seed):
    """a random table of -1 / 0 / 1: not antisymmetric, not transitive -- the result is defined by the comparisons list.sort makes, nothing else"""
    rng = random.Random(1000 * seed + n)
    table = [[rng.choice((-1, 0, 1)) for _ in range(n)] for _ in range(n)]
    items = list(range(n))
    rng.shuffle(items)
    cmp = lambda x, y: table[x][y]
    assert _replayed(items, cmp) == sorted(items, key=cmp_to_key(cmp))


@pytest.mark.parametrize("n", SIZES)
def test_replay_descending_equal_and_partly_ordered_inputs(n):
    num = lambda x, y: (x > y) - (x < y)
    desc = list(range(n, 0, -1))                      # the strictly descending run, reversed in place
    assert _replayed(desc, num) == sorted(desc, key=cmp_to_key(num)) == list(range(1, n + 1))
    same = [(7, k) for k in range(n)]                 # all equal: the order stays (tags tell the elements apart)
    by_first = lambda x, y: num(x[0], y[0])
    assert _replayed(same, by_first) == sorted(same, key=cmp_to_key(by_first)) == same
    rng = random.Random(n)
    mixed = [(rng.randrange(5), k) for k in range(n)]  # many ties behind a short run
    assert _replayed(mixed, by_first) == sorted(mixed, key=cmp_to_key(by_first))
    head = list(range(n // 2, 0, -1)) + [rng.randrange(n) for _ in range(n - n // 2)]      # a descending run, then anything
    assert _replayed(head, num) == sorted(head, key=cmp_to_key(num))


def _blk(name, x0, y0, x1, y1):
    return {"name": name, "pts": [float(v) for v in (x0, y0, x1, y0, x1, y1, x0, y1)]}


def _cycle():
    """the three blocks of test_docxlayout_host.test_sort_with_a_comparison_cycle: t < u < l < t"""
    return _blk("t", 0, 0, 10, 30), _blk("u", 12, 0, 22, 10), _blk("l", -12, 18, -2, 28)


def test_replay_on_the_comparison_cycle_in_its_three_orders():
    tall, up_right, low_left = _cycle()
    rect = lambda p: (p["pts"][0], p["pts"][1], p["pts"][2] - p["pts"][0], p["pts"][5] - p["pts"][1])
    cmp = lambda p, q: _compare_rects(rect(p), rect(q))
    assert cmp(tall, up_right) == -1 and cmp(up_right, low_left) == -1 and cmp(low_left, tall) == -1
    firsts = set()
    for order in ([tall, up_right, low_left], [low_left, tall, up_right], [up_right, low_left, tall]):
        want = [p["name"] for p in sorted(order, key=cmp_to_key(cmp))]
        assert [p["name"] for p in _replayed(order, cmp)] == want
        mine, theirs = [dict(p) for p in order], [dict(p) for p in order]
        O.sort_blocks_replayed(mine)
        sort_blocks(theirs)
        assert [p["name"] for p in mine] == [p["name"] for p in theirs] == want
        firsts.add(want[0])
    assert len(firsts) > 1


def test_replay_refuses_64():
    with pytest.raises(AssertionError):
        O.replay_sort(64, lambda i, j: i < j)


def _axis_page(seed, n=24, nf=3):
    rng = np.random.RandomState(seed)
    lay = []
    for k in range(n):
        x0, y0 = int(rng.randint(0, 500)), int(rng.randint(0, 700))
        lay.append(_blk(f"r{k}", x0, y0, x0 + int(rng.randint(5, 200)), y0 + int(rng.randint(5, 80))))
    sub = [_blk(f"f{k}", 10 + 200 * k, 0, 190 + 200 * k, 800) for k in range(nf)]
    return lay, sub


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_stability_checker_accepts_an_axis_aligned_page(seed):
    """every main angle is exactly 0: sin 0, cos 1 on both sides, nothing to perturb -- also where blocks touch or share an edge"""
    lay, sub = _axis_page(seed)
    lay += [_blk("touch_a", 0, 900, 50, 910), _blk("touch_b", 50, 900, 90, 910), _blk("touch_c", 0, 910, 50, 920)]
    assert O.blocks_are_stable(lay, sub)
    got = [it["name"] for it in O.reading_order(lay, sub)]
    import pdf_table_amd.docxlayout_stage as DS
    assert got == [it["name"] for it in DS._reading_order([dict(it) for it in lay], [dict(it) for it in sub])]


def _turned(theta, x0, y0, x1, y1):
    """the frame rectangle (x0, y0) .. (x1, y1) turned by theta into page coordinates, vertex order as a block's"""
    c, s = math.cos(theta), math.sin(theta)
    return [v for fx, fy in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)) for v in (fx * c - fy * s, fx * s + fy * c)]


def _frame_rect(pts, ang):
    sn, cs = math.sin(ang), math.cos(ang)
    xs = [pts[k] * cs + pts[k + 1] * sn for k in range(0, 8, 2)]
    ys = [pts[k + 1] * cs - pts[k] * sn for k in range(0, 8, 2)]
    return (min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys))


def test_stability_checker_refuses_a_borderline_page():
    """a sliver (1.5e-4 high, right of a tall block) whose lower edge meets the tall block's upper edge + 1e-4 within 1e-14 in the turned frame:
    "before" (-1) on one side of the rule, "overlapping, after in x, near = 0.67" (+1) on the other -- a last-bit change of sin flips the order"""
    import pdf_table_amd.docxlayout_stage as DS
    theta = math.atan2(1.0, 8.0)
    tall = {"name": "tall", "pts": _turned(theta, 0.0, 2.0, 2.0, 8.0)}

    def sliver(d):
        return {"name": "sliver", "pts": _turned(theta, 6.0, d, 12.0, d + 1.5e-4)}

    def gap(d):      # hi_a - (lo_b + 1e-4) for a = sliver, b = tall, as _relation sees it
        ang = DS._main_angle([sliver(d)["pts"], tall["pts"]])
        ra, rb = _frame_rect(sliver(d)["pts"], ang), _frame_rect(tall["pts"], ang)
        return (ra[1] + ra[3]) - (rb[1] + 1e-4)

    lo, hi = 2.0 - 1.5e-4, 2.0      # gap(lo) < 0 < gap(hi)
    assert gap(lo) < 0 < gap(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        lo, hi = (mid, hi) if gap(mid) < 0 else (lo, mid)
    d = hi
    assert abs(gap(d)) <= 1e-14, gap(d)
    assert DS._main_angle([sliver(d)["pts"], tall["pts"]]) != 0
    assert not O.blocks_are_stable([sliver(d), tall], [])
    # the same two blocks a hair apart are stable again
    assert O.blocks_are_stable([sliver(d + 1e-3), tall], []) and O.blocks_are_stable([sliver(d - 1e-3), tall], [])


def test_page_rows_is_the_host_chain():
    """page_rows (what the kernel is compared against) and docx_page_result build the same list"""
    rng = np.random.RandomState(5)
    main = np.zeros((30, 12), np.float32)
    for k in range(30):
        x0, y0, w, h = rng.uniform(0, 30), rng.uniform(0, 40), rng.uniform(1, 8), rng.uniform(1, 5)
        main[k, :8] = (x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h)
        main[k, 8], main[k, 9] = rng.uniform(0.2, 0.95), rng.randint(0, 11)
    sub = np.zeros((2, 12), np.float32)
    sub[0, :8], sub[1, :8] = (0, 0, 20, 0, 20, 48, 0, 48), (20, 0, 40, 0, 40, 48, 20, 48)
    sub[:, 8], sub[:, 9] = 0.8, (0, 1)
    cfg = DocXLayoutConfig()
    rows = O.page_rows(main, sub, (768, 640), (48, 40), cfg)
    want = docx_page_result(main, sub, (768, 640), (48, 40), cfg)
    assert len(rows) == len(want) > 10
    for r, w in zip(rows, want):
        assert [float(v) for v in r[:4]] == [float(v) for v in w["bbox"]] and int(r[5]) == w["category_id"]
        assert float("{:.2f}".format(r[4])) == w["score"]


def test_knob_refusals():
    """before an engine exists: needs no GPU.  The old knobs' refusals are unchanged"""
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    from pdf_table_amd.pipeline import OcrTablePipeline
    with pytest.raises(ValueError, match="layout_device_order"):
        OcrTablePipeline(synthetic_seed=0, layout=True, layout_device_order=True)                      # PicoDet
    with pytest.raises(ValueError, match="layout_device_order"):
        OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="picodet", layout_task_type="ch", layout_device_order=True)
    with pytest.raises(ValueError, match="layout=False"):
        OcrTablePipeline(synthetic_seed=0, layout=False, layout_model="DocXLayout", layout_task_path="/nowhere", layout_device_order=True)
    with pytest.raises(ValueError, match="device_order"):
        OcrLayoutTask(model="picodet", synthetic_seed=0, device_order=True)
    # the knob does not lift the model's own refusals
    with pytest.raises(ValueError, match="layout_task_path"):
        OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_device_order=True)
    with pytest.raises(RuntimeError, match="task_path"):
        OcrLayoutTask(model="DocXLayout", device_order=True)
    # device_decode / layout_device_decode stay PicoDet's and still raise for this model, with and without the new knob
    for extra in ({}, {"layout_device_order": True}):
        with pytest.raises(ValueError, match="layout_device_decode"):
            OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path="/nowhere", layout_device_decode=True, **extra)
    for extra in ({}, {"device_order": True}):
        with pytest.raises(ValueError, match="device_decode"):
            OcrLayoutTask(model="DocXLayout", task_path="/nowhere", device_decode=True, **extra)
    with pytest.raises(ValueError, match="layout_device_decode"):
        OcrTablePipeline(synthetic_seed=0, layout=False, layout_device_decode=True)


def test_abi_unchanged_and_entry_point_declared():
    import re
    from pdf_table_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pdftable_hip.h")).read()
    assert L.EXPECTED_ABI == 21 and re.search(r"\bint pt_op_docx_order\(", hdr)
    from pdf_table_amd import build as B
    assert "docx_order.hip" in B.ONCE_HIP_SOURCES and "pt_op_docx_order" in {name for _, name, _ in B._prototypes()}
