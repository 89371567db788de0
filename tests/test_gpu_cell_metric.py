"""WtwMetric(engine=HipEngine(0)) against WtwMetric(): the device route equals the host route field for field -- match as integers, the counts, and the
quotients, which both routes form on the host from the same integers -- on seeded pairs of 1 .. 600 cells under a budget that keeps them in one chunk
and one that forces several; a 4097-cell table goes to the host route and is listed in last_fallback; and the Lore tables of two seeded pages in bf16
are scored against the same pages' fp32 tables on both routes and through files (figures printed, not asserted: they describe seeded weights)."""
import math
import os

import numpy as np
import pytest

from pdf_table_amd import cell_metric as M
from pdf_table_amd.cell_metric import WtwMetric
from pdf_table_amd.cell_metric_synth import sized_pair, table_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    return HipEngine(0)


def equal_results(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y) == {"precision", "recall", "fp", "fn", "acc", "tp", "truep", "match"}
        assert x["match"].dtype == y["match"].dtype == np.int64 and np.array_equal(x["match"], y["match"]), k
        for f in ("precision", "recall", "fp", "fn", "acc", "tp", "truep"):
            assert type(x[f]) is type(y[f]) and x[f] == y[f], (k, f, x[f], y[f])


@pytest.fixture(scope="module")
def seeded():
    """about 40 pairs of 1 .. 600 cells, some with an empty side, and the host route's answers, computed once"""
    rng = np.random.default_rng(23)
    sizes = [1, 2, 600, 599] + [int(v) for v in rng.integers(3, 600, 32)]
    pairs = [table_pair(900 + k, n, jitter=5.0) for k, n in enumerate(sizes)]
    pairs += [sized_pair(1, 0, 7), sized_pair(2, 9, 0), sized_pair(3, 0, 0), sized_pair(4, 40, 300), sized_pair(5, 300, 40)]
    return pairs, WtwMetric().batch_evaluate(pairs)


@pytest.mark.parametrize("budget,chunks", [(1 << 28, 1), (60000, None)])
def test_device_route_equals_host_route(eng, seeded, budget, chunks):
    pairs, want = seeded
    dev = WtwMetric(engine=eng, scratch_budget=budget)
    dev.events = []
    got = dev.batch_evaluate(pairs)
    equal_results(got, want)
    assert dev.last_fallback == []
    if chunks:
        assert len(dev.events) == chunks
    else:
        assert len(dev.events) >= 8                                       # 60 KB: a pair of 600 cells is a chunk of its own
    s_dev, s_host = WtwMetric.summarize(got), WtwMetric.summarize(want)
    assert all(s_dev[k] == s_host[k] or (math.isnan(s_dev[k]) and math.isnan(s_host[k])) for k in M.METRIC_KEYS)
    assert 0.5 < s_host["acc"] < 1.0 and 0.5 < s_host["det_recall"] < 1.0 and s_host["total"] == len(pairs)
    one = dev.evaluate(*pairs[2])
    equal_results([one], [want[2]])
    other = WtwMetric(engine=eng, iou_threshold=0.8).batch_evaluate(pairs[:6])
    equal_results(other, WtwMetric(iou_threshold=0.8).batch_evaluate(pairs[:6]))
    assert sum(r["tp"] for r in other) < sum(r["tp"] for r in want[:6])


def test_oversized_table_falls_back_to_the_host(eng):
    pairs = [sized_pair(11, 50, 60), sized_pair(12, 4097, 30), sized_pair(13, 30, 4097), sized_pair(14, 4096, 20)]
    dev = WtwMetric(engine=eng)
    dev.events = []
    got = dev.batch_evaluate(pairs)
    assert dev.last_fallback == [1, 2] and len(dev.events) == 1
    equal_results(got, WtwMetric().batch_evaluate(pairs))
    with pytest.raises(ValueError, match="non-finite"):
        bad = (pairs[0][0][0].copy(), pairs[0][0][1])
        bad[0][3, 4] = np.inf
        dev.evaluate(bad, pairs[0][1])


def test_bf16_tables_scored_against_fp32_tables(eng, tmp_path):
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_pages import make_page
    pages, boxes = [], []
    for seed in (2, 3):
        page, meta = make_page(seed)
        pages.append(page)
        boxes.append(meta["tables"].reshape(-1, 4))
    tables = {}
    for precision in ("fp32", "bf16"):
        pipe = OcrTablePipeline(device=0, synthetic_seed=0, table_structure=True, precision=precision)
        res = pipe.predict(pages, table_boxes=boxes)
        tables[precision] = [M.table_from_result(t) for r in res for t in r.table_structure_result]
    assert len(tables["fp32"]) == len(tables["bf16"]) == sum(len(b) for b in boxes) > 0
    pairs = list(zip(tables["bf16"], tables["fp32"]))
    host, dev = WtwMetric().batch_evaluate(pairs), WtwMetric(engine=eng).batch_evaluate(pairs)
    equal_results(dev, host)
    summary = WtwMetric.summarize(dev)
    print(f"bf16 Lore tables against fp32 tables, {len(pairs)} tables of {[len(t[0]) for t in tables['fp32']]} (fp32) / {[len(t[0]) for t in tables['bf16']]} "
          f"(bf16) cells: {M.wtw_result(summary)}")
    # through the files LoreProcessor.save_result writes: coordinates rounded to 5 decimals, so the tables are re-read before the comparison
    pred_dir, label_dir = str(tmp_path / "pred"), str(tmp_path / "label")
    for k, (p, g) in enumerate(pairs):
        M.save_table(p[0], p[1], os.path.join(pred_dir, "center", f"t{k}.txt"), os.path.join(pred_dir, "logi", f"t{k}.txt"))
        M.save_table(g[0], g[1], os.path.join(label_dir, "gt_center", f"t{k}.txt"), os.path.join(label_dir, "gt_logi", f"t{k}.txt"))
    by_dev = WtwMetric(engine=eng).evaluate_dirs(pred_dir, label_dir)
    by_host = WtwMetric().evaluate_dirs(pred_dir, label_dir)
    equal_results(by_dev["per_pair"], by_host["per_pair"])
    assert by_dev["error_list"] == by_host["error_list"] and by_dev["file_names"] == by_host["file_names"]
    assert all(by_dev["summary"][k] == by_host["summary"][k] or math.isnan(by_host["summary"][k]) for k in M.METRIC_KEYS)
    assert by_dev["summary"]["total"] + by_dev["summary"]["error_total"] == len(pairs)
    print(f"the same through center/ + logi/ files: {by_dev['result']}")
