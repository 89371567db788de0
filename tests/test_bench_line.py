"""The ONE stdout line of bench.py stays small enough for the driver to parse (a 20.8 KB line came back `parsed: null`), and
--dump-outputs writes what the timed path returned (no GPU: the writer on hand-made results; tests/test_gpu_bench_dump.py runs it for real)."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def test_stub_line_is_one_small_json_line(tmp_path):
    detail = tmp_path / "detail.json"
    env = dict(os.environ, PT_BENCH_STUB="1")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1", "--detail-out", str(detail)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    assert len(lines[0]) < 8000
    d = json.loads(lines[0])
    for k in CONTRACT:
        assert k in d, k
    assert isinstance(d["config"]["workload"], str) and "model" not in d["config"]
    assert d["steps"] == 2 and d["warmup"] == 1
    full = json.loads(detail.read_text())
    assert full["value"] == d["value"] or abs(full["value"] - d["value"]) < 1e-3 * d["value"]


def test_compact_projection_of_a_full_record_fits():
    """The largest record the bench has produced (round 5: every leg, 20.8 KB) projects to < 6 KB and keeps roofline + cpu_baseline + summary."""
    sys.path.insert(0, REPO)
    import bench
    with open(os.path.join(REPO, "profiles", "r05", "bench_four_stages_final.json")) as f:
        rec = json.load(f)
    line = json.dumps(bench.compact_line(rec), separators=(",", ":"))
    assert len(line) < bench.LINE_LIMIT <= 6000
    d = json.loads(line)
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "launches", "avg_launch_ms"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "frac" in r["det_backbone"] and "frac" in r["det_backbone"]["net_only"]
    assert "conv3x3 implicit GEMM" in r["by_class"]["classes"]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample", "config0", "parity_sample"):
        assert k in c, k
    assert d["summary"]["pages_per_s_bf16"] == round(rec["value"], 1)


def _page(n_boxes, texts, layout, tables):
    from types import SimpleNamespace
    boxes = np.arange(n_boxes * 8, dtype=np.int32).reshape(n_boxes, 8)
    ocr = [{"index": j + 1, "text": t, "bbox": boxes[j].reshape(4, 2).astype(np.float32)} for j, t in enumerate(texts)]
    return SimpleNamespace(det_result=boxes, ocr_result=ocr, layout_result=layout, table_structure_result=tables)


def _table(n):
    if n == 0:      # TsrStage.collect()'s empty table: one zero quad, no scores
        return {"polygons": np.zeros((1, 8), np.float32), "logi": np.zeros((1, 4), np.float32), "logic_axis": np.zeros((1, 4), np.float32),
                "stacked_axis": np.zeros((1, 4), np.float32), "scores": np.zeros((0,), np.float32)}
    return {"polygons": np.full((n, 8), 1.25, np.float32), "logi": np.ones((n, 4), np.float32), "logic_axis": np.ones((n, 4), np.float32),
            "stacked_axis": np.ones((n, 4), np.float32), "scores": np.linspace(0.5, 0.9, n).astype(np.float32)}


def test_dump_outputs_writes_the_callers_arrays(tmp_path):
    """--dump-outputs: every field of the PageResults a predict_stream() caller receives, float64, pages concatenated with their counts"""
    sys.path.insert(0, REPO)
    import bench
    lay = [{"bbox": np.array([1.0, 2.0, 3.0, 4.0], np.float32), "label": "table", "score": np.float32(0.75), "category_id": 3}]
    res = [_page(3, ["ab", "", "éx"], lay, [_table(5), _table(0)]), _page(0, [], [], [])]
    info = bench.dump_outputs(str(tmp_path / "out"), res, [7, 8])
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert info["files"] == len(got) and info["pages"] == 2 and info["bytes"] <= bench.DUMP_LIMIT
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["page_ids"].tolist() == [7, 8]
    assert got["det_boxes"].shape == (3, 8) and got["det_boxes"].ravel().tolist() == list(range(24)) and got["det_boxes_per_page"].tolist() == [3, 0]
    assert got["rec_lines_per_page"].tolist() == [3, 0] and got["rec_text_lengths"].tolist() == [2, 0, 2]
    assert "".join(map(chr, got["rec_codepoints"].astype(int))) == "abéx" and np.array_equal(got["rec_bbox"], got["det_boxes"])
    assert got["layout_bbox"].tolist() == [[1, 2, 3, 4]] and got["layout_score"].tolist() == [0.75] and got["layout_category_id"].tolist() == [3]
    assert got["layout_regions_per_page"].tolist() == [1, 0] and got["tables_per_page"].tolist() == [2, 0]
    assert got["table_polygons"].shape == (6, 8) and got["table_polygons_rows"].tolist() == [5, 1]
    assert got["table_scores"].shape == (5,) and got["table_scores_rows"].tolist() == [5, 0]


def test_dump_outputs_keeps_a_seeded_sample_under_the_limit(monkeypatch):
    sys.path.insert(0, REPO)
    import bench
    res = [_page(100 + i, [], None, None) for i in range(16)]
    full = bench.output_arrays(res, list(range(16)))
    assert full["page_ids"].tolist() == list(range(16))
    monkeypatch.setattr(bench, "DUMP_LIMIT", sum(a.nbytes for a in full.values()) // 3)
    a, b = bench.output_arrays(res, list(range(16))), bench.output_arrays(res, list(range(16)))
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT
    assert 0 < len(a["page_ids"]) < 16 and a["page_ids"].tolist() == b["page_ids"].tolist()
    assert a["det_boxes_per_page"].tolist() == [100 + i for i in a["page_ids"].astype(int)]


def test_stub_refuses_dump_outputs(tmp_path):
    """the stub runner computes nothing: --dump-outputs is an error there, not an empty directory"""
    env = dict(os.environ, PT_BENCH_STUB="1")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "1", "--warmup", "0", "--detail-out", str(tmp_path / "d.json"),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode != 0 and "--dump-outputs" in p.stderr
    assert not (tmp_path / "out").exists()


def test_legs_all_needs_full(tmp_path):
    """the side legs are legs of a --full run: `--legs all` alone is refused, `--full --legs all` runs (stub runner: no legs to run)"""
    env = dict(os.environ, PT_BENCH_STUB="1")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "1", "--warmup", "0", "--detail-out", str(tmp_path / "d.json"), "--legs", "all"]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode != 0 and "--full" in p.stderr and not p.stdout.strip()
    p = subprocess.run(cmd + ["--full"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0])["steps"] == 1
