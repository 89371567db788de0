"""bench.py --dump-outputs on the GPU: a short run of the real four-stage step writes the last timed step's results, and the JSON line's
`steps` / `ms_per_step` are those of the timed region."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs(tmp_path):
    out = tmp_path / "out"
    env = dict(os.environ, PT_BENCH_PAGES="4", PT_BENCH_SPINUP="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "PT_BENCH_STUB", "PT_BENCH_DISTINCT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "3", "--warmup", "2", "--no-extra-legs", "--no-cpu-baseline",
                        "--detail-out", str(tmp_path / "detail.json"), "--dump-outputs", str(out)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2
    assert abs(d["value"] * d["ms_per_step"] - 4 * 1e3) < 1e-6 * 4e3          # 4 pages per step: pages/s x ms/step
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["page_ids"].tolist() == [0, 1, 2, 3]
    assert got["det_boxes_per_page"].sum() == len(got["det_boxes"]) > 20
    assert got["rec_lines_per_page"].sum() == len(got["rec_text_lengths"]) == len(got["rec_bbox"])
    assert got["rec_text_lengths"].sum() == len(got["rec_codepoints"]) > 0
    assert got["layout_regions_per_page"].sum() == len(got["layout_bbox"]) == len(got["layout_score"])
    assert got["tables_per_page"].sum() == len(got["table_polygons_rows"]) > 0
    assert got["table_polygons_rows"].sum() == len(got["table_polygons"]) and got["table_scores_rows"].sum() == len(got["table_scores"]) > 0


def test_bench_plain_run_stops_after_the_timed_steps(tmp_path):
    """without --full nothing runs after the timed steps: the record holds the headline and the timed region's roofline, no leg and no CPU baseline"""
    env = dict(os.environ, PT_BENCH_PAGES="4", PT_BENCH_SPINUP="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "PT_BENCH_STUB", "PT_BENCH_DISTINCT"):
        env.pop(k, None)
    detail = tmp_path / "detail.json"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1", "--detail-out", str(detail)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    full = json.loads(detail.read_text())
    assert full["roofline"]["launches"] > 0
    assert not {"det_backbone", "by_class"} & set(full["roofline"])
    assert not {"host_pages", "tolerance_mode", "cpu_baseline", "one_eighth_host"} & set(full)
