"""score_mode="slow" without a GPU: the row rule pt_op_det_poly_scores evaluates (tests/db_slow_ref.py) against oracle.db_post.fill_poly_mask on
seeded polygons, the host entry point that carries the contours (pt_db_contour_candidates_batch) against pt_db_candidates_batch and the oracle's
tracer, the knob's refusals, and the header / build / binding."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import db_slow_ref as R  # noqa: E402
from oracle import db_post as O  # noqa: E402
from pdf_table_amd import engine as E  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.det_stage import DetConfig  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def built():
    from pdf_table_amd.build import build
    build(verbose=False)


# ---- the row rule ------------------------------------------------------------------------------------------------------------------------------
def test_row_rule_equals_fill_poly_mask_on_seeded_polygons():
    """4200 polygons of 1 .. 13 vertices in masks up to 23 x 23, a third of them with vertices outside the map: the same rectangle, the same mask,
    and no row with an odd number of crossings (the rule pairs them without sorting)"""
    rng = np.random.RandomState(0)
    outside = 0
    for t in range(4200):
        k, h, w = rng.randint(1, 14), rng.randint(1, 24), rng.randint(1, 24)
        if t % 3 == 0:
            pts = np.stack([rng.randint(-6, w + 6, k), rng.randint(-6, h + 6, k)], 1)
            outside += int((pts[:, 0] < 0).any() or (pts[:, 0] >= w).any() or (pts[:, 1] < 0).any() or (pts[:, 1] >= h).any())
        else:
            pts = np.stack([rng.randint(0, w, k), rng.randint(0, h, k)], 1)
        want, rect = R.slow_mask(pts, h, w)
        got, rect2 = R.row_rule_mask(pts, h, w)
        assert rect == rect2 and np.array_equal(want, got), (pts.tolist(), h, w)
        assert not any(c & 1 for c in R.crossings_per_row(pts, h, w)), pts.tolist()
    assert outside > 1000


@pytest.mark.parametrize("dx,dy", [(7, 0), (0, 7), (7, 7), (8, 4), (9, 3), (10, 4), (4, 8), (3, 9), (5, 10), (1, 2), (2, 1), (13, 1), (1, 13)])
def test_outline_interval_is_the_line_iterator_in_all_eight_directions(dx, dy):
    """every row of every line against oracle.db_post._line_pixels, the exact halves among them (8 x 4: the minor step falls on j + 1/2)"""
    for sx in (1, -1):
        for sy in (1, -1):
            ax, ay, bx, by = 20, 20, 20 + sx * dx, 20 + sy * dy
            px = O._line_pixels(ax, ay, bx, by)
            for y in range(0, 41):
                xs = sorted(x for x, yy in px if yy == y)
                iv = R.outline_interval(ax, ay, bx, by, y)
                assert (list(range(iv[0], iv[1] + 1)) if iv else []) == xs, (ax, ay, bx, by, y)


def test_box_score_slow_on_a_known_mask():
    """an L: the polygon's mean is the arm's value, the rectangle's mean is mostly background"""
    prob = np.full((R.H, R.W), 0.25, np.float32)
    prob[10:16, 10:50] = 0.75
    prob[10:50, 10:16] = 0.75
    (c,) = R.kept_contours(prob > 0.5)
    s, cnt = R.box_score_slow(prob, c)
    assert cnt == 6 * 40 + 34 * 6 and s == 0.75 * cnt and R.score(s, cnt) == np.float32(0.75)
    assert R.box_score_slow(prob, c, mask_fn=R.row_rule_mask) == (s, cnt)


# ---- the host entry point ----------------------------------------------------------------------------------------------------------------------
def _reference(pages, max_candidates, min_size):
    return [R.kept_contours(bm, max_candidates, min_size) for bm in pages]


@pytest.mark.parametrize("max_candidates,min_size", [(1000, 3.0), (1000, 0.0), (3, 0.0)])
@pytest.mark.parametrize("threads", [1, 4])
def test_contour_candidates_equal_the_plain_call_and_the_oracle_tracer(max_candidates, min_size, threads):
    pages = R.shape_pages(0)
    words = R.pack_bits(pages)
    boxes0, counts0 = E.db_candidates_batch(words, max_candidates, min_size, threads)
    boxes, counts, pts, offs = E.db_contour_candidates_batch(words, max_candidates, min_size, threads)
    assert np.array_equal(counts, counts0) and counts[0] == 0 and counts[-1] == 0
    for i in range(len(pages)):
        assert np.array_equal(boxes[i, :counts[i]].view(np.uint32), boxes0[i, :counts0[i]].view(np.uint32))
    ref = _reference(pages, max_candidates, min_size)
    assert [len(r) for r in ref] == counts.tolist()
    if max_candidates == 3:      # the cut comes BEFORE the min_size test and bites: the pages have more contours than that
        assert all(len(O.find_contours(bm)) > 3 for bm in pages[1:5])
    flat = [c for r in ref for c in r]                                     # page-major, candidate order
    assert offs.shape == (len(flat) + 1,) and offs[0] == 0 and pts.dtype == np.int32 and offs.dtype == np.int32
    assert np.array_equal(np.diff(offs), [len(c) for c in flat])
    assert pts.shape == (int(offs[-1]), 2)
    for j, c in enumerate(flat):
        assert np.array_equal(pts[offs[j]:offs[j + 1]], c), j
    if min_size == 0.0 and max_candidates == 1000:
        lens = sorted(len(c) for c in flat)
        assert lens[-1] > 100 and len(ref[3]) > 100                        # the checkerboard: one long outer contour and a hole contour per gap
        hole = [c for c in ref[2] if len(c) == 8 and c[:, 0].min() == 14 and c[:, 0].max() == 33]      # the ring's hole contour: on the ring's pixels, corners cut
        assert len(hole) == 1
        diag = [c for c in ref[2] if len(c) == 2 and abs(int(c[0, 0]) - int(c[1, 0])) == 21]           # the diagonal: its two ends
        assert len(diag) == 1


def test_a_point_buffer_that_is_too_small_is_grown_and_nothing_is_written_past_it():
    pages = R.shape_pages(1)
    words = R.pack_bits(pages)
    want = E.db_contour_candidates_batch(words, 1000, 0.0, 2)
    total = want[2].shape[0]
    assert total > 64
    # the library alone: capacity 16, a canary behind it
    raw = np.full((total + 8, 2), -7, np.int32)
    boxes = np.empty((len(pages), 1000, 8), np.float32)
    counts = np.zeros(len(pages), np.int32)
    offs = np.zeros(len(pages) * 1000 + 1, np.int32)
    import ctypes as C
    need = C.c_longlong()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(L.load().pt_db_contour_candidates_batch(vp(words), len(pages), R.H, R.W, 1000, 0.0, 2, vp(boxes), None, 1000, vp(counts), vp(raw), 16, vp(offs),
                                                    C.byref(need)), "pt_db_contour_candidates_batch")
    assert need.value == total and (raw == -7).all()
    assert np.array_equal(counts, want[1]) and np.array_equal(offs[:int(counts.sum()) + 1], want[3])
    # exactly enough: written, and not a word more
    L.check(L.load().pt_db_contour_candidates_batch(vp(words), len(pages), R.H, R.W, 1000, 0.0, 2, vp(boxes), None, 1000, vp(counts), vp(raw), total, vp(offs),
                                                    C.byref(need)), "pt_db_contour_candidates_batch")
    assert np.array_equal(raw[:total], want[2]) and (raw[total:] == -7).all()
    # the wrapper: one retry, through the caller's allocator, with the size the library asked for
    asked = []

    def alloc(k):
        asked.append(k)
        return np.full((k, 2), -7, np.int32)
    got = E.db_contour_candidates_batch(words, 1000, 0.0, 2, points=np.full((16, 2), -7, np.int32), alloc=alloc)
    assert asked == [total]
    assert all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    assert all(np.array_equal(got[0][i, :n], want[0][i, :n]) for i, n in enumerate(want[1]))      # rows behind a page's count are not written
    with pytest.raises(ValueError, match="int32"):
        E.db_contour_candidates_batch(words, 1000, 0.0, 2, points=np.zeros((16, 2), np.int64))


def test_contour_candidates_refuses_bad_arguments():
    words = R.pack_bits(R.shape_pages(0))
    import ctypes as C
    need = C.c_longlong()
    with pytest.raises(L.PtError, match="pt_db_contour_candidates_batch"):
        L.check(L.load().pt_db_contour_candidates_batch(words.ctypes.data_as(C.c_void_p), 6, R.H, R.W, 1000, 3.0, 1, None, None, 1000, None, None, 0, None,
                                                        C.byref(need)), "pt_db_contour_candidates_batch")


# ---- the knob --------------------------------------------------------------------------------------------------------------------------------
def test_det_config_score_mode():
    assert DetConfig().score_mode == "fast" and DetConfig(score_mode="slow").resolved().score_mode == "slow"
    assert DetConfig(flavour="db").resolved().score_mode == "fast"
    with pytest.raises(ValueError, match="'fast' and 'slow'"):
        DetConfig(score_mode="bogus")
    with pytest.raises(ValueError, match="torch flavour"):
        DetConfig(flavour="db", score_mode="slow")
    cfg = DetConfig(flavour="db")
    cfg.score_mode = "slow"          # set behind the constructor's back: refused where DetStage resolves the flavour, not reset to "fast"
    with pytest.raises(ValueError, match="torch flavour"):
        cfg.resolved()
    cfg = DetConfig()
    cfg.score_mode = "Slow"
    with pytest.raises(ValueError, match="'fast' and 'slow'"):
        cfg.resolved()


def test_abi_unchanged_and_entry_points_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pdftable_hip.h")).read()
    assert L.EXPECTED_ABI == 21
    assert re.search(r"\bint pt_op_det_poly_scores\(", hdr) and re.search(r"\bint pt_db_contour_candidates_batch\(", hdr)
    from pdf_table_amd import build as B
    names = {name for _, name, _ in B._prototypes()}
    assert "det_poly_score.hip" in B.ONCE_HIP_SOURCES and {"pt_op_det_poly_scores", "pt_db_contour_candidates_batch"} <= names
    # both are exported by the generated dispatcher (the work of the host one is a plain C++ function in db_post.cpp), and bound by name
    src = B.dispatch_source()
    assert "pt_bf16::api::pt_db_contour_candidates_batch(" in src and "pt_bf16::api::pt_op_det_poly_scores(" in src
    post = open(os.path.join(root, "pdf_table_amd", "csrc", "db_post.cpp")).read()
    assert not re.search(r"^int pt_db_contour_candidates_batch\(", post, flags=re.M) and re.search(r"^int db_contour_candidates_batch\(", post, flags=re.M)
    lib = L.load()
    assert {"pt_op_det_poly_scores", "pt_db_contour_candidates_batch"} <= set(L.EXPORTS) and lib.pt_abi_version() == 21
    # the constants the binding repeats
    for name in ("PT_DET_POLY_MAX_W", "PT_DET_POLY_BANDS"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(L, name)
    assert L.PT_DET_POLY_MAX_W >= 4096 and L.PT_DET_POLY_WORK_BYTES == 12 * L.PT_DET_POLY_BANDS
