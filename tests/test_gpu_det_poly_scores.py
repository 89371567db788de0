"""pt_op_det_poly_scores (csrc/det_poly_score.hip) alone, through HipEngine.op_det_poly_scores, against box_score_slow over the oracle's fillPoly
(tests/db_slow_ref.py) on maps of 64 x 96, three pages.  Counts are compared as integers.  On the map whose values are multiples of 2^-10 every double
sum is exact in any order, so sums and scores are compared with ==; on the random float32 map both sides add `count` non-negative terms in double, each
addition within 2^-53 relative, so |sum_dev - sum_ref| <= 2 count 2^-53 sum_ref, and the score must be float32(sum_dev / count) exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import db_slow_ref as R  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5A
PAD = 256
H, W, N = R.H, R.W, 3
# the kernel's tile sizes (csrc/det_poly_score.hip)
K_CHUNK = 64         # kPsChunk: pixels a wave scans at once, and edges a wave looks at at once
K_WAVES = 4          # kPsWaves: rows a workgroup has in flight
K_BAND_ROWS = 8      # kPsBandRows: a rectangle of at most this many rows is one band (one workgroup)
K_BANDS = L.PT_DET_POLY_BANDS      # bands of the tallest rectangle


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def maps():
    """(exact, random): float32 [3, 64, 96] -- multiples of 2^-10 in [0, 1], and uniform float32 in [0, 1]; host and device copies, made once"""
    rng = np.random.RandomState(7)
    exact = (rng.randint(0, 1025, (N, H, W)) / 1024.0).astype(np.float32)
    rnd = rng.uniform(0, 1, (N, H, W)).astype(np.float32)
    return {"exact": (exact, torch.from_numpy(exact).cuda()), "random": (rnd, torch.from_numpy(rnd).cuda())}


def launch(eng, prob_t, contours, pages, extra_points=0):
    """two calls on the same canary-filled buffers -> (scores f32, sums f64, counts i32); bytes behind every buffer intact, both calls the same bytes"""
    nb = len(contours)
    pts = np.concatenate([np.asarray(c, np.int32).reshape(-1, 2) for c in contours] + [np.full((extra_points, 2), 1 << 20, np.int32)])
    offs = np.concatenate([[0], np.cumsum([len(c) for c in contours])]).astype(np.int32)
    pg = np.asarray(pages, np.int32)
    sizes = (nb * 4, nb * 8, nb * 4, nb * L.PT_DET_POLY_WORK_BYTES)
    bufs = [torch.full((m + PAD,), CANARY, dtype=torch.uint8, device="cuda") for m in sizes]
    scores, sums, counts = bufs[0][:sizes[0]].view(torch.float32), bufs[1][:sizes[1]].view(torch.float64), bufs[2][:sizes[2]].view(torch.int32)
    dev = [torch.from_numpy(v).cuda() for v in (pts, offs, pg)]
    res = []
    for _ in range(2):
        eng.op_det_poly_scores(prob_t, *dev, offs, pg, sums=sums, counts=counts, scores=scores, work=bufs[3][:sizes[3]])
        torch.cuda.synchronize()
        res.append([b.cpu().numpy().copy() for b in bufs])
    for a, b in zip(*res):
        assert np.array_equal(a, b), "a second call on the same buffers changed bytes"
    for b, m in zip(res[0], sizes):
        assert (b[m:] == CANARY).all(), "bytes behind a buffer were written"
    return res[0][0][:sizes[0]].view(np.float32), res[0][1][:sizes[1]].view(np.float64), res[0][2][:sizes[2]].view(np.int32)


def check(eng, maps, contours, pages=None, which=("exact", "random"), hw=(H, W)):
    pages = [k % N for k in range(len(contours))] if pages is None else pages
    for name in which:
        prob, prob_t = maps[name]
        assert prob.shape[1:] == hw
        scores, sums, counts = launch(eng, prob_t, contours, pages)
        for j, (c, p) in enumerate(zip(contours, pages)):
            s, cnt = R.box_score_slow(prob[p], c)
            assert counts[j] == cnt, (name, j, int(counts[j]), cnt)
            if name == "exact":
                assert sums[j] == s, (name, j, float(sums[j]), s)
                assert scores[j] == R.score(s, cnt), (name, j)
            else:
                assert abs(sums[j] - s) <= 2 * cnt * 2.0 ** -53 * s, (name, j, float(sums[j]), s)
                assert scores[j] == (np.float32(sums[j] / cnt) if cnt else np.float32(0)), (name, j)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def star(k, cx=48, cy=32, r0=8, r1=28):
    """a polygon of exactly k vertices around (cx, cy), radius alternating: concave, edges in every direction"""
    a = np.arange(k) * 2 * np.pi / k
    r = np.where(np.arange(k) % 2 == 0, r1, r0)
    return np.stack([np.rint(cx + 1.5 * r * np.cos(a)), np.rint(cy + r * np.sin(a))], 1).astype(np.int32)


def comb(teeth, x0=8, top=20, base=50, bottom=55):
    v = [(x0, bottom), (x0, base)]
    for t in range(teeth):
        x = x0 + 2 * t
        v += [(x, top), (x + 1, top), (x + 1, base)]
        if t + 1 < teeth:
            v.append((x + 2, base))
    v += [(x0 + 2 * teeth - 1, bottom)]
    return v


def test_one_to_four_vertices(eng, maps):
    check(eng, maps, [[(17, 9)], [(0, 0)], [(W - 1, H - 1)],
                      [(10, 10), (18, 14)], [(10, 10), (14, 18)], [(30, 5), (30, 40)], [(5, 33), (90, 33)],
                      [(10, 10), (40, 12), (20, 50)], [(60, 60), (61, 20), (90, 58)],
                      [(10, 10), (50, 14), (45, 40), (8, 30)], rect(20, 20, 21, 21)])


def test_exact_bresenham_halves_and_fixed_point_halves(eng, maps):
    """x-major 8 x 4 and y-major 4 x 8 lines put every minor step on j + 1/2 (the half rule decides the pixel), in all four directions; a slope of
    1/2 puts the scan line's 16.16 crossing on a low half of exactly 0x8000 on every other row"""
    segs = []
    for sx in (1, -1):
        for sy in (1, -1):
            segs += [[(40, 30), (40 + 8 * sx, 30 + 4 * sy)], [(40, 30), (40 + 4 * sx, 30 + 8 * sy)], [(40, 30), (40 + 12 * sx, 30 + 4 * sy)]]
    half = [[(10, 10), (13, 16), (30, 16), (27, 10)], [(10, 10), (11, 12), (5, 12)], [(50, 5), (41, 23), (70, 23)], [(20, 40), (29, 58), (12, 58), (3, 40)]]
    for c in half:      # the crossing of the first edge one row below its top: low half 0x8000
        (ax, ay), (bx, by) = c[0], c[1]
        assert ((bx - ax) << 16) % (by - ay) == 0 and (((bx - ax) << 16) // (by - ay)) & 0xFFFF == 0x8000
    check(eng, maps, segs + half)


def test_u_comb_ring_hole_and_tracer_contours(eng, maps):
    u = [(10, 10), (15, 10), (15, 30), (35, 30), (35, 10), (40, 10), (40, 36), (10, 36)]
    c40 = comb(40)
    assert max(R.crossings_per_row(c40, H, W)) > 64
    traced = R.kept_contours(R.shape_pages(0)[2], 1000, 0.0)       # the diagonal (2 vertices, walked there and back), the plus sign, the ring's hole and its outside
    assert sorted(len(c) for c in traced) == [2, 4, 8, 16]
    chain = R.kept_contours(R.shape_pages(0)[3], 1000, 0.0)        # corner chain and checkerboard: vertices visited twice, hundreds of them
    long = [c for c in chain if len(c) > 100]
    assert len(long) == 1
    check(eng, maps, [u, c40] + traced + long + chain[:12])


def test_rectangle_sizes_and_the_kernel_tiles(eng, maps):
    cs = [rect(30, 5, 30, 50), rect(5, 30, 80, 30),                                                     # 1 wide, 1 high
          rect(0, 0, W - 1, H - 1),                                                                     # the full map
          [(48, 0), (W - 1, 32), (48, H - 1), (0, 32)],                                                 # touching all four borders
          [(-5, -5), (100, -3), (50, 70)], [(-20, 30), (120, 20), (130, 40)], [(200, 200), (210, 205), (190, 230)]]      # vertices outside the map
    for w in (K_CHUNK - 1, K_CHUNK, K_CHUNK + 1):                                                       # 63 / 64 / 65 wide
        cs += [rect(3, 10, 3 + w - 1, 20), [(3, 40), (3 + w - 1, 44), (3 + w - 1, 50), (3, 47)]]
    for h in (K_WAVES - 1, K_WAVES, K_WAVES + 1, K_BAND_ROWS - 1, K_BAND_ROWS, K_BAND_ROWS + 1, 2 * K_BAND_ROWS + 1):
        cs += [rect(70, 2, 90, 2 + h - 1), [(20, 2), (60, 2 + h - 1), (22, 2 + h - 1)]]
    for k in (K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK + 1):                                      # vertices: 63 / 64 / 65 / 129
        s = star(k)
        assert len(s) == k
        cs.append(s)
    check(eng, maps, cs)


def test_a_candidate_split_over_workgroups(eng, maps):
    """64 rows: 8 bands of 8; 57 rows: 8 bands of 8 with a last band of one row; 9 rows: two bands"""
    check(eng, maps, [star(33, r0=10, r1=31), rect(2, 0, 93, H - 1), [(5, 3), (90, 5), (70, 59), (10, 50)], rect(10, 10, 60, 18)])


def test_the_band_limit_on_a_tall_map(eng):
    """a 136 x 96 map: K_BANDS bands of K_BAND_ROWS rows minus one, exact, plus one row (127 / 128 / 129), and the full height"""
    rng = np.random.RandomState(11)
    hh = K_BANDS * K_BAND_ROWS + 8
    exact = (rng.randint(0, 1025, (1, hh, W)) / 1024.0).astype(np.float32)
    tall = {"exact": (exact, torch.from_numpy(exact).cuda())}
    cs = []
    for h in (K_BANDS * K_BAND_ROWS - 1, K_BANDS * K_BAND_ROWS, K_BANDS * K_BAND_ROWS + 1, hh):
        cs += [rect(4, 0, 90, h - 1), [(48, 0), (90, h // 2), (50, h - 1), (3, h // 3)]]
    check(eng, tall, cs, pages=[0] * len(cs), which=("exact",), hw=(hh, W))


def test_300_candidates_with_an_empty_page_in_the_middle(eng, maps):
    """pages 0 and 2 only, alternating: candidates of the first and the last page lie next to each other in the list"""
    rng = np.random.RandomState(3)
    cs, pages = [], []
    for j in range(300):
        k = rng.randint(1, 9)
        x0, y0 = rng.randint(0, W - 20), rng.randint(0, H - 12)
        cs.append(np.stack([x0 + rng.randint(0, 20, k), y0 + rng.randint(0, 12, k)], 1))
        pages.append(0 if j % 2 == 0 else 2)
    check(eng, maps, cs, pages=pages)


def test_points_the_offsets_do_not_name_are_not_read(eng, maps):
    """wild points behind the last offset, and a candidate without a vertex: count 0, score 0"""
    prob, prob_t = maps["exact"]
    cs = [rect(5, 5, 20, 9), np.zeros((0, 2), np.int32), [(40, 40), (60, 50), (45, 60)]]
    scores, sums, counts = launch(eng, prob_t, cs, [0, 1, 2], extra_points=5)
    assert counts[1] == 0 and sums[1] == 0 and scores[1] == 0
    for j in (0, 2):
        s, cnt = R.box_score_slow(prob[j], cs[j])
        assert (counts[j], sums[j], scores[j]) == (cnt, s, R.score(s, cnt))


def test_nb_zero_launches_nothing(eng, maps):
    _, prob_t = maps["exact"]
    z = torch.zeros((0,), dtype=torch.int32, device="cuda")
    out = eng.op_det_poly_scores(prob_t, z.view(0, 2), torch.zeros((1,), dtype=torch.int32, device="cuda"), z, np.zeros(1, np.int32), np.zeros(0, np.int32))
    torch.cuda.synchronize()
    assert out.shape == (0,)


def test_refusals_leave_the_outputs_untouched(eng, maps):
    _, prob_t = maps["exact"]
    pts = torch.from_numpy(np.array(rect(5, 5, 20, 9) + rect(30, 30, 50, 40), np.int32)).cuda()
    nb = 2
    out = [torch.full((nb * k,), CANARY, dtype=torch.uint8, device="cuda") for k in (4, 8, 4, L.PT_DET_POLY_WORK_BYTES)]
    kw = dict(scores=out[0].view(torch.float32), sums=out[1].view(torch.float64), counts=out[2].view(torch.int32), work=out[3])

    def refused(offs, pages, prob=prob_t, match="pt_op_det_poly_scores"):
        offs, pages = np.asarray(offs, np.int32), np.asarray(pages, np.int32)
        with pytest.raises(L.PtError, match=match):
            eng.op_det_poly_scores(prob, pts, torch.from_numpy(offs).cuda(), torch.from_numpy(pages).cuda(), offs, pages, **kw)
        torch.cuda.synchronize()
        assert all(bool((b == CANARY).all()) for b in out)

    refused([0, 5, 4], [0, 1], match="decrease")            # offsets that are not non-decreasing
    refused([4, 0, 8], [0, 1], match="decrease")
    refused([0, 4, 9], [0, 1], match="outside")             # ... or that leave the point list
    refused([-1, 4, 8], [0, 1], match="outside")
    refused([0, 4, 8], [0, N], match="page")                # a page index outside [0, n)
    refused([0, 4, 8], [-1, 0], match="page")
    wide = torch.zeros((1, 2, L.PT_DET_POLY_MAX_W + 32), dtype=torch.float32, device="cuda")
    refused([0, 4, 8], [0, 0], prob=wide, match="PT_DET_POLY_MAX_W")
    small = dict(kw, work=out[3][:nb * L.PT_DET_POLY_WORK_BYTES - 8])
    offs, pages = np.array([0, 4, 8], np.int32), np.array([0, 1], np.int32)
    with pytest.raises(L.PtError, match="work buffer"):
        eng.op_det_poly_scores(prob_t, pts, torch.from_numpy(offs).cuda(), torch.from_numpy(pages).cuda(), offs, pages, **small)
    # nb < 0: only the library itself can be asked
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.pt_op_det_poly_scores(vp(prob_t), N, H, W, vp(pts), 8, vp(pts), offs.ctypes.data_as(C.c_void_p), vp(pts), pages.ctypes.data_as(C.c_void_p), -1,
                                       vp(out[0]), vp(out[1]), vp(out[2]), vp(out[3]), out[3].numel(), None)
    assert rc != 0 and b"negative" in eng.lib.pt_last_error()
    torch.cuda.synchronize()
    assert all(bool((b == CANARY).all()) for b in out)
    # the limit itself is served: a map PT_DET_POLY_MAX_W wide, a contour across all of it
    rng = np.random.RandomState(5)
    row = (rng.randint(0, 1025, (1, 3, L.PT_DET_POLY_MAX_W)) / 1024.0).astype(np.float32)
    c = rect(0, 0, L.PT_DET_POLY_MAX_W - 1, 2)
    scores, sums, counts = launch(eng, torch.from_numpy(row).cuda(), [c], [0])
    s, cnt = float(row.astype(np.float64).sum()), 3 * L.PT_DET_POLY_MAX_W
    assert (counts[0], sums[0], scores[0]) == (cnt, s, R.score(s, cnt))
