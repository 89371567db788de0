"""pt_op_lore_match (csrc/lore_match.hip) through HipEngine.op_lore_match against the host chain the pipeline runs without device_match:
transform_quads + the crop offset + process_logic_output + table_cells_from_logits + find_top1_match (tests/lore_match_ref.py: host_chain).
Both sides compute in fp32 / fp64 without contraction, so they must agree as integers: no tolerance, no case left out.

Every table lives in full-size buffers ([PT_TSR_MAX_CELLS, 9] / [.., 4]) whose rows at and beyond the count hold 1e30; the logical axes are
a random permutation of the input order unless a case says otherwise."""
import numpy as np
import pytest
import torch

from lore_match_ref import host_chain, page_polygons
from pdf_table_amd import lib as L
from pdf_table_amd.tsr_stage import lore_geometry, process_logic_output, quad_inverse_map

pytestmark = pytest.mark.gpu

MAXC = L.PT_TSR_MAX_CELLS
GARBAGE = np.float32(1e30)


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    return HipEngine(0)


def _geometry(upper_left, crop_w, crop_h):
    inp = 768 if upper_left else 1024
    return lore_geometry(crop_h, crop_w, inp, inp, upper_left)[1], inp // 4


def _quad(x1, y1, x2, y2):
    return [x1, y1, x2, y1, x2, y2, x1, y2]          # TL, TR, BR, BL: bottom-left y > top-right y


def make_table(dets, axes, upper_left=False, crop=(600, 420), offset=(37, 12), count=None):
    """dets [n, 8] quads in heat-map pixels, axes [n, 4] unrounded -> the table record the helpers below take"""
    n = len(dets)
    meta, _ = _geometry(upper_left, *crop)
    d = np.full((MAXC, 9), GARBAGE, np.float32)
    a = np.full((MAXC, 4), GARBAGE, np.float32)
    d[:n, :8] = np.asarray(dets, np.float32).reshape(n, 8)
    d[:n, 8] = 0.5
    a[:n] = np.asarray(axes, np.float32).reshape(n, 4)
    return {"dets": d, "axes": a, "n": n, "count": n if count is None else count, "meta": meta, "upper_left": upper_left,
            "offset": np.asarray(offset, np.float64), "lines": np.zeros((0, 4), np.float32)}


def grid_table(rng, n, upper_left=False, crop=(600, 420), offset=(37, 12), permute=True):
    """n cells of a grid in heat-map pixels with jittered corners, noisy axes, rows in a random order"""
    _, out = _geometry(upper_left, *crop)
    cols = max(1, int(np.ceil(np.sqrt(n * 1.3))))
    rows = -(-n // cols)
    cw, ch = out * 0.9 / cols, out * 0.6 / rows
    dets, axes = [], []
    for k in range(n):
        r, c = divmod(k, cols)
        x1, y1 = out * 0.05 + c * cw, out * 0.2 + r * ch
        dets.append(np.array(_quad(x1, y1, x1 + cw, y1 + ch)) + rng.uniform(-0.1, 0.1, 8) * min(cw, ch))
        axes.append(np.array([c, c, r, r]) + rng.uniform(-0.3, 0.3, 4))
    dets, axes = np.array(dets), np.array(axes)
    if permute and n > 1:
        p = rng.permutation(n)
        dets, axes = dets[p], axes[p]
    return make_table(dets, axes, upper_left, crop, offset)


def polys_of(t):
    return page_polygons(t["dets"][:t["n"]], t["meta"], t["upper_left"], t["offset"])


def random_lines(rng, t, m):
    """m integer line boxes (the detector's are integers) in page pixels: inside cells, across their borders, beside the table"""
    p = polys_of(t)
    out = []
    for _ in range(m):
        q = p[int(rng.integers(len(p)))]
        x1, x2 = sorted((q[6], q[2]))
        y1, y2 = sorted((q[7], q[3]))
        w, h = x2 - x1, y2 - y1
        out.append([x1 + rng.uniform(-0.5 * w, 0.4 * w), y1 + rng.uniform(-0.5 * h, 0.4 * h), x2 - rng.uniform(-0.5 * w, 0.4 * w),
                    y2 - rng.uniform(-0.5 * h, 0.4 * h)])
    return np.trunc(np.array(out).reshape(-1, 4)).astype(np.float32)


def expected(tables):
    out = []
    for t in tables:
        n = min(max(int(t["count"]), 0), MAXC)
        if n == 0:
            out.append(np.full(len(t["lines"]), -1, np.int64))
        else:
            out.append(host_chain(t["dets"][:n], t["axes"][:n], t["meta"], t["upper_left"], t["offset"], t["lines"]))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def upload(eng, tables, offsets=None):
    dev = eng._tdev
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lines = np.concatenate([x["lines"] for x in tables]).astype(np.float32).reshape(-1, 4)
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([len(x["lines"]) for x in tables])])
    affine = np.stack([quad_inverse_map(x["meta"], x["upper_left"]).reshape(6) for x in tables]).astype(np.float64)
    return (t(np.stack([x["dets"] for x in tables])), t(np.stack([x["axes"] for x in tables])),
            t(np.array([x["count"] for x in tables], np.int32)), t(affine), t(np.stack([x["offset"] for x in tables]).astype(np.float64)),
            t(lines), t(np.asarray(offsets, np.int32)))


def device_match(eng, tables):
    got = eng.op_lore_match(*upload(eng, tables))
    torch.cuda.synchronize()
    eng.check()
    return got.cpu().numpy().astype(np.int64)


def check(eng, tables):
    want = expected(tables)
    got = device_match(eng, tables)
    assert got.tolist() == want.tolist()
    return want


# ---- sizes: within one lane stride, across one, across a workgroup stride, the cap; 0 .. 9 lines; B = 1 and 5 --------------------------------------
def test_five_tables_with_an_empty_one_between_and_one_without_lines(eng):
    rng = np.random.default_rng(0)
    tables = [grid_table(rng, 1, offset=(5, 300)), grid_table(rng, 63), grid_table(rng, 65, upper_left=True, crop=(333, 777)),
              grid_table(rng, 257), grid_table(rng, 40, offset=(0, 0))]
    for t, m in zip(tables, (9, 5, 3, 0, 7)):
        t["lines"] = random_lines(rng, t, m)
    tables[2]["count"] = 0                                            # the decode found nothing: its three lines get -1
    want = check(eng, tables)
    assert want[14:17].tolist() == [-1, -1, -1] and (want[:14] >= 0).all() and (want[17:] >= 0).all()
    # the sort matters: some line's cell is not the one an unsorted "first containing / first minimum" walk would give
    assert len(set(want[9:14].tolist())) > 1


@pytest.mark.parametrize("n,m,upper_left", [(1, 1, False), (63, 2, True), (65, 4, False), (257, 6, True), (257, 0, False), (MAXC, 9, False),
                                            (MAXC, 8, True)])
def test_one_table(eng, n, m, upper_left):
    rng = np.random.default_rng(100 + n + m)
    t = grid_table(rng, n, upper_left=upper_left, crop=(901, 640) if n == MAXC else (512, 300))
    t["lines"] = random_lines(rng, t, m)
    want = check(eng, [t])
    assert len(want) == m
    if n == MAXC and m:
        assert want.max() > 256                                       # rows behind the first workgroup stride do win


def test_second_call_on_the_same_buffers(eng):
    rng = np.random.default_rng(7)
    tables = [grid_table(rng, 130), grid_table(rng, 20)]
    for t in tables:
        t["lines"] = random_lines(rng, t, 9)
    args = upload(eng, tables)
    first = eng.op_lore_match(*args).cpu().numpy()
    second = eng.op_lore_match(*args).cpu().numpy()
    assert first.tolist() == second.tolist() == expected(tables).tolist()


# ---- ties ------------------------------------------------------------------------------------------------------------------------------------------
def test_identical_and_nested_cells_the_first_in_sorted_order_wins(eng):
    big, small, far = _quad(40, 40, 120, 100), _quad(60, 55, 100, 85), _quad(150, 40, 200, 100)
    # 0: two identical cells with identical axes: the smaller input row.  1: identical cells, the LATER row sorts first (smaller top).
    # 2: a cell inside another, both contain the line; the outer one comes later in the input and first in the sort
    t0 = make_table([far, big, big], [[5, 5, 0, 0], [1, 1, 2, 2], [1, 1, 2, 2]])
    t1 = make_table([far, big, big], [[5, 5, 0, 0], [1, 1, 3, 3], [1, 1, 2, 2]])
    t2 = make_table([far, small, big], [[5, 5, 9, 9], [2, 2, 4, 4], [1, 1, 4, 4]])
    t3 = make_table([far, big, small], [[5, 5, 9, 9], [2, 2, 4, 4], [1, 1, 4, 4]])
    inner = polys_of(t2)[1]                                          # a line well inside the small cell (and so inside the big one)
    for t in (t0, t1, t2, t3):
        t["lines"] = np.trunc(np.array([[inner[6] + 4, inner[3] + 4, inner[2] - 4, inner[7] - 4]])).astype(np.float32)
    want = check(eng, [t0, t1, t2, t3])
    assert want.tolist() == [1, 2, 2, 2]


def test_equal_k1_and_distance_fall_to_the_sort_key(eng):
    """two cells of identical geometry, neither containing the line: (k1, dist) are equal bit for bit, the axes decide, then the row"""
    a, far = _quad(40, 40, 120, 100), _quad(10, 150, 30, 170)
    t0 = make_table([far, a, a], [[0, 0, 9, 9], [3, 3, 2, 2], [2, 2, 2, 2]])       # row 2: equal top, smaller left
    t1 = make_table([far, a, a], [[0, 0, 9, 9], [3, 3, 2, 2], [3, 3, 2, 2]])       # all equal: row 1
    t2 = make_table([far, a, a], [[0, 0, 9, 9], [3, 4, 2, 5], [3, 3, 2, 5]])       # equal top, left, bottom: smaller right -> row 2
    for t in (t0, t1, t2):
        p = polys_of(t)[1]
        t["lines"] = np.trunc(np.array([[p[2] + 10, p[3] - 30, p[2] + 60, p[3] - 10]])).astype(np.float32)      # right of and above the cell
    want = check(eng, [t0, t1, t2])
    assert want.tolist() == [2, 1, 2]


def test_axis_fraction_at_just_above_and_just_below_one_half(eng):
    """process_logic_output rounds up only where the fraction is > 0.5 in float32"""
    a, far = _quad(40, 40, 120, 100), _quad(150, 150, 170, 170)
    up, half, below = np.nextafter(np.float32(2.5), np.float32(3)), np.float32(2.5), np.nextafter(np.float32(2.5), np.float32(2))
    assert process_logic_output(np.array([up, half, below], np.float32)).tolist() == [3.0, 2.0, 2.0]
    t0 = make_table([far, a, a], [[9, 9, 9, 9], [0, 0, up, 5], [0, 0, half, 5]])         # row 1 -> top 3, row 2 -> top 2: row 2
    t1 = make_table([far, a, a], [[9, 9, 9, 9], [1, 1, 2.0, 5], [0, 0, below, 5]])       # both top 2, row 2 has the smaller left: row 2
    t2 = make_table([far, a, a], [[9, 9, 9, 9], [0, 0, 3.0, 5], [0, 0, up, 5]])          # both top 3: row 1
    t3 = make_table([far, a, a], [[9, 9, 9, 9], [0, 0, -1.5, 5], [0, 0, np.nextafter(np.float32(-1.5), np.float32(0)), 5]])  # -2 against -1: row 1
    for t in (t0, t1, t2, t3):
        p = polys_of(t)[1]
        t["lines"] = np.trunc(np.array([[p[6] + 5, p[3] + 5, p[2] - 5, p[7] - 5]])).astype(np.float32)
    want = check(eng, [t0, t1, t2, t3])
    assert want.tolist() == [2, 2, 1, 1]


# ---- the diff boundary ---------------------------------------------------------------------------------------------------------------------------
def test_line_exactly_on_the_diff_boundary(eng):
    """t0 == c0 - 2 and t2 == c2 + 2 in double: still inside, and of the two identical cells that contain the line the one sorting first wins.
    One float32 step further out on either side: neither contains it any more, and a cell that does -- the whole table, sorting last -- takes it"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        x1, x2 = rng.uniform(30, 60), rng.uniform(120, 160)
        cell = _quad(x1, 40, x2, 100)
        t = make_table([_quad(10, 150, 30, 170), cell, cell], [[0, 0, 0, 0], [1, 1, 5, 5], [1, 1, 4, 4]], offset=(0, 0))
        p = polys_of(t)[1]
        lo, hi = p[6] - 2.0, p[2] + 2.0
        if np.float64(np.float32(lo)) == lo and np.float64(np.float32(hi)) == hi and p[7] - p[3] > 20:
            break
    else:
        raise AssertionError("no cell whose grown edges are float32 numbers")
    y_top, y_bot = np.float32(np.trunc(p[3] + 5)), np.float32(np.trunc(p[7] - 5))
    lo32, hi32 = np.float32(lo), np.float32(hi)
    out_lo, out_hi = np.nextafter(lo32, np.float32(-1e9)), np.nextafter(hi32, np.float32(1e9))
    # a third cell that contains even the lines one step out, sorting LAST: it wins only when the twins no longer contain the line
    t = make_table([_quad(1, 1, 250, 250), cell, cell], [[0, 0, 9, 9], [1, 1, 5, 5], [1, 1, 4, 4]], offset=(0, 0))
    t["lines"] = np.array([[lo32, y_top, hi32, y_bot], [out_lo, y_top, hi32, y_bot], [lo32, y_top, out_hi, y_bot]], np.float32)
    want = check(eng, [t])
    assert want.tolist() == [2, 0, 0]


# ---- a pair with overlap ---------------------------------------------------------------------------------------------------------------------------
def test_overlap_decides_for_cells_whose_corners_are_flipped(eng):
    """a quad written bottom-up has y1 < y2 in the (bottom-left, top-right) box, so compute_iou_v2's intersection is not empty: a line that no
    cell contains goes to the cell it overlaps most, not to the nearest by the corner distance"""
    def flipped(x1, y1, x2, y2):
        return [x1, y2, x2, y2, x2, y1, x1, y1]                     # "TL" at the bottom: vertex 3 (x1, y1) lies above vertex 1 (x2, y2)
    # heat-map pixels.  The line (10, 42) .. (208, 118) sticks out of the big cell on the left and out of the low one on the right: iou 0.76
    # with the big cell at corner distance 50, iou 0.61 with the low one at distance 36
    cells = [flipped(50, 40, 210, 120), flipped(10, 42, 200, 90), _quad(88, 58, 112, 82), flipped(30, 130, 60, 160)]
    t = make_table(cells + [flipped(10, 42, 208, 118)], [[0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [4, 4, 4, 4]])
    p = polys_of(t)
    assert p[0][7] < p[0][3] and p[2][7] > p[2][3]
    line = np.trunc(np.array([[p[4][6], p[4][7], p[4][2], p[4][3]]])).astype(np.float32)
    t = make_table(cells, [[0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3]])
    p = polys_of(t)
    t["lines"] = np.concatenate([line, random_lines(np.random.default_rng(5), t, 8)])
    want = check(eng, [t])
    from pdf_table_amd.table_text_match import find_top1_match
    cb = np.stack([p[:, 6], p[:, 7], p[:, 2], p[:, 3]], 1)
    tl = t["lines"][:1].astype(np.float64)
    d1 = np.abs(cb[:, 0] - tl[0, 0]) + np.abs(cb[:, 1] - tl[0, 1])
    d2 = np.abs(cb[:, 2] - tl[0, 2]) + np.abs(cb[:, 3] - tl[0, 3])
    nearest = int(np.argmin((d1 + d2) + np.minimum(d1, d2)))
    assert find_top1_match(tl, cb).tolist() == [want[0]]             # rows are in sorted order already here
    assert want[0] == 0 and nearest == 1                             # the overlap term decided, not the distance


# ---- clamps ------------------------------------------------------------------------------------------------------------------------------------------
def test_counts_out_of_range_are_clamped(eng):
    rng = np.random.default_rng(11)
    t0 = grid_table(rng, MAXC, crop=(901, 640))
    t0["lines"] = random_lines(rng, t0, 5)
    t0["count"] = MAXC + 500
    t1 = grid_table(rng, 30)
    t1["lines"] = random_lines(rng, t1, 4)
    t1["count"] = -3
    want = check(eng, [t0, t1])
    assert (want[:5] >= 0).all() and want[5:].tolist() == [-1] * 4


def test_offsets_that_are_not_monotone_touch_nothing_outside_the_lines(eng):
    """offsets [-5, 3, 6, 4, 99] over M = 9 lines: table 0 owns 0 .. 2, table 1 3 .. 5, table 2 nothing (6 .. 4), table 3 4 .. 8 -- it shares two
    lines with table 1, so the two are the same table and write the same rows.  A canary region behind the output stays as it was."""
    from pdf_table_amd.engine import _ptr
    rng = np.random.default_rng(13)
    a, b = grid_table(rng, 70), grid_table(rng, 90)
    lines_a, lines_b = random_lines(rng, a, 3), random_lines(rng, b, 6)
    a["lines"], b["lines"] = lines_a, lines_b
    want = np.concatenate([host_chain(a["dets"][:70], a["axes"][:70], a["meta"], False, a["offset"], lines_a),
                           host_chain(b["dets"][:90], b["axes"][:90], b["meta"], False, b["offset"], lines_b)])
    twin = dict(b, lines=np.zeros((0, 4), np.float32))               # upload() concatenates the lines: a's 3, then b's 6
    dets, axes, counts, affine, offset, lines, offsets = upload(eng, [a, b, grid_table(rng, 10), twin], offsets=[-5, 3, 6, 4, 99])
    M, pad = 9, 1024
    assert lines.shape == (M, 4)
    out = torch.full((M + pad,), -77, dtype=torch.int32, device=eng._tdev)
    L.check(eng.lib.pt_op_lore_match(_ptr(dets), _ptr(axes), _ptr(counts), 4, _ptr(affine), _ptr(offset), _ptr(lines), _ptr(offsets), M,
                                     _ptr(out), eng._stream()), "pt_op_lore_match")
    torch.cuda.synchronize()
    eng.check()
    got = out.cpu().numpy()
    assert got[:M].tolist() == want.tolist()
    assert (got[M:] == -77).all()


def test_argument_checks(eng):
    rng = np.random.default_rng(17)
    t = grid_table(rng, 5)
    t["lines"] = random_lines(rng, t, 2)
    dets, axes, counts, affine, offset, lines, offsets = upload(eng, [t])
    with pytest.raises(L.PtError):
        eng.op_lore_match(dets, axes, counts, affine.float(), offset, lines, offsets)
    with pytest.raises(ValueError):
        eng.op_lore_match(dets[:, :100].contiguous(), axes, counts, affine, offset, lines, offsets)
    with pytest.raises(ValueError):
        eng.op_lore_match(dets, axes, counts, affine, offset, lines, offsets[:1])
    assert eng.op_lore_match(dets, axes, counts, affine, offset, lines[:0], torch.zeros(2, dtype=torch.int32, device=eng._tdev)).numel() == 0
