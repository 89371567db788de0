"""pt_op_table_match (csrc/table_match.hip) through HipEngine.op_table_match against the host chain of pdf_table_amd/table_structure_match.py --
filter_lines + match_result on the polygons TableLabelDecode.decode_ids and the page-frame shift produce from the same head outputs.  The two must
agree as integers: the host module reproduces the reference's recorded results exactly (tests/test_table_structure_match_host.py), and the kernel
restates the same float32 / float64 operations unfused, so there is nothing to tolerate.

Three tables per call -- 0: an ordinary one, 1: no cell row at all, 2: steps < T with a cell token lying behind steps -- at T = 10, 65 and 130 (rows
within one lane stride, across one, across two), L = 4 and 8, per-table line counts out of 0, 1, 5 and 9, frames with non-zero x0 / y0."""
import json
import os

import numpy as np
import pytest
import torch

from pdf_table_amd import table_structure_match as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
V, CELL_IDS = 30, (5, 7)
FRAMES = np.array([[317, 211, 40, 25], [200, 150, 0, 0], [123, 457, 301, 7]], np.float32)      # (w, h, x0, y0)
COUNTS = {10: (9, 5, 1), 65: (0, 1, 5), 130: (5, 9, 0)}


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    return HipEngine(0)


def flags():
    f = np.zeros(V, np.uint8)
    f[list(CELL_IDS)] = 1
    return f


def host_polygons(loc, ids, steps, frame):
    """one table: (polygons [cells, 8] float32 in page pixels as SlaNetStage.finish makes them, step index of every cell)"""
    w, h, x0, y0 = (float(v) for v in frame)
    rows = [t for t in range(int(steps)) if flags()[ids[t]]]
    polys = []
    for t in rows:
        bb = np.array(loc[t], dtype=np.float32)
        bb[0::2] *= w                                  # TableLabelDecode.decode_ids
        bb[1::2] *= h
        if len(bb) == 4:                               # slanet_shape_result
            x1, y1, x2, y2 = bb
            bb = np.array([x1, y1, x2, y1, x2, y2, x1, y2], np.float32)
        polys.append(bb + np.tile(np.array([x0, y0], np.float32), 4))      # the page-frame shift
    return (np.stack(polys) if polys else np.zeros((0, 8), np.float32)), rows


def host_match(loc, ids, steps, frames, lines, offsets):
    out = np.full(len(lines), -1, np.int32)
    for b in range(len(frames)):
        polys, rows = host_polygons(loc[b], ids[b], steps[b], frames[b])
        lb = lines[offsets[b]:offsets[b + 1]]
        if len(polys) == 0 or len(lb) == 0:
            continue
        kept = M.filter_lines(polys, lb)
        for cell, ls in M.match_result(lb[kept], polys).items():
            out[offsets[b] + kept[ls]] = rows[cell]
    return out


def device_match(eng, loc, ids, steps, frames, lines, offsets):
    dev = eng._tdev
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = eng.op_table_match(t(loc), t(ids), None if steps is None else t(steps), t(flags()), t(frames), t(lines.astype(np.float32)), t(offsets))
    torch.cuda.synchronize()
    eng.check()
    return got.cpu().numpy()


def case(T, L, seed):
    g = np.random.default_rng(seed)
    loc = g.uniform(0.02, 0.98, (3, T, L)).astype(np.float32)
    if L == 4:
        loc[0] = np.sort(loc[0].reshape(T, 2, 2), axis=1).reshape(T, 4)        # table 0: proper (x1, y1, x2, y2); the others: any order (min / max)
    others = [i for i in range(1, V - 1) if i not in CELL_IDS]
    ids = np.where(g.uniform(size=(3, T)) < 0.6, g.choice(CELL_IDS, (3, T)), g.choice(others, (3, T))).astype(np.int32)
    ids[1] = g.choice(others, T)                                                # table 1: no cell row
    steps = np.array([T, T, T - 4], np.int32)
    ids[2, T - 2] = CELL_IDS[0]                                                 # a cell token behind steps: must be ignored
    loc[2, T - 2] = 0.5
    ids[2, 1], ids[0, 3] = CELL_IDS[1], CELL_IDS[0]
    if T > 67:                                                                  # the same cell at rows 3 and 67: 3 must win
        ids[0, 67], loc[0, 67] = CELL_IDS[1], loc[0, 3]
    counts = COUNTS[T]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    lines = []
    for b, n in enumerate(counts):
        w, h, x0, y0 = FRAMES[b]
        xy = np.stack([g.integers(x0 - 5, x0 + w - 20, n), g.integers(y0 - 5, y0 + h - 10, n)], 1)
        lines.append(np.concatenate([xy, xy + np.stack([g.integers(5, 120, n), g.integers(4, 40, n)], 1)], 1))
    lines = np.concatenate(lines).astype(np.float64)
    if counts[0] >= 5:
        polys, rows = host_polygons(loc[0], ids[0], T, FRAMES[0])
        c3 = polys[rows.index(3)]
        lines[0] = [np.ceil(c3[0::2].min()), np.ceil(c3[1::2].min()), np.floor(c3[0::2].max()), np.floor(c3[1::2].max())]      # cell 3's box, to the pixel
        lines[1] = [FRAMES[0][2], 0.0, FRAMES[0][2] + 30.0, 1.0]                                                                # above every cell: dropped
    return loc, ids, steps, lines, offsets


@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("T", [10, 65, 130])
def test_kernel_equals_the_host_chain(eng, T, L):
    loc, ids, steps, lines, offsets = case(T, L, 100 * T + L)
    want = host_match(loc, ids, steps, FRAMES, lines, offsets)
    got = device_match(eng, loc, ids, steps, FRAMES, lines, offsets)
    print(f"T {T} L {L}: lines per table {COUNTS[T]}, want {want.tolist()}")
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    n0, n1 = offsets[1], offsets[2]
    assert (got[n0:n1] == -1).all()                                             # the table without a cell row
    assert not (got[n1:] == T - 2).any() and (got[n1:] < T - 4).all()           # nothing behind steps
    if COUNTS[T][0] >= 5:
        assert got[0] == 3 and got[1] == -1                                     # the duplicate at row 67 loses to row 3; the line above the cells is dropped
        assert (got[:n0] >= 0).sum() >= 3


def test_steps_may_be_null(eng):
    loc, ids, _, lines, offsets = case(65, 8, 7)
    full = np.full(3, 65, np.int32)
    want = host_match(loc, ids, full, FRAMES, lines, offsets)
    assert device_match(eng, loc, ids, None, FRAMES, lines, offsets).tolist() == want.tolist()
    assert (want[offsets[2]:] >= 0).any()


@pytest.mark.parametrize("name", ["f32_area_decides", "random_f32_dense", "y_filter", "identical_cells", "iou0_equal_distance", "equal_iou_mirror"])
def test_golden_cases_through_the_kernel(eng, name):
    """the reference's recorded match maps, cells fed as loc with a unit frame (fl32(fl32(c * 1) + 0) = c).  f32_area_decides is the case where the
    float32 rounding of the cell's own area decides the winner"""
    with open(os.path.join(HERE, "golden", "table_match.json")) as f:
        gold = next(c for c in json.load(f)["cases"] if c["name"] == name)
    cells = np.array(gold["cells"], np.float32)
    lines = np.array(gold["lines"], np.float64)
    T = len(cells) + 3
    loc = np.zeros((1, T, 4), np.float32)
    loc[0, 2:2 + len(cells)] = cells                                            # cells at steps 2 ..: step index = cell index + 2
    ids = np.full((1, T), 1, np.int32)
    ids[0, 2:2 + len(cells)] = CELL_IDS[0]
    want = np.full(len(lines), -1, np.int32)
    for cell, ls in gold["matched"]:
        want[np.array(gold["kept"])[ls]] = cell + 2
    got = device_match(eng, loc, ids, np.array([T], np.int32), np.array([[1, 1, 0, 0]], np.float32), lines, np.array([0, len(lines)], np.int32))
    assert got.tolist() == want.tolist()
    if name == "f32_area_decides":
        assert got[0] - 2 != gold["float64_winner"]


def test_bad_arguments_name_the_entry_point(eng):
    from pdf_table_amd.lib import PtError
    dev = eng._tdev
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    with pytest.raises(PtError, match="pt_op_table_match"):
        eng.op_table_match(z((1, 10, 6), torch.float32), z((1, 10), torch.int32), None, z((V,), torch.uint8), z((1, 4), torch.float32),
                           z((2, 4), torch.float32), z((2,), torch.int32))
    with pytest.raises(PtError, match="pt_op_table_match"):
        eng.op_table_match(z((1, 4096, 4), torch.float32), z((1, 4096), torch.int32), None, z((V,), torch.uint8), z((1, 4), torch.float32),
                           z((2, 4), torch.float32), z((2,), torch.int32))
