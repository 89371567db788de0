"""pt_op_cell_metric (csrc/cell_metric.hip) alone, through HipEngine.op_cell_metric: `match` and the counts compared AS INTEGERS with
tests/cell_metric_ref.py's loop-for-loop restatement of the reference (tables up to 300 cells) or with the package's host route (above; the host route
itself is pinned to the reference's own run and to the restatement in tests/test_cell_metric_host.py).

Sizes: n_pred / n_gt from {0, 1, 63, 64, 65, 255, 256, 257} (a thread ranks cells tid, tid + 256, ..: 256 is where a second one appears; 64 is a wave),
1023 / 1024 / 1025 (the kernel places 1024 prediction cells per LDS tile) and 3071 / 3072 / 3073 (it stages 3072 sort keys per tile).  Every golden case.
Constructed cases: the only match at the last rank; a match in the second tile with a higher IoU in the third; all keys equal; keys descending in input
order; a chunk of 70 pairs with empty pairs first, in the middle and last and canaries behind both outputs; one 4096 x 4096 pair; a second call on the
same buffers; 4097 cells, a range outside N, matches outside d_match and a zero threshold refused with nothing written."""
import json
import os

import numpy as np
import pytest
import torch

import cell_metric_ref as R
from pdf_table_amd import cell_metric as M
from pdf_table_amd.cell_metric_synth import sized_pair
from pdf_table_amd.lib import PtError

pytestmark = pytest.mark.gpu

CANARY = -777
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "cell_metric.json")) as _f:
    CASES = json.load(_f)["cases"]

SIZES = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 257), (257, 1), (63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (64, 256), (1023, 1025),
         (1024, 1024), (1025, 1023), (3071, 90), (3072, 90), (3073, 90)]


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    return HipEngine(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tables(pred, gt):
    return M._table(pred), M._table(gt)


def want_of(pred, gt):
    """(match list, tp, truep): the restatement's loops up to 300 cells a side, the host route above"""
    if max(len(pred[0]), len(gt[0])) <= 300:
        r = R.pair(R.units_of(*pred), R.units_of(*gt))
        return r["match"], r["tp"], r["truep"]
    m, tp, truep = M.match_pair(pred, gt)
    return m.tolist(), tp, truep


def run(eng, pairs, thr=0.5, canary=8):
    """one launch over `pairs`; -> (per pair match list, counts [P, 2], the buffers for a second call).  Canaries behind both outputs are checked."""
    boxes, axes, rec, moff = M.pack_chunk([tables(p, g) for p, g in pairs])
    P, total = len(rec), int(rec[:, 3].sum())
    match = torch.full((total + canary,), CANARY, dtype=torch.int32, device="cuda")
    counts = torch.full((P + canary, 2), CANARY, dtype=torch.int32, device="cuda")
    args = (dev(boxes), dev(axes), dev(rec), rec, thr)
    kw = dict(moff=dev(moff), h_moff=moff, match=match, counts=counts, match_elems=total)
    eng.op_cell_metric(*args, **kw)
    m, c = match.cpu().numpy(), counts.cpu().numpy()
    assert np.all(m[total:] == CANARY) and np.all(c[P:] == CANARY)
    return [m[moff[k]:moff[k] + rec[k, 3]].tolist() for k in range(P)], c[:P], (args, kw, match, counts)


def check(eng, pairs, wants=None):
    got, counts, bufs = run(eng, pairs)
    wants = wants or [want_of(*tables(p, g)) for p, g in pairs]
    for k, (w, g) in enumerate(zip(wants, got)):
        assert g == w[0], (k, [(i, a, b) for i, (a, b) in enumerate(zip(g, w[0])) if a != b][:8])
        assert counts[k].tolist() == [w[1], w[2]], k
    return got, counts, bufs


@pytest.fixture(scope="module")
def size_cases():
    """pairs and reference answers of SIZES, computed once"""
    out = {}
    for k, (n_pred, n_gt) in enumerate(SIZES):
        pred, gt = sized_pair(100 + k, n_pred, n_gt)
        out[(n_pred, n_gt)] = ((pred, gt), want_of(*tables(pred, gt)))
    return out


@pytest.mark.parametrize("n_pred,n_gt", SIZES)
def test_sizes(eng, size_cases, n_pred, n_gt):
    pair, want = size_cases[(n_pred, n_gt)]
    got, counts, _ = check(eng, [pair], [want])
    if min(n_pred, n_gt) >= 63:
        assert 0 < counts[0, 1] < counts[0, 0] <= n_gt                    # some matches, some of them with wrong axes: the comparison is not vacuous
    if n_pred == 0:
        assert got[0] == [-1] * n_gt and counts[0].tolist() == [0, 0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases(eng, name):
    c = CASES[name]
    pu, gu = R.load_lines(c["center"], c["logi"]), R.load_lines(c["gt_center"], c["gt_logi"])
    arr = lambda us: (np.asarray([[u.point1[0][0], u.point1[0][1], 0, 0, u.point3[0][0], u.point3[0][1], 0, 0] for u in us], np.float64).reshape(-1, 8),
                      np.asarray([u.axis[:4] for u in us], np.int64).reshape(-1, 4))
    ref = R.pair(pu, gu)
    assert ref["match_sorted"] == c["match_sorted"]                        # the restatement gives what the reference gave for this case
    check(eng, [(arr(pu), arr(gu))], [(ref["match"], ref["tp"], ref["truep"])])


def far_boxes(n):
    """n boxes of 10 x 10 far from the origin and from each other"""
    k = np.arange(n, dtype=np.float64)
    x, y = 1000 + 20 * (k % 64), 1000 + 20 * (k // 64)
    return np.stack([x, y, x + 10, y, x + 10, y + 10, x, y + 10], 1).reshape(n, 8)


def box(x1, y1, x3, y3):
    return np.asarray([x1, y1, x3, y1, x3, y3, x1, y3], np.float64)


@pytest.mark.parametrize("n", [300, 1025, 2500])
def test_only_match_at_the_last_rank(eng, n):
    rng = np.random.default_rng(n)
    pb, rank = far_boxes(n), rng.permutation(n)                           # cell i sorts at rank[i]
    pa = np.stack([np.zeros(n), np.zeros(n), rank, np.zeros(n)], 1).astype(np.int64)
    last = int(np.nonzero(rank == n - 1)[0][0])
    pb[last] = box(0, 0, 10, 9)
    gt = (np.stack([box(0, 0, 10, 10), box(500, 500, 510, 510)]), np.asarray([[0, 0, n - 1, 0], [1, 1, 1, 1]]))
    check(eng, [((pb, pa), gt)], [([last, -1], 1, 1)])


def test_first_rank_wins_over_a_higher_iou_in_a_later_tile(eng):
    n = 2500
    rng = np.random.default_rng(5)
    pb, rank = far_boxes(n), rng.permutation(n)
    pa = np.stack([rank % 7, np.zeros(n), rank, np.zeros(n)], 1).astype(np.int64)
    second, third = int(np.nonzero(rank == 1500)[0][0]), int(np.nonzero(rank == 2200)[0][0])
    pb[second], pb[third] = box(0, 0, 10, 6), box(0, 0, 10, 10)        # IoU 0.6 in the second LDS tile, IoU 1 in the third
    gt = (box(0, 0, 10, 10)[None], pa[third][None])
    check(eng, [((pb, pa), gt)], [([second], 1, 0)])
    pb[second] = box(0, 0, 10, 4)                                        # IoU 0.4: now the third tile's cell is the first to reach 0.5
    check(eng, [((pb, pa), gt)], [([third], 1, 1)])


@pytest.mark.parametrize("keys", ["equal", "descending"])
def test_key_orders(eng, keys):
    n = 250
    (pb, pa), gt = sized_pair(77, n, 240, jitter=6.0)
    pb = np.concatenate([pb, pb[:40] + 1.0])                              # 40 near-duplicates: which of the two is taken depends on the order alone
    pa = np.concatenate([pa, pa[:40]])
    if keys == "equal":
        pa[:] = 3
    else:
        pa[:, 2] = np.arange(len(pa))[::-1]
    check(eng, [((pb, pa), gt)])


def test_chunk_of_70_pairs_and_second_call(eng):
    sizes = [(0, 0)] + [(7 * k % 97 + 1, 11 * k % 89 + 1) for k in range(1, 69)] + [(5, 0)]
    sizes[33], sizes[34], sizes[50] = (0, 12), (0, 0), (300, 260)
    pairs = [sized_pair(500 + k, a, b) for k, (a, b) in enumerate(sizes)]
    assert len(pairs) == 70
    got, counts, (args, kw, match, counts_d) = check(eng, pairs)
    assert counts[0].tolist() == [0, 0] and counts[34].tolist() == [0, 0] and counts[69].tolist() == [0, 0] and got[33] == [-1] * 12
    first = (match.cpu().numpy().copy(), counts_d.cpu().numpy().copy())
    eng.op_cell_metric(*args, **kw)                                       # the same buffers again
    assert np.array_equal(match.cpu().numpy(), first[0]) and np.array_equal(counts_d.cpu().numpy(), first[1])
    # the default offsets (derived from the pair records) and allocated outputs give the same
    m2, c2 = eng.op_cell_metric(*args)
    total = int(args[3][:, 3].sum())
    assert np.array_equal(m2.cpu().numpy()[:total], first[0][:total]) and np.array_equal(c2.cpu().numpy()[:70], first[1][:70])


def test_4096_by_4096(eng):
    pair = sized_pair(4096, 4096, 4096)
    _, counts, _ = check(eng, [pair])
    assert 2000 < counts[0, 1] < counts[0, 0] <= 4096


def test_refusals_write_nothing(eng):
    (pb, pa), (gb, ga) = sized_pair(1, 20, 20)
    boxes, axes, rec, moff = M.pack_chunk([tables((pb, pa), (gb, ga))])
    match = torch.full((64,), CANARY, dtype=torch.int32, device="cuda")
    counts = torch.full((4, 2), CANARY, dtype=torch.int32, device="cuda")
    d_boxes, d_axes, d_moff = dev(boxes), dev(axes), dev(moff)
    call = lambda r, thr=0.5, me=20: eng.op_cell_metric(d_boxes, d_axes, dev(r), r, thr, moff=d_moff, h_moff=moff, match=match, counts=counts, match_elems=me)
    big = rec.copy()
    big[0, 1] = 4097
    with pytest.raises(PtError, match="4097"):
        call(big)
    out = rec.copy()
    out[0, 2] = 21                                                        # the truth's 20 cells would end one behind the 40 of the arrays
    with pytest.raises(PtError, match="of 40"):
        call(out)
    neg = rec.copy()
    neg[0, 0] = -1
    with pytest.raises(PtError, match="names cells"):
        call(neg)
    with pytest.raises(PtError, match="d_match holds 19"):
        call(rec, me=19)
    for thr in (0.0, -1.0, float("nan")):
        with pytest.raises(PtError, match="threshold"):
            call(rec, thr=thr)
    torch.cuda.synchronize()
    assert np.all(match.cpu().numpy() == CANARY) and np.all(counts.cpu().numpy() == CANARY)
    call(rec)                                                             # and the untouched record is served
    w = want_of(*tables((pb, pa), (gb, ga)))
    assert match.cpu().numpy()[:20].tolist() == w[0] and counts.cpu().numpy()[0].tolist() == [w[1], w[2]]
    assert np.all(match.cpu().numpy()[20:] == CANARY)
    # a whole table of 4097 cells, as the metric would pack it: refused as well
    with pytest.raises(PtError, match="4097"):
        run(eng, [sized_pair(2, 4097, 3)])
    assert eng.op_cell_metric(d_boxes, d_axes, dev(np.zeros((0, 4), np.int64)), np.zeros((0, 4), np.int64))[1].shape == (1, 2)      # P == 0: no launch
