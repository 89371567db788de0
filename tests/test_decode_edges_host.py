"""CPU half of the decode edge cases: the tie-breaking top-K helper equals the oracle's on tie-free maps, and every generator of
tests/decode_edge_synth.py really produces the edge it is named after, judged by the CPU references (oracle.lore_decode,
tests/centernet_ref.py).  The GPU half (tests/test_gpu_decode_edges.py) compares the kernels with the same references."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import centernet_ref as R  # noqa: E402
import decode_edge_ref as E  # noqa: E402
from lore_synth import synth_lore_heads  # noqa: E402
from oracle import lore_decode as od  # noqa: E402

HEAT_CAP = 16384          # PT_HEAT_CAP, pdf_table_amd/csrc/common.h


@pytest.mark.parametrize("seed,H,W", [(1, 80, 80), (2, 72, 96), (3, 80, 80), (4, 128, 128)])
def test_lexsort_topk_equals_oracle_topk_without_ties(seed, H, W):
    """bit for bit, both classes at their K, on the maps of test_tsr_decode_matches_oracle.  Non-peaks are exact zeros after the
    max-pool mask -- ties among themselves -- so the maps are cut where the scores reach zero: there the indices are compared as far as
    the positive scores go and the scores over all K rows."""
    hm = torch.sigmoid(torch.from_numpy(synth_lore_heads(seed, H, W)["hm"]))
    for cls, K in ((0, od.K_CELLS), (1, od.K_CORNERS)):
        nm = od.nms_peaks(hm[:, cls:cls + 1])
        a, b = od.topk_1class(nm, K), E.lexsort_topk_1class(nm, K)
        npos = int((a[0] > 0).sum())
        assert npos > 50 and len(np.unique(a[0][0, :npos].numpy())) == npos          # tie-free where it matters
        assert torch.equal(a[0], b[0])
        for x, y in zip(a[1:], b[1:]):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert torch.equal(x[0, :npos], y[0, :npos])


@pytest.mark.parametrize("seed,H,W,rev", [(1, 80, 80, True), (2, 72, 96, True), (3, 80, 80, False), (4, 128, 128, True)])
def test_tie_breaking_reference_equals_oracle_without_ties(seed, H, W, rev):
    """the whole decode with both replacements of the tie cases (index-ascending top-K, stable re-sort after the snap) gives the plain
    oracle's rows and logic features bit for bit on the tie-free maps of test_tsr_decode_matches_oracle"""
    heads = synth_lore_heads(seed, H, W)
    a, b = E.lore_reference(heads, rev, ties=False), E.lore_reference(heads, rev, ties=True)
    n = a["n"]
    assert n == b["n"] > 20
    assert np.array_equal(a["raw"][:n], b["raw"][:n]) and np.array_equal(a["logi"], b["logi"])


def test_torch_topk_is_not_index_ascending_on_ties():
    """the helper's tie order is the kernels' contract, index ascending; torch.topk promises none (here it does not come back
    ascending on this map -- printed, not asserted: it is a property of the torch build)"""
    flat = torch.full((1, 1, 40, 40), 0.7)
    _, ind, _, _ = od.topk_1class(flat, 1000)
    _, ind2, _, _ = E.lexsort_topk_1class(flat, 1000)
    assert torch.equal(ind2[0], torch.arange(1000))
    print("torch.topk ascending on a constant map:", bool(torch.equal(ind[0], torch.arange(1000))))


def _lore_peaks(heads):
    """per class: (flat indices in (score desc, index asc) order of the peaks at or above the class threshold, their scores)"""
    hm = torch.sigmoid(torch.from_numpy(heads["hm"]))
    out = []
    for cls, thr in ((0, 0.2), (1, 0.3)):
        nm = od.nms_peaks(hm[:, cls:cls + 1])
        s, ind, _, _ = E.lexsort_topk_1class(nm, nm.numel())
        keep = s[0].numpy() >= np.float32(thr)
        out.append((ind[0].numpy()[keep], s[0].numpy()[keep]))
    return out


def _cn_peaks(heads):
    sig = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(heads["hm"][0]))).numpy()
    return [R._peaks_topk(sig[cls], sig[cls].size) for cls in range(2)]


def _check_common(peaks, facts, ties=False):
    assert [len(p[0]) for p in peaks] == list(facts["peaks"]), ([len(p[0]) for p in peaks], facts["peaks"])
    # no two DIFFERENT scores of a class closer than 2e-6: the device's sigmoid (expf) may differ from the reference's in the last bits,
    # and the order must not hang on them.  Equal scores come from equal logits (the plateaus of the tie cases) and stay equal on the device.
    for idx, s in peaks:
        d = -np.diff(s.astype(np.float64))
        assert ties or (d > 0).all()
        assert (d[d > 0] > 2e-6).all()


@pytest.mark.parametrize("name", list(E.LORE_CASES))
def test_lore_case_exercises_its_edge(name):
    heads, facts, rev, ref = E.lore_case(name)
    H, W = heads["hm"].shape[2:]
    assert H <= 144 and W <= 144 and H * W >= od.K_CORNERS
    peaks = _lore_peaks(heads)
    _check_common(peaks, facts, ties=E.LORE_CASES[name][2])
    raw, n = ref["raw"], ref["n"]
    if name in ("ties", "ties_rev"):
        for cls in range(2):
            assert np.array_equal(peaks[cls][0], facts["order"][cls])
            s = peaks[cls][1]
            assert (s[:36] == 1.0).all() and len(np.unique(s[-64:])) == 1 and s[36] < 1.0 and s[-65] > s[-64]
        if rev:
            # the corner class's tie order is visible: cells are hit by several corners of EQUAL score, whose replay order in the snap loop
            # is their order in the list; and the snap moved vertices, so the output depends on it
            bboxes, scores, gboxes, cxs, cys, cscores = ref["snap"]
            nc = facts["peaks"][1]
            tied = 0
            for i in range(facts["peaks"][0]):
                hit = [j for j in range(nc) if od.is_group(bboxes[i], gboxes[j])]
                sc = cscores[hit]
                tied += int(len(sc) - len(np.unique(sc)) >= 1)
            assert tied >= 10, tied
            assert n >= 10
        else:
            assert n == facts["peaks"][0]
    elif name.startswith("cap_cells"):
        assert facts["peaks"][0] > od.K_CELLS and (H * W) % 1024 == 0
        assert n == od.K_CELLS, n                 # every kept cell stays visible: the cap, not a threshold, ends the list
        assert peaks[0][1][od.K_CELLS] * 0.4 >= 0.2           # ... and the first dropped one would have been visible too
        assert ref["snap"] is None or (ref["snap"][5] >= 0.3).sum() == 0
    elif name == "cap_corners":
        assert facts["peaks"][1] > od.K_CORNERS and (H * W) % 1024 != 0 and facts["peaks"][0] <= 20
        bboxes, scores, gboxes, cxs, cys, cscores = ref["snap"]
        assert (cscores >= 0.3).all()
        # corners beyond the cap lie inside cells: with a larger K the result could differ
        dropped = peaks[1][0][od.K_CORNERS:]
        inside = 0
        for c in facts["cells"]:
            cy, cx = divmod(int(c), W)
            inside += int(((np.abs(dropped // W - cy) < 12) & (np.abs(dropped % W - cx) < 12)).sum())
        assert inside >= 5, inside
        assert n >= 1
    elif name.startswith("overflow"):
        cls = facts["cls"]
        assert facts["peaks"][cls] == 17368 > HEAT_CAP
        K = od.K_CORNERS if cls else od.K_CELLS
        want = np.concatenate([facts["first"], np.arange(K - 5)])
        assert np.array_equal(peaks[cls][0][:K], want)
        if cls == 0:
            assert n == od.K_CELLS
        else:
            assert n >= 5 and (ref["snap"][5] >= 0.3).all()
    elif name.startswith("rim"):
        assert W % 2 == 1
        for cls in range(2):
            assert set(peaks[cls][0].tolist()) == set(facts["pixels"].tolist())
        s = torch.sigmoid(torch.from_numpy(heads["hm"]))[0].numpy().reshape(2, -1)
        p = facts["pixels"]
        assert p[9] == p[8] + 1 and p[11] == p[10] + 1           # memory neighbours ...
        assert (s[:, p[9]] > s[:, p[8]]).all() and (s[:, p[10]] > s[:, p[11]]).all()
        assert n == 12
    elif name.startswith("outside"):
        b = torch.from_numpy(raw[:n, :8].copy())
        if rev:         # the corner pixels are taken from the rows in their order before the re-sort: the same set of rows
            assert n == facts["peaks"][0]
        xs, ys = b[:, 0::2], b[:, 1::2]
        cc = torch.round(xs + W * torch.round(ys)).to(torch.int64).numpy()
        x_out = (xs.numpy() < -0.5) | (xs.numpy() >= W - 0.5)
        assert (cc < 0).sum() >= facts["min_neg"] and (cc >= H * W).sum() >= facts["min_past"]
        assert (x_out & (cc >= 0) & (cc < H * W)).sum() >= facts["min_wrap"]
    elif name == "rounds":
        bboxes, scores, gboxes, cxs, cys, cscores = ref["snap"]
        ncorner = int((cscores >= 0.3).sum())
        assert ncorner == facts["peaks"][1] > 64 * 3
        cell_pix = peaks[0][0]
        hits = {int(cell_pix[i]): [j for j in range(ncorner) if od.is_group(bboxes[i], gboxes[j])] for i in range(len(cell_pix))}
        for c in facts["big"]:
            h = hits[int(c)]
            assert len(h) >= 150 and max(h) // 64 - min(h) // 64 >= 2, (c, len(h))
        assert len(hits[int(facts["two"])]) == 2 and len(hits[int(facts["three"])]) == 3
        s0 = dict(zip(peaks[0][0].tolist(), peaks[0][1].tolist()))
        final = sorted(raw[:7, 8].tolist())
        assert any(abs(f - np.float32(s0[int(facts["two"])]) * np.float32(0.4)) < 1e-7 for f in final)
        assert any(f == np.float32(s0[int(facts["three"])]) for f in final)


def _seams_lie_inside_workgroups(facts, npix, wg=1024):
    """every seam s = t * npix lies strictly inside a workgroup of the peak kernel (batch-flat pixel index // 1024), and the seam peaks of
    the table before it (table 0) or after it (table 2) sit in that very workgroup, together with pixels of the empty middle table"""
    for t in (1, 2):
        s = t * npix
        assert s % wg != 0
        own = 0 if t == 1 else 2
        flat = own * npix + facts["tables"][own]["seam"]
        assert len(flat) == 8 and (flat // wg == s // wg).all(), (t, flat)


def test_lore_seam_case_exercises_its_edge():
    tables, facts, refs = E.lore_seam_case()
    npix = facts["npix"]
    assert len(tables) == 3 and npix >= od.K_CORNERS and npix % 1024 == 64
    _seams_lie_inside_workgroups(facts, npix)
    for t, (h, f, r) in enumerate(zip(tables, facts["tables"], refs)):
        peaks = _lore_peaks(h)
        _check_common(peaks, f)
        got = set(peaks[0][0].tolist()) | set(peaks[1][0].tolist())
        assert set(f["seam"].tolist()) <= got
        if t == 0:
            assert (f["seam"] >= npix - 64).all()
        elif t == 2:
            assert (f["seam"] < 64).all()
        assert (r["n"] == 0) == (t == 1)


@pytest.mark.parametrize("name", list(E.CN_CASES))
def test_centernet_case_exercises_its_edge(name):
    (heads, (cw, ch)), facts, ref = E.cn_case(name)
    H, W = heads["hm"].shape[2:]
    assert H <= 144 and W <= 144
    peaks = _cn_peaks(heads)
    _check_common(peaks, facts, ties=name in ("ties", "overflow"))
    if name == "ties":
        for cls in range(2):
            assert np.array_equal(peaks[cls][0], facts["order"][cls])
            assert (peaks[cls][1][:36] == 1.0).all() and len(np.unique(peaks[cls][1][-64:])) == 1
        assert len(ref) == facts["peaks"][0]
    elif name == "cap_verts":
        assert facts["peaks"][1] > R.K_VERT and 25 <= len(ref) <= 35
        # vertices claim corners: the grouping is not idle
        q = R.centernet_cells({**heads, "hm": np.concatenate([heads["hm"][:, :1], np.full_like(heads["hm"][:, 1:], -20.0)], 1)}, cw, ch)
        assert (q[:, :8] != ref[:, :8]).any(1).sum() >= 5
    elif name == "overflow":
        assert facts["peaks"][0] == 17368 > HEAT_CAP
        assert np.array_equal(peaks[0][0][:R.K_CELL], np.concatenate([facts["first"], np.arange(R.K_CELL - 5)]))
        assert len(ref) == R.K_CELL
    elif name == "rim":
        assert W % 2 == 1 and (H, W) == (40, 33)
        for cls in range(2):
            assert set(peaks[cls][0].tolist()) == set(facts["pixels"].tolist())
        assert len(ref) == 12
    elif name == "rounds":
        from pdf_table_amd.centernet_stage import centernet_decode_affine
        assert np.array_equal(peaks[1][0], facts["vertex_order"])
        r = facts["ranks"]
        assert len({x // 64 for x in (r[1] if 8 in r else 10, 70, 130, 200)}) == 4
        k = int(np.where(peaks[0][0] == facts["q_pixel"])[0][0])
        assert np.array_equal(ref[k, :8], facts["q_corners"]), (ref[k, :8], facts["q_corners"])
        d = int(np.where(peaks[0][0] == facts["degenerate_pixel"])[0][0])
        assert len(np.unique(ref[d, 0:8:2])) == 1 and len(np.unique(ref[d, 1:8:2])) == 1          # still its own point: nothing claimed
        if 8 in r:
            assert np.array_equal(centernet_decode_affine(H, W, H, W), np.array([[1.0, 0, 0], [0, 1.0, 0]]))


def test_centernet_seam_case_exercises_its_edge():
    cases, facts, refs = E.cn_seam_case()
    npix = facts["npix"]
    assert len(cases) == 3
    _seams_lie_inside_workgroups(facts, npix)
    for t, ((h, _), f, r) in enumerate(zip(cases, facts["tables"], refs)):
        peaks = _cn_peaks(h)
        _check_common(peaks, f)
        assert set(f["seam"].tolist()) <= set(peaks[0][0].tolist()) | set(peaks[1][0].tolist())
        assert (len(r) == 0) == (t == 1)
