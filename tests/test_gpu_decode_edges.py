"""The two heat-map decodes (pt_tsr_decode, pt_centernet_decode) at the inputs where order-dependent integer kernels go wrong: equal
scores, the top-K caps really exceeded, more peaks than the candidate buffer holds, peaks on the rim and across the row wrap, table
seams inside a workgroup, corner pixels outside the map, more hits than one 64-lane round.  Inputs: tests/decode_edge_synth.py; references:
tests/decode_edge_ref.py (tests/test_decode_edges_host.py asserts on the CPU that every case exercises its edge).

Pass criteria, those of test_gpu_tsr.py / test_gpu_centernet.py: Lore dets[:, :8] and the logic features bit-equal to the oracle, scores
within 1e-6, count equal; CenterNet the same cells in the same order, coordinates within 1e-3 px, count equal to centernet_cells."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import centernet_ref as R  # noqa: E402
import decode_edge_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu

HEAT_CAP = 16384          # PT_HEAT_CAP, pdf_table_amd/csrc/common.h: the overflow cases hold more peaks per list than this


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _nhwc(t, cs):
    n, c, h, w = t.shape
    o = torch.zeros(n, h, w, cs)
    o[..., :c] = torch.from_numpy(t).permute(0, 2, 3, 1)
    return o.cuda()


def _lore_decode(eng, tables, rev):
    dev = {k: _nhwc(np.concatenate([h[k] for h in tables]), 256 if k in ("ax", "cr") else 8) for k in tables[0]}
    counts, dets, lg = eng.tsr_decode(dev, wiz_rev=rev, vis_thresh=0.2)
    torch.cuda.synchronize()
    return counts, dets.cpu().numpy(), lg.cpu().numpy()


def _lore_equal(counts, dets, lg, b, ref, tag):
    n = ref["n"]
    assert counts[b] == n, (tag, counts[b], n)
    d, raw = dets[b, :n], ref["raw"]
    assert np.array_equal(d[:, :8], raw[:n, :8]), (tag, np.abs(d[:, :8] - raw[:n, :8]).max(initial=0.0))
    assert np.allclose(d[:, 8], raw[:n, 8], atol=1e-6, rtol=0), tag
    assert np.array_equal(lg[b, :n], ref["logi"]), tag


def _cn_decode(eng, cases):
    from pdf_table_amd.centernet_stage import centernet_decode_affine
    heads = {k: torch.cat([_nhwc(h[k], 8) for h, _ in cases]) for k in R.HEADS}
    H, W = cases[0][0]["hm"].shape[2:]
    aff = np.stack([centernet_decode_affine(ch, cw, H, W) for _, (cw, ch) in cases])
    counts, cells = eng.centernet_decode(heads, aff)
    torch.cuda.synchronize()
    return counts, cells.cpu().numpy()


def _cn_equal(counts, cells, b, ref, tag):
    from pdf_table_amd.centernet_stage import centernet_order
    assert counts[b] == len(ref), (tag, counts[b], len(ref))
    got = cells[b, :counts[b]]
    assert np.abs(got[:, :8] - ref[:, :8]).max(initial=0.0) <= 1e-3, tag              # row by row: the top-K order
    assert np.abs(got[:, 8] - ref[:, 8]).max(initial=0.0) <= 1e-6, tag
    a, r = centernet_order(got), centernet_order(ref)
    assert a.shape == r.shape and np.abs(a - r).max(initial=0.0) <= 1e-3, tag


@pytest.mark.parametrize("name", [n for n in E.LORE_CASES if not n.startswith("overflow")])
def test_tsr_decode_edge_matches_oracle(eng, name):
    """ties (a), caps exceeded (b), rim and row wrap (d), corner pixels outside the map (f), several 64-corner rounds (g)"""
    heads, facts, rev, ref = E.lore_case(name)
    counts, dets, lg = _lore_decode(eng, [heads], rev)
    _lore_equal(counts, dets, lg, 0, ref, name)


@pytest.mark.parametrize("name", ["overflow_cells", "overflow_corners"])
def test_tsr_decode_more_peaks_than_the_candidate_buffer(eng, name):
    """(c) 17368 peaks in one list: the first K in (score desc, index asc) order whatever the order of the appends -- two decodes, the
    same bits, the reference's rows"""
    heads, facts, rev, ref = E.lore_case(name)
    assert facts["peaks"][facts["cls"]] > HEAT_CAP
    c1, d1, l1 = _lore_decode(eng, [heads], rev)
    c2, d2, l2 = _lore_decode(eng, [heads], rev)
    n = ref["n"]
    assert c1[0] == c2[0] == n, (c1, c2, n)
    assert np.array_equal(d1[0, :n], d2[0, :n]) and np.array_equal(l1[0, :n], l2[0, :n]), "two decodes of one map differ"
    _lore_equal(c1, d1, l1, 0, ref, name)


def test_tsr_decode_table_seams_inside_a_workgroup(eng):
    """(e) three 72 x 72 tables (5184 % 1024 = 64), the middle one empty, peaks in the last / first 64 pixels around it: every table
    equals its solo decode bit for bit, and the oracle"""
    tables, facts, refs = E.lore_seam_case()
    counts, dets, lg = _lore_decode(eng, tables, True)
    for b, (h, ref) in enumerate(zip(tables, refs)):
        c1, d1, l1 = _lore_decode(eng, [h], True)
        n = ref["n"]
        assert counts[b] == c1[0] == n, (b, counts[b], c1[0], n)
        assert np.array_equal(dets[b, :n], d1[0, :n]) and np.array_equal(lg[b, :n], l1[0, :n]), b
        _lore_equal(counts, dets, lg, b, ref, f"seam table {b}")


@pytest.mark.parametrize("name", [n for n in E.CN_CASES if n != "overflow"])
def test_centernet_decode_edge_matches_reference(eng, name):
    """ties (a), the vertex cap exceeded (b), rim and row wrap on a 40 x 33 map (d), claims from four 64-vertex rounds, a contested corner,
    a degenerate cell and the 2-px pointer rule at exactly 2.0 px (g)"""
    case, facts, ref = E.cn_case(name)
    counts, cells = _cn_decode(eng, [case])
    _cn_equal(counts, cells, 0, ref, name)
    if name == "rounds":          # the claims are exact copies of vertex positions
        k = int(np.where(np.all(ref[:, :8] == facts["q_corners"], 1))[0][0])
        assert np.array_equal(cells[0, k, :8], facts["q_corners"])


def test_centernet_decode_more_peaks_than_the_candidate_buffer(eng):
    """(c) class 0 flat at logit 2.0 on 136 x 128 (17368 peaks) under five higher peaks late in the map: they come first, then pixels
    0, 1, 2, ...; two decodes, the same bits"""
    case, facts, ref = E.cn_case("overflow")
    assert facts["peaks"][0] > HEAT_CAP
    c1, cells1 = _cn_decode(eng, [case])
    c2, cells2 = _cn_decode(eng, [case])
    assert c1[0] == c2[0] == len(ref), (c1, c2, len(ref))
    assert np.array_equal(cells1[0, :c1[0]], cells2[0, :c2[0]]), "two decodes of one map differ"
    _cn_equal(c1, cells1, 0, ref, "overflow")


def test_centernet_decode_table_seams_inside_a_workgroup(eng):
    """(e) three 24 x 40 tables (960 pixels each: both seams lie inside a workgroup of 1024, next to the peaks at the end of table 0
    and at the start of table 2), the middle one empty: every table equals its solo decode bit for bit, and the reference"""
    cases, facts, refs = E.cn_seam_case()
    counts, cells = _cn_decode(eng, cases)
    for b, (case, ref) in enumerate(zip(cases, refs)):
        c1, solo = _cn_decode(eng, [case])
        assert counts[b] == c1[0] == len(ref), (b, counts[b], c1[0], len(ref))
        assert np.array_equal(cells[b, :counts[b]], solo[0, :c1[0]]), b
        _cn_equal(counts, cells, b, ref, f"seam table {b}")
