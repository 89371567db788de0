"""pt_docx_decode (csrc/docx_decode.hip) on seeded head maps (tests/docxlayout_synth.py): counts, pixel indices, classes, arg-max columns and
keep flags EQUAL to the reference's fixture and to the CPU restatement, coordinates bit-equal, scores within 4 x the largest difference
between torch's float32 sigmoid and a float64 sigmoid on the test's own logits (the rule of tests/layout_decode_ref.py; the figure is
printed).  Tie cases are held to the engine's stated rule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docxlayout_ref as R  # noqa: E402
import docxlayout_synth as S  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

K = 100
CANARY = 0x5A


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def post(golden_dir):
    return np.load(os.path.join(golden_dir, "docxlayout_post.npz"))


def _nhwc(t, cs):
    n, c, h, w = t.shape
    o = torch.full((n, h, w, cs), -77.0)      # padding channels hold a value that would be a peak nowhere and a wrong corner everywhere
    o[..., :c] = torch.from_numpy(t).permute(0, 2, 3, 1)
    return o.contiguous()


def _device_heads(z):
    return {k: _nhwc(v, 16 if k == "hm" else 8).cuda() for k, v in z.items()}


def _sig_bound(z):
    worst = 0.0
    for k in ("hm", "hm_sub"):
        x = torch.from_numpy(np.ascontiguousarray(z[k]))
        worst = max(worst, float((torch.sigmoid(x).double() - torch.sigmoid(x.double())).abs().max()))
    return 4.0 * worst


def _run(eng, z, k=K):
    """one call with canary bytes behind every output -> numpy (counts [n,2], recs [n,2,k,12], inds [n,2,k], keep [n,2,k])"""
    n = z["hm"].shape[0]
    heads = _device_heads(z)
    pad = 64
    bufs = [torch.full((n * 2 * m + pad,), CANARY, dtype=torch.uint8, device="cuda") for m in (4, k * 12 * 4, k * 4, k)]
    out = (bufs[0][:n * 8].view(torch.int32).view(n, 2), bufs[1][:n * 2 * k * 48].view(torch.float32).view(n, 2, k, 12),
           bufs[2][:n * 2 * k * 4].view(torch.int32).view(n, 2, k), bufs[3][:n * 2 * k].view(n, 2, k))
    res = []
    for _ in range(2):      # a second call on the same buffers gives the same bytes
        eng.docx_decode(heads, top_k=k, out=out)
        torch.cuda.synchronize()
        res.append([b.cpu().numpy().copy() for b in bufs])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for b, m in zip(res[0], (4, k * 12 * 4, k * 4, k)):
        assert (b[n * 2 * m:] == CANARY).all(), "write behind an output"
    return tuple(o.cpu().numpy() for o in out)


def _check_page(got, i, z, j, bound, tag):
    """page i of the device's outputs against the restatement of page j of z: everything equal, scores within the bound; returns the rows"""
    counts, recs, inds, keep = got
    rows = []
    for b, (rec, idx) in enumerate((R.branch_list(z["hm"][j], z["wh"][j], z["reg"][j], z["cls"][j], z["ftype"][j]),
                                    R.branch_list(z["hm_sub"][j], z["wh_sub"][j], z["reg_sub"][j]))):
        m = int(counts[i, b])
        assert m == len(rec), (tag, b, m, len(rec))
        g = recs[i, b, :m]
        assert np.array_equal(inds[i, b, :m], idx), (tag, b, "pixel indices")
        assert np.array_equal(g[:, :8].view(np.uint32), rec[:, :8].view(np.uint32)), (tag, b, "coordinates")
        assert np.array_equal(g[:, 9:], rec[:, 9:]), (tag, b, "class / arg-max columns")
        assert np.abs(g[:, 8].astype(np.float64) - rec[:, 8]).max(initial=0.0) <= bound, (tag, b, "scores")
        assert np.array_equal(keep[i, b, :m] != 0, R.pnms_keep(rec)), (tag, b, "keep flags")
        rows.append(g[keep[i, b, :m] != 0])
    return rows


@pytest.mark.parametrize("size", S.SIZES)
def test_decode_matches_reference_fixture_and_restatement(eng, post, size):
    """B = 4 in one call, an empty page among them, border peaks on page 0 and on the last page"""
    cases = ["borders", "empty", "many", "nms"]
    z = S.stack(cases, size)
    bound = _sig_bound(z)
    got = _run(eng, z)
    print(f"docx decode {size}: score bound {bound:.3e}")
    worst = 0.0
    for i, case in enumerate(cases):
        tag = f"{case}_{size[0]}x{size[1]}"
        _check_page(got, i, z, i, bound, tag)
        counts, recs, _, keep = got
        for b, name in enumerate(("main", "sub")):
            ref = post[f"dets_{name}_{tag}"]
            ref = ref[ref[:, 8] >= R.THR_LO]
            m = int(counts[i, b])
            assert m == len(ref), (tag, name)
            g = recs[i, b, :m].copy()
            g[:, 9] += 11 * b
            ncol = 12 if b == 0 else 10
            assert np.array_equal(g[:, :8].view(np.uint32), ref[:, :8].view(np.uint32)) and np.array_equal(g[:, 9:ncol], ref[:, 9:ncol]), (tag, name)
            worst = max(worst, float(np.abs(g[:, 8].astype(np.float64) - ref[:, 8]).max(initial=0.0)))
            kept = post[f"kept_{name}_{tag}"]
            mine = g[keep[i, b, :m] != 0]
            assert len(mine) == len(kept) and np.array_equal(mine[:, :8].view(np.uint32), kept[:, :8].view(np.uint32)), (tag, name, "pnms")
    print(f"docx decode {size}: largest score difference to the reference {worst:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("size", S.SIZES)
def test_decode_second_batch_and_host_chain(eng, golden_dir, size):
    """the fifth reference case beside the tie pages; the device's kept rows through the product's host half give the reference's final list"""
    import json
    from pdf_table_amd.docxlayout_stage import docx_page_result
    cases = ["few", "flat", "plateau", "borders"]
    z = S.stack(cases, size)
    bound = _sig_bound(z)
    got = _run(eng, z)
    with open(os.path.join(golden_dir, "docxlayout_post.json")) as f:
        js = json.load(f)
    for i in (0, 3):
        tag = f"{cases[i]}_{size[0]}x{size[1]}"
        rows = _check_page(got, i, z, i, bound, tag)
        res = docx_page_result(rows[0], rows[1], S.page_hw(size), size)
        want = js[tag]
        assert len(res) == len(want), tag
        for g, w in zip(res, want):
            assert [float(v) for v in g["bbox"]] == w["bbox"] and g["label"] == w["label"] and float(g["score"]) == w["score"], (tag, g, w)


def test_decode_tie_rules(eng):
    """plateau, equal scores, equal arg-max maxima, the flat map, the two logits around 0.3: the engine's stated rule"""
    size = S.SIZES[0]
    h, w = size
    cases = ["plateau", "equal_pair", "argmax_tie", "flat", "threshold"]
    z = S.stack(cases, size)
    counts, recs, inds, keep = _run(eng, z)
    # plateau: all four pixels are peaks, in index order
    assert counts[0].tolist() == [4, 4]
    assert inds[0, 0, :4].tolist() == [3 * h * w + y * w + x for y in (5, 6) for x in (9, 10)]
    assert inds[0, 1, :4].tolist() == [1 * h * w + y * w + x for y in (2, 3) for x in (2, 3)]
    assert keep[0, :, :4].all()
    # equal scores: both listed in index order, neither suppressed although each holds the other's centre
    assert counts[1].tolist() == [2, 0] and inds[1, 0, :2].tolist() == [5 * h * w + 9 * w + 8, 5 * h * w + 9 * w + 11]
    assert recs[1, 0, 0, 8] == recs[1, 0, 1, 8] and keep[1, 0, :2].tolist() == [1, 1]
    # equal arg-max maxima: the first wins
    assert counts[2].tolist() == [1, 0] and recs[2, 0, 0, 9:].tolist() == [6.0, 1.0, 0.0]
    # flat: every value is a peak (h * w * 11 of them); the list is the first K flat indices
    assert counts[3].tolist() == [K, K]
    assert inds[3, 0].tolist() == list(range(K)) and inds[3, 1].tolist() == list(range(K))
    assert (recs[3, 0, :, 9] == 0).all() and keep[3].all()
    # around 0.3: both logits are listed (thr_lo = 0.3 - 1e-3); a row is kept by the NMS exactly when its own score is not below 0.3 as a double
    assert counts[4].tolist() == [2, 2]
    for b in range(2):
        sc = recs[4, b, :2, 8].astype(np.float64)
        assert sc[0] >= sc[1] and abs(sc[0] - 0.3) < 1e-6 and abs(sc[1] - 0.3) < 1e-6
        assert keep[4, b, :2].tolist() == [int(not v < 0.3) for v in sc]
    # the same pages through the restatement, where it has a rule of its own (index order among equal scores)
    for i, case in enumerate(cases[:4]):
        _check_page((counts, recs, inds, keep), i, z, i, _sig_bound(z), case)


def test_decode_flat_map_full_size(eng):
    """192 x 192 x 11 equal values: the radix-select path at the model's own map size, K = 100 and K = 128"""
    z = {k: np.zeros((1, c, 192, 192), np.float32) for k, c in R.HEADS.items()}
    z["hm"][0, :, 100, 100] = 1.0      # one larger value per class: ranks 0 .. 10, then the flat rest in index order
    for k in (100, 128):
        counts, recs, inds, keep = _run(eng, z, k)
        assert counts[0].tolist() == [k, k]
        top = [c * 192 * 192 + 100 * 192 + 100 for c in range(11)]
        rest = [i for i in range(k + 9) if i not in top and not _near(i, 100, 100)]
        assert inds[0, 0].tolist() == top + rest[:k - 11]
        assert inds[0, 1].tolist() == list(range(k))


def _near(i, y, x, w=192):
    """flat index i (class 0) is a 3 x 3 neighbour of (y, x): not a peak beside the larger value"""
    py, px = (i % (w * w)) // w, i % w
    return abs(py - y) <= 1 and abs(px - x) <= 1


def test_decode_refuses_out_of_range_arguments(eng):
    z = S.stack(["empty"], S.SIZES[0])
    heads = _device_heads(z)
    out = eng.docx_decode(heads)
    torch.cuda.synchronize()
    before = [o.clone() for o in out]
    for kw in ({"top_k": 129}, {"top_k": 0}, {"ncls_main": 17}, {"ncls_sub": 9}):
        with pytest.raises(L.PtError, match="pt_docx_decode"):
            eng.docx_decode(heads, out=out, **kw)
    big = {k: torch.zeros((1, 513, 8, 16 if k == "hm" else 8), device="cuda") for k in R.HEADS}
    with pytest.raises(L.PtError, match="512"):
        eng.docx_decode(big)
    torch.cuda.synchronize()
    for a, b in zip(before, out):
        assert torch.equal(a, b)      # nothing was launched
