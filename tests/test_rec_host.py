"""Recognition stage, CPU side: oracle pinned to the reference CRNN golden; product host geometry (vectorised) against
the oracle's literal restatement and the reference's own order_point outputs."""
import os

import numpy as np
import pytest
import torch

from oracle import crnn as ocrnn
from pdf_table_amd import rec_stage as R
from pdf_table_amd.synth_weights import crnn_state_dict


def test_oracle_crnn_matches_reference_module(golden_dir):
    """run in float64 like the reference module that produced the golden: in float32 the difference is the two CPUs' summation orders
    (thread count, ISA), which on another machine crosses these bounds"""
    g = np.load(os.path.join(golden_dir, "crnn.npz"))
    sd = {k: v.double() if v.is_floating_point() else v for k, v in crnn_state_dict(int(g["seed"])).items()}
    with torch.no_grad():
        y = ocrnn.crnn_forward_fp32(sd, torch.from_numpy(g["x"]).double()).numpy()
    np.testing.assert_allclose(y[:, :, ::16], g["logits_sub"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(y.max(-1), g["maxval"], rtol=0, atol=2e-5)
    np.testing.assert_array_equal(y.argmax(-1), g["argmax"])


def test_order_points_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "db_host_numpy.npz"))
    got = R.order_points(g["order_point_in"])
    np.testing.assert_array_equal(got, g["order_point_out"])
    for row, ref in zip(g["order_point_in"], g["order_point_out"]):
        np.testing.assert_array_equal(ocrnn.order_point(row), ref)


def _random_quads(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = rng.uniform(50, 900, 2)
        wh = rng.uniform([20, 8], [400, 40])
        ang = rng.uniform(-0.3, 0.3)
        Rm = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        q = (np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]]) * wh / 2) @ Rm.T + c
        out.append(np.round(q[rng.permutation(4)]).reshape(-1))
    return np.array(out, dtype=np.float64)


def test_crop_geometry_and_matrix_match_oracle():
    quads = _random_quads(60, 5)
    pts = R.order_points(quads)
    src, dst, ow, oh = R.crop_geometry(pts)
    minv = R.perspective_inverse(src, dst)
    for i in range(len(quads)):
        s2, d2, w2, h2 = ocrnn.crop_geometry(ocrnn.order_point(quads[i]))
        np.testing.assert_array_equal(src[i], s2)
        np.testing.assert_array_equal(dst[i], d2)
        assert (ow[i], oh[i]) == (w2, h2)
        m = np.linalg.inv(ocrnn.get_perspective_transform(s2, d2)).reshape(-1)
        np.testing.assert_array_equal(minv[i], m)


def test_build_lines_layout():
    boxes = [_random_quads(3, 1), np.zeros((0, 8)), _random_quads(2, 2)]
    lines = R.build_lines(boxes)
    assert lines.dtype.itemsize == 88 and len(lines) == 5
    assert lines["page"].tolist() == [0, 0, 0, 2, 2]
    assert (lines["crop_w"] > 0).all() and (lines["crop_h"] > 0).all()


def test_ctc_collapse_matches_oracle():
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 4, (20, 160)).astype(np.int32)
    ids[3] = 0
    ids[4] = 7
    assert R.ctc_collapse(ids) == ocrnn.ctc_greedy_ids(ids)
    assert R.ctc_collapse(ids)[3] == [] and R.ctc_collapse(ids)[4] == [7]


def test_warp_oracle_known_answers():
    # identity-like crop of an axis-aligned box on a smooth ramp: values follow the ramp at the mapped positions
    yy, xx = np.mgrid[0:120, 0:300]
    img = np.stack([xx * 0.5 + 20, yy * 1.0 + 10, (xx + yy) * 0.3], -1).astype(np.uint8)
    quad = np.array([[40, 30], [240, 30], [240, 70], [40, 70]], np.float32)
    crop = ocrnn.crop_image(img, ocrnn.order_point(quad))
    assert crop.shape == (40, 200, 3)
    # dst x in [0,199] maps to src x = 40 + x*200/199
    xs = 40 + np.arange(200) * 200 / 199
    assert np.abs(crop[0, :, 0].astype(float) - (xs * 0.5 + 20)).max() <= 1.0
    assert np.abs(crop[:, 0, 1].astype(float) - ((30 + np.arange(40) * 40 / 39) + 10)).max() <= 1.0
    # keep-ratio resize + pad: width = int(32 * 200 / 40) = 160, zeros beyond
    m = ocrnn.keepratio_resize(crop)
    assert m.shape == (32, 640, 3) and (m[:, 160:] == 0).all() and m[:, :160].any()
