"""CPU-side proof that the cases of tests/preprocess_edge_synth.py exercise the edges they are named after, and that the comparisons
of tests/test_gpu_preprocess_edges.py would notice a kernel that is subtly wrong: the expected tensors are computed again with
deliberately wrong variants of the oracle (a wrong exact-2x branch, clamp-to-edge instead of the zero border, the page index ignored, the
crop bound ignored, rows read across the page seam, the offset scan's carry dropped after element 1023) and every variant must change at
least one value in the cases meant to catch it.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_edge_synth as S  # noqa: E402
from oracle import crnn, db_pre, rec_pp  # noqa: E402

BRANCHES = {"copy", "area2", "general"}


# ---- which branch every case takes --------------------------------------------------------------------------------------------------
def branch_table():
    """kernel -> [(case, source w x h, resized w x h, branch)]"""
    t = {}
    rows = []
    for cases in (S.REC_SMALL, S.REC_WIDE):
        for c in cases:
            _, cw, ch = S.line_geometry(c)
            nw = S.rec_nw(cw, ch, S.REC_W)
            rows.append((c[0], (cw, ch), (nw, S.REC_H), S.classify(cw, ch, nw, S.REC_H)))
    t["rec_resize_gray_kernel (640)"] = rows
    names, crops, _ = S.cvit_case()
    t["rec_resize_gray_kernel (804, fp32)"] = [
        (n, (c.shape[1], c.shape[0]), (S.rec_nw(c.shape[1], c.shape[0], S.CVIT_W), S.REC_H),
         S.classify(c.shape[1], c.shape[0], S.rec_nw(c.shape[1], c.shape[0], S.CVIT_W), S.REC_H)) for n, c in zip(names, crops)]
    rows = []
    for tag, names, crops in (("crops", [s[0] for s in S.PP_SIZES], S.pp_crops_case()[0]), ("page", [c[0] for c in S.PP_PAGE], S.pp_page_case()[0])):
        for n, c, (rw, _) in zip(names, crops, S.pp_resized(crops)):
            rows.append((f"{tag}:{n}", (c.shape[1], c.shape[0]), (rw, S.PP_H), S.classify(c.shape[1], c.shape[0], rw, S.PP_H)))
    t["rec_pp_resize_norm_kernel"] = rows
    t["mtl_preprocess_kernel"] = [(n, (x2 - x1, y2 - y1), S.mtl_nwh(x2 - x1, y2 - y1), S.classify(x2 - x1, y2 - y1, *S.mtl_nwh(x2 - x1, y2 - y1)))
                                  for n, _, (x1, y1, x2, y2) in S.MTL_BOXES + S.MTL_FLAT]
    rows = []
    for c in S.DET_CASES:
        nh, nw = S.det_plan(c)
        h, w = c[2]
        rows.append((c[0], (w, h), (nw, nh), S.classify(w, h, nw, nh)))
    t["det_preprocess_kernel"] = rows
    return t


def test_every_resize_kernel_meets_its_three_branches():
    table = branch_table()
    for kernel, rows in table.items():
        print(kernel)
        for name, src, dst, br in rows:
            print(f"  {name}: {src[0]} x {src[1]} -> {dst[0]} x {dst[1]}: {br}")
        assert BRANCHES <= {r[3] for r in rows}, (kernel, {r[3] for r in rows})
    by = {k: {r[0]: r[3] for r in rows} for k, rows in table.items()}
    rec = by["rec_resize_gray_kernel (640)"]
    assert rec["copy_40x32"] == "copy" and rec["area2_100x64"] == rec["area2_120x64"] == rec["area2_1280x64"] == "area2"
    assert rec["off_copy_40x33"] == rec["off_area2_100x63"] == rec["cut_641x32"] == "general"
    assert rec["nw0_1x64"] == rec["zero_size"] == "empty"
    cv = by["rec_resize_gray_kernel (804, fp32)"]
    assert cv["area2_1280x64_crop"] == cv["area2_1608x64_crop"] == "area2" and cv["cut_805x32_crop"] == "general" and cv["nw0_1x64_crop"] == "empty"
    det = by["det_preprocess_kernel"]
    assert det["layout_w2x_only"] == "general" and det["layout_area2_64"] == det["layout_area2_1600x1216"] == "area2" and det["none_32x64"] == "copy"
    mtl = by["mtl_preprocess_kernel"]
    assert mtl["copy_48x48"] == "copy" and mtl["area2_96x96"] == "area2" and mtl["flat_1000x3"] == "general"
    assert S.mtl_nwh(1000, 3) == (48, 1) and int(48 / 1000 * 3) == 0          # the resized height clamps from 0 to 1


def test_narrow_detector_pages_take_the_byte_path_for_every_pixel():
    """det_preprocess_kernel reads two neighbouring pixels with one 8-byte load unless the window would end past the row (3 * s0 + 8 >
    3 * w): pages 1 or 2 pixels wide take byte loads everywhere, and a 1-pixel page has s0 == s1"""
    for c in S.DET_CASES:
        (h, w), (nh, nw) = c[2], S.det_plan(c)
        if w > 2:
            continue
        s0, s1, _, _ = db_pre._coef(nw, w, True)
        assert (3 * s0 + 8 > 3 * w).all(), c[0]
        if w == 1:
            assert (s0 == s1).all() and (s0 == 0).all()
    widths = {c[2][1] for c in S.DET_CASES}
    assert {1, 2, 3, 5} <= widths


def test_scan_case_is_longer_than_one_chunk_and_neighbours_differ():
    cases, crops, gray = S.many_expected()
    assert len(cases) == S.MANY > 1024
    px = [c.shape[0] * c.shape[1] for c in crops]
    assert all(a != b for a, b in zip(px, px[1:]))
    assert all(2 <= c.shape[1] <= 9 and 2 <= c.shape[0] <= 5 for c in crops)
    assert {c[1] for c in cases} == {0, 1}
    assert all(S.rec_nw(c.shape[1], c.shape[0], S.REC_W) <= S.MANY_KEEP_W for c in crops)
    assert bool((gray.flatten(1).abs().max(1).values > 0).all())


# ---- the cases hold what their names say -----------------------------------------------------------------------------------------------
def test_overhanging_lines_hold_border_and_page_pixels():
    crops, gray = S.rec_small()
    names = [c[0] for c in S.REC_SMALL]
    for n in S.OVERHANG:
        c = crops[names.index(n)]
        zero = (c == 0).all(2)
        assert zero.any() and (~zero).any(), n
        assert 0.02 < zero.mean() < 0.6, (n, zero.mean())
    for n in S.ALL_ZERO:
        assert float(gray[names.index(n)].abs().max()) == 0.0, n
    for n in ("before_nw0", "after_nw0", "after_zero_size"):
        assert float(gray[names.index(n)].abs().max()) > 0.0, n
    _, _, cv = S.cvit_case()
    cn = S.cvit_case()[0]
    for n in ("nw0_1x64_crop", "zero_size", "outside"):
        assert float(cv[cn.index(n)].abs().max()) == 0.0, n
    assert float(cv[cn.index("after_crop")].abs().max()) > 0.0


def test_letterboxed_table_crops_are_mostly_border():
    for bgr in (True, False):
        x = S.lore_case(bgr)
        names = [b[0] for b in S.LORE_BOXES]
        z = S.lore_zero_pixel(bgr)
        for n in ("thin_3x90", "flat_90x3"):
            border = (x[names.index(n)] == z).all(-1)
            assert 0.8 < border.mean() < 1.0, (n, border.mean())
        assert not (x[names.index("whole_page")] == z).all(-1).all()


def test_mtl_cases_pad_and_sizes():
    x, sizes = S.mtl_case()
    xf, sf = S.mtl_flat_case()
    assert sf == [(48, 1), (48, 1)]
    assert (xf[:, 1:] == -1.0).all() and (xf[:, 0] != -1.0).any()
    for (n, _, (x1, y1, x2, y2)), (nw, nh), im in zip(S.MTL_BOXES, sizes, x):
        assert (nw, nh) == S.mtl_nwh(x2 - x1, y2 - y1)
        assert (im[nh:] == -1.0).all() and (im[:, nw:] == -1.0).all(), n


def test_pp_mini_batches_of_three_share_a_width():
    crops, ref = S.pp_crops_case()
    items, batches, total = S.pp_plan(crops)
    assert [b[1] for b in batches] == [3, 3, 2]
    for (beg, n, img_w, off), r in zip(batches, ref):
        assert r["image"].shape == (n, 3, S.PP_H, img_w)
        rw = items["resized_w"][beg:beg + n]
        assert n < 3 or len(set(rw.tolist())) == 3, rw               # three different resized widths under one padded width
        for k in range(n):
            assert (r["image"][k, :, :, rw[k]:] == 0).all()
    ends = [off + n * 3 * S.PP_H * w for _, n, w, off in batches]
    assert batches[0][3] == S.GUARD and all(b[3] - e == S.GUARD for b, e in zip(batches[1:], ends)) and total - ends[-1] == S.GUARD


# ---- sensitivity: wrong variants of the oracle ------------------------------------------------------------------------------------------
def _resize_without_area(img, nw, nh, trunc_area=False):
    """cv2_resize_linear_u8 without the switch to INTER_AREA at exact 2x; trunc_area: with the switch, but the 2 x 2 mean truncated
    instead of rounded"""
    h, w, _ = img.shape
    if (h, w) == (nh, nw):
        return img.copy()
    src = img.astype(np.int64)
    if trunc_area and w == 2 * nw and h == 2 * nh:
        return ((src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2]) >> 2).astype(np.uint8)
    x0, x1, ax0, ax1 = db_pre._coef(nw, w, True)
    y0, y1, ay0, ay1 = db_pre._coef(nh, h, False)
    hor = src[:, x0, :] * ax0[None, :, None] + src[:, x1, :] * ax1[None, :, None]
    out = (((ay0[:, None, None] * (hor[y0] >> 4)) >> 16) + ((ay1[:, None, None] * (hor[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def _differs(a, b):
    return not np.array_equal(np.asarray(a), np.asarray(b))


def _warm():
    """the cached (right) expectations, computed before an oracle function is replaced"""
    S.rec_small(), S.rec_wide(), S.cvit_case(), S.pp_crops_case(), S.pp_page_case(), S.mtl_case(), S.mtl_flat_case()
    S.det_case("layout_area2_64"), S.det_case("layout_w2x_only")


def test_exact_2x_bilinear_equals_the_area_mean():
    """Dropping the 2x branch is NOT a wrong variant: at exactly 2x every fixed-point coefficient is 1024 / 2048 and no tap is clamped, so
    ((1024 * (S0 >> 4)) >> 16) + ((1024 * (S1 >> 4)) >> 16) + 2) >> 2 is the rounded 2 x 2 mean, bit for bit.  The branch can only be wrong in
    its own arithmetic or addressing, which is what the variant below models (a truncated mean)"""
    rng = np.random.default_rng(1)
    for h, w in ((64, 100), (2, 2), (96, 400)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(_resize_without_area(img, w // 2, h // 2), db_pre.cv2_resize_linear_u8(img, w // 2, h // 2))
    img = np.full((4, 4, 3), 255, np.uint8)
    assert np.array_equal(_resize_without_area(img, 2, 2), db_pre.cv2_resize_linear_u8(img, 2, 2))


def test_wrong_variant_area_branch(monkeypatch):
    _warm()
    good_det = S.det_case("layout_area2_64")[1], S.det_case("layout_w2x_only")[1]
    for mod in (crnn, db_pre, rec_pp):
        monkeypatch.setattr(mod, "cv2_resize_linear_u8", lambda img, nw, nh: _resize_without_area(img, nw, nh, trunc_area=True))
    names = [c[0] for c in S.REC_SMALL]
    _, gray = S.rec_small()
    _, bad = S.rec_expected(S.small_pages(), S.REC_SMALL)
    for i, n in enumerate(names):
        assert _differs(gray[i], bad[i]) == n.startswith("area2"), n
    _, bad = S.rec_expected(S.wide_pages(), S.REC_WIDE)
    assert _differs(S.rec_wide()[1][0], bad[0]) and not _differs(S.rec_wide()[1][1:], bad[1:])
    cn, crops, cv = S.cvit_case()
    for n in ("area2_1280x64_crop", "area2_1608x64_crop"):
        assert _differs(cv[cn.index(n)], S.gray_of(crops[cn.index(n)], S.CVIT_W)), n
    for crops, ref in (S.pp_crops_case(), S.pp_page_case()):
        bad = S.pp_expected(crops)
        assert any(_differs(r["image"], b["image"]) for r, b in zip(ref, bad))
    bad, _ = S.mtl_expected(S.small_pages(), S.MTL_BOXES)
    k = [b[0] for b in S.MTL_BOXES].index("area2_96x96")
    assert _differs(S.mtl_case()[0][k], bad[k]) and not _differs(np.delete(S.mtl_case()[0], k, 0), np.delete(bad, k, 0))
    S.det_case.cache_clear()
    try:
        bad = S.det_case("layout_area2_64")[1]
        bad2 = S.det_case("layout_w2x_only")[1]
    finally:
        S.det_case.cache_clear()
    monkeypatch.undo()
    assert _differs(good_det[0], bad) and not _differs(good_det[1], bad2)


def _warp_clamped(img, M, out_w, out_h, pad=40):
    """warp_perspective_u8 with the border replicated instead of zero (exact for taps up to `pad` pixels outside)"""
    big = np.pad(img, ((pad, pad), (pad, pad), (0, 0)), mode="edge")
    shift = np.array([[1, 0, -pad], [0, 1, -pad], [0, 0, 1]], np.float64)
    return _WARP(big, np.asarray(M, np.float64) @ shift, out_w, out_h)


_WARP = crnn.warp_perspective_u8


def test_wrong_variant_clamp_to_edge(monkeypatch):
    _warm()
    monkeypatch.setattr(crnn, "warp_perspective_u8", _warp_clamped)
    names = [c[0] for c in S.REC_SMALL]
    _, gray = S.rec_small()
    _, bad = S.rec_expected(S.small_pages(), S.REC_SMALL)
    for n in S.OVERHANG:
        assert _differs(gray[names.index(n)], bad[names.index(n)]), n
    for n in ("copy_40x32", "rotated", "keystone"):                 # lines inside the page do not notice
        assert not _differs(gray[names.index(n)], bad[names.index(n)]), n
    bad_cls = S.cls_line_inputs()
    monkeypatch.undo()
    good = S.cls_line_inputs()
    for i, c in enumerate(S.CLS_LINES):
        if c[0] in S.OVERHANG:
            assert _differs(good[i], bad_cls[i]), c[0]


def test_wrong_variant_page_index_ignored():
    names = [c[0] for c in S.REC_SMALL]
    _, gray = S.rec_small()
    _, bad = S.rec_expected(S.small_pages(), S.REC_SMALL, ignore_page=True)
    for i, c in enumerate(S.REC_SMALL):
        assert _differs(gray[i], bad[i]) == (c[1] == 1 and c[0] not in S.ALL_ZERO), c[0]
    good, bad_cls = S.cls_line_inputs(), S.cls_line_inputs(ignore_page=True)
    for i, c in enumerate(S.CLS_LINES):
        assert _differs(good[i], bad_cls[i]) == (c[1] == 1), c[0]
    assert any(_differs(r["image"], b["image"]) for r, b in zip(S.pp_page_case()[1], S.pp_page_case(True)[1]))
    for bgr in (True, False):
        bad = S.lore_expected(S.small_pages(), S.LORE_BOXES, bgr, ignore_page=True)
        for i, b in enumerate(S.LORE_BOXES):
            assert _differs(S.lore_case(bgr)[i], bad[i]) == (b[1] == 1), b[0]
    bad, _ = S.mtl_expected(S.small_pages(), S.MTL_BOXES, ignore_page=True)
    for i, b in enumerate(S.MTL_BOXES):
        assert _differs(S.mtl_case()[0][i], bad[i]) == (b[1] == 1), b[0]
    bad, _ = S.mtl_expected(S.flat_pages(), S.MTL_FLAT, ignore_page=True)
    assert _differs(S.mtl_flat_case()[0][0], bad[0]) and _differs(S.mtl_flat_case()[0][1], bad[1])
    for c in S.DET_CASES:
        if c[2][0] * c[2][1] > 64 * 64:
            continue
        good, bad = S.det_case(c[0])[1], S.det_case(c[0], True)[1]
        assert not _differs(good[0], bad[0]) and _differs(good[1], bad[1]), c[0]


def test_wrong_variant_crop_bound_ignored():
    names = [b[0] for b in S.LORE_BOXES]
    for bgr in (True, False):
        good = S.lore_case(bgr)
        bad = S.lore_expected(S.small_pages(), S.LORE_BOXES, bgr, ignore_crop=True)
        for n in ("px_1x1", "thin_3x90", "flat_90x3", "top_row_p1"):
            assert _differs(good[names.index(n)], bad[names.index(n)]), n
        assert not _differs(good[names.index("whole_page")], bad[names.index("whole_page")])      # the crop is the page


def test_wrong_variant_rows_read_across_the_page_seam():
    """the two pages as one tall image: a tap above row 0 of page 1 reads the last rows of page 0"""
    tall = np.concatenate(list(S.small_pages()), 0)
    names = [c[0] for c in S.REC_SMALL]
    _, gray = S.rec_small()
    for n in ("over_top_p1_seam", "over_top_p1_seam_rot", "over_bottom_p0"):
        c = S.REC_SMALL[names.index(n)]
        M, ow, oh = S.line_geometry(c)
        shift = np.array([[1, 0, 0], [0, 1, -S.PAGE_H * c[1]], [0, 0, 1]], np.float64)
        bad = S.gray_of(crnn.warp_perspective_u8(tall, M @ shift, ow, oh), S.REC_W)
        assert _differs(gray[names.index(n)], bad), n
    k = [b[0] for b in S.LORE_BOXES].index("top_row_p1")
    n, p, (x1, y1, x2, y2) = S.LORE_BOXES[k]
    # crop bound AND page bound ignored: against the page-bounded variant, so that the difference is the seam alone
    in_page = S.lore_expected(S.small_pages(), [S.LORE_BOXES[k]], True, ignore_crop=True)
    across = S.lore_expected(tall[None], [(n, 0, (x1, y1 + S.PAGE_H * p, x2, y2 + S.PAGE_H * p))], True, ignore_crop=True)
    assert _differs(in_page, across)


def test_wrong_variant_scan_carry_dropped():
    """off[i] = carry + the chunk's inclusive scan: without the carry, line i >= 1024 starts at the sum of lines 1024 .. i - 1 only"""
    cases, crops, gray = S.many_expected()
    px = np.array([c.shape[0] * c.shape[1] for c in crops], np.int64)
    true = np.concatenate([[0], np.cumsum(px)[:-1]])
    again = S.regather(crops, true)
    assert all(np.array_equal(a, b) for a, b in zip(again, crops))
    wrong = true.copy()
    wrong[1024:] -= true[1024]
    bad = S.regather(crops, wrong)
    for i in range(1024, S.MANY):
        assert _differs(gray[i], S.gray_of(bad[i], S.REC_W)[:, :S.MANY_KEEP_W]), i


def test_pplcnet_rescale_is_the_float64_product():
    """the classifier's input value of a byte: float32(v * (1 / 255) in float64), then float32 normalisation -- what
    transformers.image_transforms.rescale computes and what the engine's table holds"""
    from oracle import pil_resize
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    got = pil_resize.pplcnet_preprocess(img, 16, 16)
    r = (np.arange(256, dtype=np.float64) * (1 / 255)).astype(np.float32)
    for c in range(3):
        want = (r - np.float32(pil_resize.IMAGENET_MEAN[c])) / np.float32(pil_resize.IMAGENET_STD[c])
        assert np.array_equal(got[c].reshape(-1), want)
