"""The pixel pre-processors (pt_det_preprocess, pt_layout_preprocess, pt_rec_preprocess, pt_rec_cvit_preprocess_crops, pt_rec_pp_preprocess*,
pt_cls_preprocess, pt_cls_forward_lines*, pt_tsr_preprocess, pt_tsr_mtl_preprocess) at the inputs where resampling kernels go wrong: the
copy and exact-2x branches of every cv2.resize restatement and one size off each, 1-pixel crops, quads that hang over a page edge or over
the seam between two pages, crops in the last rows of the last page, more than 1024 lines in one offset scan, zero-size records.
Inputs and expected tensors: tests/preprocess_edge_synth.py (tests/test_preprocess_edges_host.py asserts on the CPU that every case
exercises its edge and that a subtly wrong kernel would change the expected values).

Pass criteria, those of the existing pre-process tests: bf16 / f16 outputs equal the oracle's fp32 tensor rounded to the format, bit for
bit; bf16x3 hi and lo bit-equal to the oracle's split for the recogniser, the detector and the layout input, |hi + lo - oracle| <= 2e-5
for the Lore, MtlTabNet and classifier inputs; fp32 outputs equal; padding channels zero.  Every element of every output is compared,
in PT_PRECISION_BF16, PT_PRECISION_F16 and PT_PRECISION_BF16X3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_edge_synth as S  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "bf16x3": L.PT_PRECISION_BF16X3}
TOL_PAIR = 2e-5           # hi + lo carries 16 mantissa bits of the fp32 value (test_gpu_tsr.py, test_gpu_mtl.py, test_gpu_cls.py)


@pytest.fixture(scope="module", params=list(PRECISIONS))
def eng(request):
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    e = HipEngine(0)
    e.set_precision(PRECISIONS[request.param])
    e.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True), fmt=e.weight_fmt))
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check16(eng, out, want, tag, pair_exact):
    """out: the engine's 16-bit tensor [..., C] ([..., hi C | lo C] in the pair mode); want: fp32 [..., c] with c <= C -- the first c
    channels hold values, the others are zero"""
    got = out.cpu()
    want = torch.as_tensor(want)
    c, dt = want.shape[-1], eng.act_dtype
    assert got.dtype == dt and got.shape[:-1] == want.shape[:-1], (tag, got.shape, want.shape)
    if not eng.split:
        assert torch.equal(_bits(got[..., :c]), _bits(want.to(dt))), (tag, float((got[..., :c].float() - want).abs().max()))
        assert not _bits(got[..., c:]).any(), tag
        return
    ch = got.shape[-1] // 2
    hi, lo = got[..., :ch], got[..., ch:]
    assert not _bits(hi[..., c:]).any() and not _bits(lo[..., c:]).any(), tag
    if pair_exact:
        wh = want.to(dt)
        assert torch.equal(_bits(hi[..., :c]), _bits(wh)), (tag, "hi")
        assert torch.equal(_bits(lo[..., :c]), _bits((want - wh.float()).to(dt))), (tag, "lo")
    else:
        d = float((hi[..., :c].float() + lo[..., :c].float() - want).abs().max())
        print(f"{tag}: max|hi + lo - oracle| = {d:.3e}")
        assert d <= TOL_PAIR, (tag, d)


def _gray16(eng, gray, want, tag):
    _check16(eng, gray if eng.split else gray.unsqueeze(-1), want.unsqueeze(-1), tag, True)


# ---- text-line warp + recogniser resize ----------------------------------------------------------------------------------------------
def test_rec_lines_branches_overhangs_and_empty_records(eng):
    """copy, exact 2x and one off each; 1-pixel crops; rotated and keystone quads; quads over each page edge on both pages (the top of page 1 is
    the seam); a quad outside the page, a crop whose resized width is 0 and a zero-size record are all-zero lines and their neighbours are right"""
    _, want = S.rec_small()
    gray = eng.rec_preprocess(torch.from_numpy(S.small_pages()).cuda(), S.line_records(S.REC_SMALL))
    torch.cuda.synchronize()
    eng.check()
    _gray16(eng, gray, want, "rec small")
    names = [c[0] for c in S.REC_SMALL]
    for n in S.ALL_ZERO:
        assert not _bits(gray[names.index(n)].cpu()).any(), n


def test_rec_lines_full_width_2x_and_ratio_cut_off(eng):
    """1280 x 64 -> 640 x 32 (exact 2x over the whole line), 641 x 32 (ratio just over 640 / 32), 640 x 32 (copy), on 1288-wide pages"""
    _, want = S.rec_wide()
    gray = eng.rec_preprocess(torch.from_numpy(S.wide_pages()).cuda(), S.line_records(S.REC_WIDE))
    torch.cuda.synchronize()
    _gray16(eng, gray, want, "rec wide")


def test_rec_1100_lines_in_one_offset_scan(eng):
    """rec_preprocess() -> pt_rec_preprocess hands all its lines to one rec_pre_chunk (only pt_rec_forward* micro-batch), so ONE
    pt_launch_rec_offsets call scans all 1100 records: two chunks of 1024 with the running carry.  Every line against the oracle"""
    cases, _, want = S.many_expected()
    gray = eng.rec_preprocess(torch.from_numpy(S.small_pages()).cuda(), S.line_records(cases))
    torch.cuda.synchronize()
    eng.check()
    g = gray.cpu()
    _gray16(eng, g[:, :, :S.MANY_KEEP_W], want, "rec 1100")
    assert not _bits(g[:, :, S.MANY_KEEP_W:]).any()


def test_cvit_crops_fp32(eng):
    """the same crops, and 1280 x 64, 1608 x 64 (2x on the 804 path), 805 x 32 (cut-off 804 / 32), 1 x 64 (resized width 0), through the crops
    entry: fp32 [n, 32, 804] equal to the oracle"""
    names, crops, want = S.cvit_case()
    got = eng.rec_cvit_preprocess_crops(crops).cpu()
    for i, n in enumerate(names):
        assert torch.equal(got[i], want[i]), (n, float((got[i] - want[i]).abs().max()))
    for n in ("nw0_1x64_crop", "zero_size", "outside"):
        assert not got[names.index(n)].any(), n


# ---- PP-OCR recogniser pre-processor ---------------------------------------------------------------------------------------------------
def _rec_pp(eng, crops, pages=None, lines=None):
    """pt_rec_pp_preprocess[_crops] as HipEngine.rec_pp_preprocess calls it, into a buffer of our own: the plan leaves GUARD floats before,
    between and after the mini-batches, pre-set to a sentinel"""
    from pdf_table_amd.engine import REC_LINE_DTYPE, _ptr, _upload
    items, batches, total = S.pp_plan(crops)
    out = torch.full((total,), S.SENTINEL, dtype=torch.float32, device="cuda")
    if lines is None:
        lines = np.zeros(len(crops), dtype=REC_LINE_DTYPE)
        lines["crop_w"], lines["crop_h"] = [c.shape[1] for c in crops], [c.shape[0] for c in crops]
    d, px = eng._lines_to_device(lines)
    di = _upload(np.ascontiguousarray(items).view(np.uint8).reshape(-1), eng._tdev)
    max_w = int(items["img_w"].max())
    if pages is None:
        dc = torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])).cuda()
        L.check(eng.lib.pt_rec_pp_preprocess_crops(eng._h, _ptr(dc), _ptr(d), px.ctypes.data_as(C.c_void_p), len(lines), _ptr(di), len(items),
                                                   S.PP_H, max_w, _ptr(out), eng._stream()), "pt_rec_pp_preprocess_crops")
    else:
        n, h, w, _ = pages.shape
        L.check(eng.lib.pt_rec_pp_preprocess(eng._h, _ptr(pages), n, h, w, _ptr(d), px.ctypes.data_as(C.c_void_p), len(lines), _ptr(di),
                                             len(items), S.PP_H, max_w, _ptr(out), eng._stream()), "pt_rec_pp_preprocess")
    torch.cuda.synchronize()
    return items, batches, out.cpu().numpy()


def _rec_pp_equal(items, batches, flat, ref, tag):
    used = np.zeros(flat.shape, bool)
    assert len(batches) == len(ref)
    for (beg, n, img_w, off), r in zip(batches, ref):
        assert np.array_equal(r["indices"], items["line"]) and r["batch_beg_img_no"] == beg
        size = n * 3 * S.PP_H * img_w
        got = flat[off:off + size].reshape(n, 3, S.PP_H, img_w)
        used[off:off + size] = True
        assert np.array_equal(got, r["image"]), (tag, beg, float(np.abs(got - r["image"]).max()))
        for k in range(n):
            assert not got[k, :, :, int(items["resized_w"][beg + k]):].any(), (tag, beg, k)          # zeros right of resized_w
    assert (~used).sum() == S.GUARD * (len(batches) + 1)
    assert (flat[~used] == S.SENTINEL).all(), f"{tag}: written outside a mini-batch's block"


def test_rec_pp_crops_branches_and_guards(eng):
    """crops of resized_w x 48 (copy), 2 resized_w x 96 (2x), one off each, 1 x 1; mini-batches of three items of different resized widths
    under one padded width; nothing written outside the blocks"""
    crops, ref = S.pp_crops_case()
    items, batches, flat = _rec_pp(eng, crops)
    _rec_pp_equal(items, batches, flat, ref, "rec_pp crops")


def test_rec_pp_page_lines_overhangs_and_guards(eng):
    """the page form: lines cut from two pages, over the right edge of page 0, the bottom of page 1 and the seam"""
    crops, ref = S.pp_page_case()
    items, batches, flat = _rec_pp(eng, crops, torch.from_numpy(S.small_pages()).cuda(), S.line_records(S.PP_PAGE))
    _rec_pp_equal(items, batches, flat, ref, "rec_pp page")


# ---- classifiers ---------------------------------------------------------------------------------------------------------------------------
def _net_input(eng, x):
    """fp32 [n, 3, H, W] -> the engine's NHWC4 input ((hi | lo) in the pair mode)"""
    t = torch.from_numpy(x).permute(0, 2, 3, 1)
    v = torch.zeros(t.shape[:3] + (4,))
    v[..., :3] = t
    hi = v.to(eng.act_dtype)
    if eng.split:
        hi = torch.cat([hi, (v - hi.float()).to(eng.act_dtype)], -1)
    return hi.contiguous().cuda()


def test_cls_lines_equal_the_net_on_the_oracle_input(eng):
    """overhanging, seam, outside and 1-pixel lines through pt_cls_forward_lines and pt_cls_forward_lines_direct: the logits of
    pt_cls_forward_net fed crop_image + the PP-LCNet processor from the oracle, bit for bit (18 lines: one micro-batch in all three calls)"""
    pages = torch.from_numpy(S.small_pages()).cuda()
    lines = S.line_records(S.CLS_LINES)
    assert len(lines) < 1024 and (lines["crop_w"] > 0).all() and (lines["crop_h"] > 0).all()
    ref = eng.cls_forward_net(_net_input(eng, S.cls_line_inputs()), 0, True)
    via_crops = eng.cls_forward_lines(pages, lines, S.CLS_HW, 0, True)
    direct = eng.cls_forward_lines_direct(pages, lines, S.CLS_HW, 0, True)
    torch.cuda.synchronize()
    eng.check()
    assert ref.shape == (len(lines), 2) and torch.isfinite(ref).all()
    assert len({tuple(r) for r in ref.cpu().numpy().tolist()}) > len(lines) // 2          # the lines do give different logits
    bad = [c[0] for c, a, b in zip(S.CLS_LINES, via_crops.cpu(), ref.cpu()) if not torch.equal(a, b)]
    assert not bad, ("pt_cls_forward_lines", bad)
    bad = [c[0] for c, a, b in zip(S.CLS_LINES, direct.cpu(), ref.cpu()) if not torch.equal(a, b)]
    assert not bad, ("pt_cls_forward_lines_direct", bad)


def test_cls_preprocess_one_pixel_images_in_a_ragged_batch(eng):
    """1 x 1, 1 x 300 and 300 x 1 images beside an ordinary one"""
    imgs, want = S.cls_images()
    out = eng.cls_preprocess(imgs, S.CLS_HW)
    torch.cuda.synchronize()
    _check16(eng, out, want.transpose(0, 2, 3, 1), "cls images", False)


def test_cls_preprocess_refuses_tables_over_64kb(eng):
    (h, w), out_hw = S.CLS_TOO_WIDE
    img = np.zeros((h, w, 3), np.uint8)
    with pytest.raises(L.PtError) as ei:
        eng.cls_preprocess([img], out_hw)
    msg = str(ei.value)
    assert "(status 1)" in msg and f"cls resize: {h}x{w} -> {out_hw[0]}x{out_hw[1]} needs" in msg and "coefficient tables (limit 64 KB)" in msg
    imgs, want = S.cls_images()                  # the engine still works
    out = eng.cls_preprocess(imgs, S.CLS_HW)
    torch.cuda.synchronize()
    eng.check()
    _check16(eng, out, want.transpose(0, 2, 3, 1), "cls images after the refusal", False)


# ---- detector and layout -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in S.DET_CASES])
def test_det_and_layout_preprocess(eng, name):
    """pages 1, 2, 3 and 5 pixels wide (the byte tail of a row for every pixel), w == 2 nw with h != 2 nh, the exact 2x at 64 x 64 and at
    1600 x 1216, a 37 x 23 page up to 608 x 800; page 1 as well as page 0"""
    case = S.DET_CASES[[c[0] for c in S.DET_CASES].index(name)]
    pages, want = S.det_case(name)
    dev = torch.from_numpy(pages).cuda()
    if case[1] == "layout":
        out = eng.layout_preprocess(dev, *case[3])
    else:
        fl = {"db_pp": L.PT_DET_PRE_DB_PP, "db_torch": L.PT_DET_PRE_DB_TORCH, "none": L.PT_DET_PRE_NONE}[case[1]]
        assert eng.det_plan(*case[2], fl) == tuple(S.det_plan(case))
        out = eng.det_preprocess(dev, fl)
    torch.cuda.synchronize()
    _check16(eng, out, want, name, True)


# ---- table crops -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [True, False])
def test_lore_preprocess_crop_and_page_bounds(eng, bgr):
    """the whole page, the bottom-right corner of the last page, 1 x 1 crops, 3 x 90 and 90 x 3 (the letterbox is the normalised zero pixel,
    not the page next to the crop), a crop whose top row is row 0 of page 1"""
    want = S.lore_case(bgr)
    out = eng.tsr_preprocess(torch.from_numpy(S.small_pages()).cuda(), S.table_records(S.LORE_BOXES, True), *S.LORE_HW, bgr=bgr)
    torch.cuda.synchronize()
    _check16(eng, out, want, f"lore bgr={bgr}", False)


def _mtl(eng, pages, boxes, want, sizes, tag):
    out = eng.mtl_preprocess(torch.from_numpy(pages).cuda(), S.table_records(boxes, False), S.MTL_SIZE)
    torch.cuda.synchronize()
    assert out.shape == (len(boxes), S.MTL_SIZE, S.MTL_SIZE, 64 if eng.split else 32)
    _check16(eng, out, want, tag, False)                   # channels 3 .. 31 zero (hi and lo)
    v = out.cpu().float()
    v = v[..., :3] + (v[..., 32:35] if eng.split else 0)
    for (n, _, (x1, y1, x2, y2)), (nw, nh), im in zip(boxes, sizes, v):
        assert eng.mtl_resized_size(x2 - x1, y2 - y1, S.MTL_SIZE) == (nw, nh), n
        assert (im[nh:] == -1.0).all() and (im[:, nw:] == -1.0).all(), n          # the pad value outside the resized image


def test_mtl_preprocess_branches_and_last_rows(eng):
    """48 x 48 (copy), 96 x 96 (2x), one off each, 1 x 1, a crop ending at the last row and column of the last page, crops on page 1"""
    want, sizes = S.mtl_case()
    _mtl(eng, S.small_pages(), S.MTL_BOXES, want, sizes, "mtl")


def test_mtl_preprocess_resized_height_one(eng):
    """1000 x 3 crops on 1000-wide pages: int(48 / 1000 * 3) = 0, one resized row; the second crop ends at the last row of the last page"""
    want, sizes = S.mtl_flat_case()
    assert sizes == [(48, 1), (48, 1)]
    _mtl(eng, S.flat_pages(), S.MTL_FLAT, want, sizes, "mtl flat")
