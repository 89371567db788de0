"""Inputs and expected tensors for the edge cases of the pixel pre-processors (tests/test_preprocess_edges_host.py,
tests/test_gpu_preprocess_edges.py): the copy / exact-2x / general branches of every cv2.resize restatement, 1-pixel crops, quads that
hang over a page edge or over the seam between two pages, crops in the last rows of the last page, more lines than one chunk of the
offset scan.  CPU only, deterministic.

Pages are random uint8 (a wrong tap changes the value) and the pages of a batch are drawn independently (a read across the seam
shows).  Expected tensors come from the numpy oracles (oracle/crnn.py, db_pre.py, rec_pp.py, lore_pre.py, mtl_tabnet.py, pil_resize.py,
picodet.py); the host halves that turn boxes into records (rec_stage.build_lines, tsr_stage.lore_geometry, rec_pp_stage.rec_pp_plan) are the
package's own, as in the other GPU tests.  Builders take ``ignore_page`` / ``ignore_crop`` so that the host test can compute deliberately
wrong expectations; the other wrong variants replace an oracle function (monkeypatch) and call the same builders."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import crnn, db_pre, lore_pre, pil_resize, picodet, rec_pp
from oracle import mtl_tabnet as omt

PAGE_H, PAGE_W = 96, 128
REC_H, REC_W, CVIT_W = 32, 640, 804
CLS_HW = (80, 160)
LORE_HW = (64, 96)
MTL_SIZE = 48
PP_H = 48
PP_BATCH = 3              # rec_batch_num of the PP-OCR plan used here: mini-batches of three


def rand_pages(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def small_pages():
    return rand_pages(9001, 2, PAGE_H, PAGE_W)


@functools.lru_cache(maxsize=None)
def wide_pages():
    return rand_pages(9002, 2, 64, 1288)


# ---- which branch of a cv2.resize restatement a case takes --------------------------------------------------------------------------
def classify(cw, ch, nw, nh):
    """(source size, destination size) -> 'copy' | 'area2' | 'general' | 'empty' (nothing is resized)"""
    if cw <= 0 or ch <= 0 or nw <= 0 or nh <= 0:
        return "empty"
    if (cw, ch) == (nw, nh):
        return "copy"
    if cw == 2 * nw and ch == 2 * nh:
        return "area2"
    return "general"


def rec_nw(cw, ch, tw):
    """keepratio_resize's width (processor_ocr_recognition.py:44-62)"""
    if cw <= 0 or ch <= 0:
        return 0
    r = cw / float(ch)
    return tw if r > float(tw) / REC_H else int(REC_H * r)


def mtl_nwh(cw, ch, size=MTL_SIZE):
    fw, fh = float(cw), float(ch)
    if fw < fh:
        fw, fh = size / fh * fw, size
    else:
        fh, fw = size / fw * fh, size
    return max(int(fw), 1), max(int(fh), 1)


# ---- text lines -------------------------------------------------------------------------------------------------------------------------
def rect(x0, y0, w, h):
    return np.array([x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h], np.float64)


def quad(cx, cy, w, h, ang):
    c, s = np.cos(ang), np.sin(ang)
    pts = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
    return (pts @ np.array([[c, s], [-s, c]]) + [cx, cy]).reshape(8)


# (name, page, quad, forced (crop_w, crop_h) or None).  A forced size keeps the quad's matrix and changes the output size of the warp:
# a 1-pixel quad has a singular cv2.getPerspectiveTransform system, so 1-pixel crops are cut with a valid matrix (as
# test_gpu_cls_lines_direct.py does)
REC_SMALL = [
    ("copy_40x32", 0, rect(20, 30, 40, 32), None),
    ("area2_100x64", 1, rect(10, 10, 100, 64), None),
    ("area2_120x64", 0, rect(4, 20, 120, 64), None),
    ("w41_h32", 1, rect(50, 5, 41, 32), None),                 # nw = int(32 * 41 / 32) = 41: still the copy branch
    ("off_copy_40x33", 0, rect(60, 40, 40, 33), None),
    ("off_area2_100x63", 1, rect(14, 16, 100, 63), None),
    ("px_1x1", 0, rect(30, 30, 20, 10), (1, 1)),
    ("px_wx1", 1, rect(30, 50, 37, 10), (37, 1)),
    ("px_1xh", 0, rect(70, 20, 10, 20), (1, 20)),
    ("rotated", 1, quad(64, 48, 70, 20, 0.3), None),
    ("keystone", 0, np.array([20, 20, 100, 28, 96, 52, 22, 60], np.float64), None),
    ("over_left_p0", 0, rect(-5, 30, 50, 20), None),
    ("over_right_p0", 0, rect(90, 30, 45, 20), None),
    ("over_top_p0", 0, rect(30, -6, 50, 20), None),
    ("over_bottom_p0", 0, rect(30, 82, 50, 20), None),
    ("over_left_p1", 1, rect(-9, 40, 60, 24), None),
    ("over_right_p1", 1, rect(85, 10, 46, 18), None),
    ("over_top_p1_seam", 1, rect(20, -7, 64, 22), None),
    ("over_bottom_p1", 1, rect(10, 80, 70, 19), None),
    ("over_top_p1_seam_rot", 1, quad(64, 4, 80, 24, 0.15), None),
    ("outside", 0, rect(200, 150, 40, 16), None),
    ("before_nw0", 1, rect(8, 8, 30, 12), None),
    ("nw0_1x64", 0, rect(40, 10, 20, 64), (1, 64)),
    ("after_nw0", 1, rect(60, 60, 33, 17), None),
    ("zero_size", 0, rect(10, 10, 30, 20), (0, 20)),
    ("after_zero_size", 1, rect(5, 70, 90, 21), None),
]
OVERHANG = [c[0] for c in REC_SMALL if c[0].startswith("over_")]
ALL_ZERO = ["outside", "nw0_1x64", "zero_size"]

# on the 64 x 1288 pages: the exact 2x reduction to the full 640 columns, and the ratio cut-off 640 / 32
REC_WIDE = [
    ("area2_1280x64", 1, rect(3, 0, 1280, 64), None),
    ("cut_641x32", 0, rect(100, 20, 641, 32), None),
    ("wide_copy_640x32", 1, rect(300, 5, 640, 32), None),
]


def line_geometry(case):
    """-> (M 3x3 float64, crop_w, crop_h) of a case: order_point + the host part of crop_image, then the forced size"""
    src, dst, ow, oh = crnn.crop_geometry(crnn.order_point(case[2]))
    if case[3] is not None:
        ow, oh = case[3]
    return crnn.get_perspective_transform(src, dst), ow, oh


def line_records(cases):
    """pt_rec_line records in case order (page and forced sizes applied)"""
    from pdf_table_amd.rec_stage import build_lines
    lines = build_lines([np.stack([c[2] for c in cases])])
    for i, c in enumerate(cases):
        lines["page"][i] = c[1]
        if c[3] is not None:
            lines["crop_w"][i], lines["crop_h"][i] = c[3]
    return lines


def line_crop(pages, case, ignore_page=False):
    M, ow, oh = line_geometry(case)
    return crnn.warp_perspective_u8(pages[0 if ignore_page else case[1]], M, ow, oh)


def gray_of(crop, tw):
    """crop uint8 -> fp32 [32, tw]: keepratio_resize, / 255, gray; an empty crop is an all-zero line (the engine's contract where
    cv2.resize raises)"""
    if crop.shape[0] <= 0 or crop.shape[1] <= 0:
        return torch.zeros(REC_H, tw)
    x = crnn.rec_preprocess(crop, REC_H, tw)
    return (x[:, 0:1] * 0.2989 + x[:, 1:2] * 0.5870 + x[:, 2:3] * 0.1140)[0, 0]


def rec_expected(pages, cases, tw=REC_W, ignore_page=False, keep_w=None):
    """-> (crops, gray fp32 [n, 32, keep_w or tw])"""
    crops = [line_crop(pages, c, ignore_page) for c in cases]
    return crops, torch.stack([gray_of(c, tw)[:, :keep_w] for c in crops])


@functools.lru_cache(maxsize=None)
def rec_small():
    return rec_expected(small_pages(), REC_SMALL)


@functools.lru_cache(maxsize=None)
def rec_wide():
    return rec_expected(wide_pages(), REC_WIDE)


# ---- the ConvNextViT path: already-cropped lines, 804 columns ------------------------------------------------------------------------
CVIT_SIZES = [("area2_1280x64", 64, 1280), ("area2_1608x64", 64, 1608), ("cut_805x32", 32, 805), ("copy_641x32", 32, 641),
              ("copy_804x32", 32, 804), ("off_1608x63", 63, 1608), ("nw0_1x64", 64, 1), ("px_1x1", 1, 1), ("after", 20, 90)]


@functools.lru_cache(maxsize=None)
def cvit_case():
    """-> (names, crops, gray fp32 [n, 32, 804]): the page crops of REC_SMALL (the zero-size one included), then random crops"""
    rng = np.random.default_rng(9003)
    names = [c[0] for c in REC_SMALL] + [s[0] + "_crop" for s in CVIT_SIZES]
    crops = list(rec_small()[0]) + [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _, h, w in CVIT_SIZES]
    return names, crops, torch.stack([gray_of(c, CVIT_W) for c in crops])


# ---- more lines than one chunk of the offset scan ------------------------------------------------------------------------------------
MANY = 1100
MANY_KEEP_W = 160         # 32 * 9 / 2 = 144 columns at the most carry text: the rest of every line is zero


def many_cases(n=MANY):
    """n lines of 2..9 x 2..5 px, neighbours never of the same size, alternating between the two pages"""
    rng = np.random.default_rng(9004)
    cases, last = [], None
    while len(cases) < n:
        w, h = int(rng.integers(2, 10)), int(rng.integers(2, 6))
        if (w, h) == last or (last and w * h == last[0] * last[1]):
            continue
        last = (w, h)
        cases.append((f"many{len(cases)}", len(cases) % 2, rect(int(rng.integers(0, PAGE_W - w)), int(rng.integers(0, PAGE_H - h)), w, h), None))
    return cases


@functools.lru_cache(maxsize=None)
def many_expected():
    """-> (cases, crops, gray fp32 [1100, 32, 160])"""
    cases = many_cases()
    crops, gray = rec_expected(small_pages(), cases, keep_w=MANY_KEEP_W)
    return cases, crops, gray


def regather(crops, offsets):
    """the crops as a consumer reads them from the ragged buffer when line i is believed to start at pixel offsets[i]"""
    flat = np.concatenate([c.reshape(-1, 3) for c in crops] + [np.zeros((64, 3), np.uint8)])
    return [flat[o:o + c.shape[0] * c.shape[1]].reshape(c.shape) for c, o in zip(crops, offsets)]


# ---- PP-OCR recogniser pre-processor ---------------------------------------------------------------------------------------------------
PP_SIZES = [("copy_60x48", 48, 60), ("area2_120x96", 96, 120), ("off_copy_60x47", 47, 60), ("off_area2_121x96", 96, 121),
            ("px_1x1", 1, 1), ("copy_200x48", 48, 200), ("area2_400x96", 96, 400), ("copy_30x48", 48, 30)]
PP_PAGE = [("copy_60x48", 0, rect(30, 20, 60, 48), None), ("area2_120x96", 1, rect(4, 0, 120, 96), None),
           ("off_copy_61x49", 0, rect(10, 40, 61, 49), None), ("over_top_p1_seam", 1, rect(20, -7, 64, 22), None),
           ("over_right_p0", 0, rect(90, 30, 45, 20), None), ("px_1x1", 1, rect(30, 30, 20, 10), (1, 1)),
           ("over_bottom_p1", 1, rect(10, 80, 70, 19), None)]
GUARD = 64
SENTINEL = -12345.5


def pp_plan(crops):
    """rec_pp_plan with mini-batches of three, every mini-batch's block moved so that GUARD floats lie before the first, between two and
    after the last -> (items, [(beg, n, img_w, offset)], total floats)"""
    from pdf_table_amd.rec_pp_stage import PPOcrRecConfig, rec_pp_plan
    items, batches, total = rec_pp_plan([c.shape[1] for c in crops], [c.shape[0] for c in crops], PPOcrRecConfig(rec_batch_num=PP_BATCH))
    items = items.copy()
    moved = []
    for k, (beg, n, img_w, off) in enumerate(batches):
        items["out_off"][beg:beg + n] += GUARD * (k + 1)
        moved.append((beg, n, img_w, off + GUARD * (k + 1)))
    return items, moved, total + GUARD * (len(batches) + 1)


def pp_expected(crops):
    return rec_pp.rec_pp_preprocess(crops, rec_batch_num=PP_BATCH)


@functools.lru_cache(maxsize=None)
def pp_crops_case():
    rng = np.random.default_rng(9005)
    crops = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _, h, w in PP_SIZES]
    return crops, pp_expected(crops)


@functools.lru_cache(maxsize=None)
def pp_page_case(ignore_page=False):
    crops = [line_crop(small_pages(), c, ignore_page) for c in PP_PAGE]
    return crops, pp_expected(crops)


def pp_resized(crops):
    """per crop (resized_w, img_w) of the plan"""
    items, _, _ = pp_plan(crops)
    out = [None] * len(crops)
    for it in items:
        out[int(it["line"])] = (int(it["resized_w"]), int(it["img_w"]))
    return out


# ---- line classifier ---------------------------------------------------------------------------------------------------------------------
CLS_LINES = [c for c in REC_SMALL if c[0] in OVERHANG + ["px_1x1", "px_wx1", "px_1xh", "rotated", "outside", "nw0_1x64", "copy_40x32"]]


def cls_line_inputs(ignore_page=False):
    """fp32 [n, 3, 80, 160]: crop_image, then the PP-LCNet processor"""
    return np.stack([pil_resize.pplcnet_preprocess(line_crop(small_pages(), c, ignore_page), *CLS_HW) for c in CLS_LINES])


@functools.lru_cache(maxsize=None)
def cls_images():
    rng = np.random.default_rng(9006)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (1, 300), (300, 1), (60, 90))]
    return imgs, np.stack([pil_resize.pplcnet_preprocess(im, *CLS_HW) for im in imgs])


CLS_TOO_WIDE = ((1, 7841), (224, 224))       # 224 * (2 * ceil(7841 / 224) + 1 + 2) * 4 bytes = 67200 > 64 KB


# ---- detector and layout ---------------------------------------------------------------------------------------------------------------
# (name, flavour 'db_pp' | 'db_torch' | 'none' | 'layout', page (h, w), layout target (inp_h, inp_w) or None)
DET_CASES = [
    ("pp_w1", "db_pp", (40, 1), None), ("pp_w2", "db_pp", (40, 2), None), ("pp_w3", "db_pp", (40, 3), None), ("pp_w5", "db_pp", (40, 5), None),
    ("torch_w1", "db_torch", (1, 1), None), ("torch_w2", "db_torch", (3, 2), None), ("torch_w3", "db_torch", (2, 3), None),
    ("torch_w5", "db_torch", (4, 5), None),
    ("none_32x64", "none", (32, 64), None),
    ("layout_w2x_only", "layout", (40, 64), (32, 32)),
    ("layout_area2_64", "layout", (64, 64), (32, 32)),
    ("layout_w1", "layout", (5, 1), (32, 32)),
    ("layout_up_37x23", "layout", (23, 37), (800, 608)),
    ("layout_area2_1600x1216", "layout", (1600, 1216), (800, 608)),
]


def det_plan(case):
    _, fl, (h, w), tgt = case
    if fl == "db_pp":
        return db_pre.det_plan_db_pp(h, w)
    if fl == "db_torch":
        return db_pre.det_plan_db_torch(h, w)
    return (h, w) if fl == "none" else tgt


@functools.lru_cache(maxsize=None)
def det_case(name, ignore_page=False):
    """-> (pages uint8 [2, h, w, 3], expected fp32 [2, nh, nw, 3])"""
    k = [c[0] for c in DET_CASES].index(name)
    case = DET_CASES[k]
    _, fl, (h, w), tgt = case
    pages = rand_pages(9100 + k, 2, h, w)
    out = []
    for b in range(2):
        img = pages[0 if ignore_page else b]
        if fl == "db_torch":
            chw = db_pre.preprocess_db_torch(img)[0]
        elif fl == "layout":
            chw = picodet.picodet_preprocess(img, *tgt)[0]
        else:
            chw = db_pre.preprocess_db_pp(img)[0]
        out.append(np.ascontiguousarray(chw.transpose(1, 2, 0)))
    return pages, np.stack(out)


# ---- table crops -------------------------------------------------------------------------------------------------------------------------
# (name, page, (x1, y1, x2, y2)) on the 96 x 128 pages
LORE_BOXES = [
    ("whole_page", 0, (0, 0, PAGE_W, PAGE_H)),
    ("bottom_right_p1", 1, (90, 70, PAGE_W, PAGE_H)),
    ("px_1x1", 0, (50, 40, 51, 41)),
    ("px_1x1_last", 1, (PAGE_W - 1, PAGE_H - 1, PAGE_W, PAGE_H)),
    ("thin_3x90", 1, (60, 3, 63, 93)),
    ("flat_90x3", 0, (20, 50, 110, 53)),
    ("top_row_p1", 1, (10, 0, 70, 30)),
]


def table_records(boxes, with_minv):
    from pdf_table_amd.engine import TSR_TABLE_DTYPE
    from pdf_table_amd.tsr_stage import lore_geometry
    recs = np.zeros(len(boxes), dtype=TSR_TABLE_DTYPE)
    for i, (_, p, (x1, y1, x2, y2)) in enumerate(boxes):
        recs["page"][i], recs["x0"][i], recs["y0"][i], recs["crop_w"][i], recs["crop_h"][i] = p, x1, y1, x2 - x1, y2 - y1
        if with_minv:
            recs["minv"][i] = lore_geometry(y2 - y1, x2 - x1, *LORE_HW)[0].reshape(6)
    return recs


def lore_expected(pages, boxes, bgr, ignore_page=False, ignore_crop=False):
    """fp32 [n, 64, 96, 3].  ignore_crop: the warp samples the whole page through the crop's matrix moved to page coordinates, so a tap
    next to the crop reads page content instead of the zero border"""
    from oracle.lore_decode import lore_preprocess_geometry
    out = []
    for _, p, (x1, y1, x2, y2) in boxes:
        page = pages[0 if ignore_page else p]
        if ignore_crop:
            trans, _ = lore_preprocess_geometry(y2 - y1, x2 - x1, *LORE_HW)
            trans = np.asarray(trans, np.float64).copy()
            trans[:, 2] -= trans[:, 0] * x1 + trans[:, 1] * y1
            src = page[:, :, ::-1] if bgr else page
            warped = lore_pre.warp_affine_u8(np.ascontiguousarray(src), trans, LORE_HW[1], LORE_HW[0])
            x = ((warped / 255.0 - lore_pre.MEAN.reshape(1, 1, 3)) / lore_pre.STD.reshape(1, 1, 3)).astype(np.float32)
        else:
            crop = page[y1:y2, x1:x2]
            x = lore_pre.lore_preprocess(np.ascontiguousarray(crop[:, :, ::-1] if bgr else crop), *LORE_HW)[0][0].permute(1, 2, 0).numpy()
        out.append(x)
    return np.stack(out)


def lore_zero_pixel(bgr):
    """the normalised value of a border pixel (the warp's constant 0)"""
    return ((0.0 - lore_pre.MEAN) / lore_pre.STD).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lore_case(bgr):
    return lore_expected(small_pages(), LORE_BOXES, bgr)


MTL_BOXES = [
    ("copy_48x48", 0, (10, 10, 58, 58)),
    ("area2_96x96", 1, (16, 0, 112, 96)),
    ("off_copy_49x48", 0, (10, 10, 59, 58)),
    ("off_area2_96x95", 1, (16, 0, 112, 95)),
    ("px_1x1", 0, (5, 5, 6, 6)),
    ("last_row_col_p1", 1, (100, 80, PAGE_W, PAGE_H)),
    ("tall_p1", 1, (40, 6, 60, 90)),
]
MTL_FLAT = [("flat_1000x3", 1, (0, 2, 1000, 5)), ("flat_1000x3_last_rows", 1, (0, 5, 1000, 8))]


@functools.lru_cache(maxsize=None)
def flat_pages():
    return rand_pages(9007, 2, 8, 1000)


def mtl_expected(pages, boxes, ignore_page=False):
    """-> (fp32 [n, 48, 48, 3], [(resized w, resized h)] from the oracle's img_shape)"""
    out, sizes = [], []
    for _, p, (x1, y1, x2, y2) in boxes:
        x, meta = omt.mtl_preprocess(np.ascontiguousarray(pages[0 if ignore_page else p][y1:y2, x1:x2]), MTL_SIZE)
        out.append(x.permute(1, 2, 0).numpy())
        sizes.append((meta["img_shape"][1], meta["img_shape"][0]))
    return np.stack(out), sizes


@functools.lru_cache(maxsize=None)
def mtl_case():
    return mtl_expected(small_pages(), MTL_BOXES)


@functools.lru_cache(maxsize=None)
def mtl_flat_case():
    return mtl_expected(flat_pages(), MTL_FLAT)
