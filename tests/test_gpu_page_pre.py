"""Image-page straightening on the GPU (csrc/page_pre.hip, PagePreStage, OcrTablePipeline(deskew=..., sideways_check=...)) against the numpy
restatement tests/page_pre_ref.py, bit for bit, and end to end against predict() on the upright pages."""
import numpy as np
import pytest
import torch

import page_pre_ref as R
from pdf_table_amd import lib as L
from pdf_table_amd.synth_pages import make_page

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _dev(pages):
    return torch.from_numpy(np.ascontiguousarray(np.stack(pages))).cuda()


def _noisy(seed, h, w):
    rng = np.random.default_rng(seed)
    pg = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    pg[h // 3:h // 3 + 3, 20:w - 20] = 0         # a dark rule through the noise
    return pg


def _masks_equal(eng, pages):
    got = eng.page_line_mask(_dev(pages)).cpu().numpy().view(np.uint64)
    for k, pg in enumerate(pages):
        ref = R.pack_bits(R.line_mask(pg))
        assert np.array_equal(got[k], ref), f"page {k}: {int((got[k] != ref).sum())} words differ"


def test_mask_generator_pages(eng):
    _masks_equal(eng, [make_page(i)[0] for i in range(2)])


def test_mask_shapes(eng):
    full = make_page(2)[0]
    big = np.concatenate([full, full[:, ::-1]], 1)[:, :1240]        # 1024 x 1240
    big = np.concatenate([big, big[:216]], 0)                          # 1240 x 1240
    _masks_equal(eng, [_noisy(1, 300, 517)])
    _masks_equal(eng, [np.ascontiguousarray(big[:877])])               # 877 x 1240
    _masks_equal(eng, [np.ascontiguousarray(big[:, :877])])            # 1240 x 877
    strip = np.ascontiguousarray(full[500:509, 100:800])               # 9 x 700: shorter than the blur block
    strip[4] = 0
    _masks_equal(eng, [strip])
    _masks_equal(eng, [make_page(i)[0] for i in range(3, 7)] + [_noisy(2, 1024, 1024)])     # five pages, one launch
    # pages wider than 1920 px run the 8-row band (A4 at 300 dpi is 2480 px wide)
    wide = np.ascontiguousarray(np.concatenate([full, full[:, ::-1], full[:, :432]], 1)[:300])       # 300 x 2480
    assert wide.shape[1] == 2480
    _masks_equal(eng, [wide, np.ascontiguousarray(wide[::-1])])


def test_mask_rejects_bad_arguments(eng):
    lib = L.load()
    assert lib.pt_page_line_mask(None, 1, 10, 100, None, None) != 0
    p = torch.zeros((1, 10, 39, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(L.PtError):
        eng.page_line_mask(p)
    assert lib.pt_page_quarter_turn(None, 1, 4, 4, 3, None, None) != 0


@pytest.mark.parametrize("shape", [(512, 512), (300, 437)])
def test_warp_cubic(eng, shape):
    h, w = shape
    rng = np.random.default_rng(h)
    src = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    src[1] = np.ascontiguousarray(np.resize(make_page(0)[0], (h, w, 3)))
    angles = [0.2, -0.35, 1.7, -2.9, 7.5, -33.0]
    idx = [k % 2 for k in range(len(angles))]
    minv = np.stack([R.rotation_minv(h, w, a) for a in angles])
    got = eng.page_warp_cubic(_dev(list(src)), minv, idx).cpu().numpy()
    for j, a in enumerate(angles):
        ref = R.warp_cubic(src[idx[j]], minv[j])
        assert np.array_equal(got[j], ref), f"angle {a}: {int((got[j] != ref).any(-1).sum())} pixels differ"


def test_quarter_turns(eng):
    rng = np.random.default_rng(3)
    for h, w in [(37, 70), (100, 33), (64, 64)]:
        pages = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
        d = _dev(list(pages))
        for code, k in [(L.PT_ROTATE_90_CLOCKWISE, -1), (L.PT_ROTATE_180, 2), (L.PT_ROTATE_90_COUNTERCLOCKWISE, 1)]:
            got = eng.page_quarter_turn(d, code).cpu().numpy()
            assert np.array_equal(got, np.rot90(pages, k, axes=(1, 2))), (h, w, code)


def test_deskew_stage(eng):
    from pdf_table_amd.page_pre_stage import PagePreStage
    st = PagePreStage(eng)
    thetas = [-1.5, -0.6, 0.8, 1.5]
    pages = [R.warp_cubic(make_page(i)[0], R.rotation_minv(1024, 1024, t)) for i, t in enumerate(thetas)] + [make_page(4)[0]]
    d = _dev(pages)
    out, angles = st.deskew(d)
    out = out.cpu().numpy()
    for k, pg in enumerate(pages):
        ref, ang = R.deskew(pg)
        assert angles[k] == ang, (k, angles[k], ang)
        assert np.array_equal(out[k], ref), k
    for t, a in zip(thetas, angles):
        assert abs(t + a) <= 0.25, (t, a)
    assert angles[-1] == 0.0 and np.array_equal(out[-1], pages[-1])


def _pipeline():
    from pdf_table_amd.det_stage import DetConfig
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_weights import db_resnet18_state_dict, pplcnet_state_dict
    from pdf_table_amd.weights import pack_db_resnet18, pack_pplcnet
    p = OcrTablePipeline(device=0, synthetic_seed=0, layout=True, table_structure=True, table_html=True, text_orientation=True,
                         deskew=True, sideways_check=True)
    p.engine.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=p.engine.weight_fmt))
    p.text_detector._stage.cfg = DetConfig(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5).resolved()
    p.engine.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True),
                                                               fmt=p.engine.weight_fmt))
    return p


@pytest.fixture(scope="module")
def pipe():
    return _pipeline()


def _same(a, b):
    assert np.array_equal(a.det_result, b.det_result)
    assert [o["text"] for o in a.ocr_result] == [o["text"] for o in b.ocr_result]
    assert all(np.array_equal(x["bbox"], y["bbox"]) for x, y in zip(a.ocr_result, b.ocr_result))
    assert len(a.layout_result) == len(b.layout_result)
    for la, lb in zip(a.layout_result, b.layout_result):
        assert la["label"] == lb["label"] and np.array_equal(la["bbox"], lb["bbox"]) and la["score"] == lb["score"]
    assert len(a.table_structure_result) == len(b.table_structure_result)
    for ta, tb in zip(a.table_structure_result, b.table_structure_result):
        assert (ta is None) == (tb is None)
        if ta is not None:
            assert np.array_equal(ta["polygons"], tb["polygons"]) and np.array_equal(ta["logi"], tb["logi"])
            assert ta.get("table_html") == tb.get("table_html")


def _plain(p, pages):
    p.deskew = p.sideways_check = False
    try:
        return p.predict(pages)
    finally:
        p.deskew = p.sideways_check = True


def test_restoration_end_to_end(pipe):
    from pdf_table_amd.page_pre_stage import sideways_ratio
    up = [make_page(i)[0] for i in range(4)]
    crop = np.ascontiguousarray(up[0][:, :768])                      # 1024 x 768: the page changes shape when turned
    inputs = [up[0], np.ascontiguousarray(np.rot90(up[1], -1)), np.ascontiguousarray(np.rot90(up[2], 1)),
              np.ascontiguousarray(up[3][::-1, ::-1]), np.ascontiguousarray(np.rot90(crop, -1))]
    want = _plain(pipe, up + [crop])
    for k in (1, 2, 4):                                                 # precondition: the sideways copies detect tall boxes
        r = sideways_ratio(pipe._detect_boxes(torch.from_numpy(inputs[k][None]).cuda())[0])
        assert r is not None and r < 1, (k, r)
    got = pipe.predict(inputs)
    flags = [(False, False), (True, False), (True, True), (False, True), (True, False)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g.rotated_90, g.rotated_180) == flags[k], k
        assert g.image_shape == (up + [crop])[k].shape and g.skew_angle == 0.0
        assert w.rotated_180 is False and w.rotated_90 is False and w.skew_angle is None
        _same(g, w)


def test_page_orientation_switch():
    from pdf_table_amd.pipeline import OcrTablePipeline
    p = OcrTablePipeline(device=0, synthetic_seed=0, page_orientation=True, table_attribute=True)
    pages = [make_page(i)[0] for i in (5, 6)]
    got = p.predict(pages)
    for g in got:
        assert set(g.page_orientation) >= {"angle", "score"} and len(g.table_attribute["attributes"]) == 6
        assert g.image_shape in ((1024, 1024, 3),) and g.skew_angle is None and not g.rotated_90
    with pytest.raises(ValueError):
        next(iter(p.predict_stream([pages])))


def test_noop_and_refusals(pipe):
    pages = [make_page(i)[0] for i in (5, 6)]
    got = pipe.predict(pages)
    want = _plain(pipe, pages)
    for g, w in zip(got, want):
        assert not g.rotated_90 and not g.rotated_180 and g.skew_angle == 0.0
        _same(g, w)
    with pytest.raises(ValueError):
        pipe.predict(pages, table_boxes=[np.zeros((0, 4), np.int64)] * 2)
    with pytest.raises(ValueError):
        next(iter(pipe.predict_stream([pages])))


def _oracle_orient(sd_o, sd_a, page):
    """rotate_image_v2 driven by the fp32 oracle: (first result, second result or None, kept page, attribute result)"""
    from oracle import pil_resize, pplcnet
    from pdf_table_amd.page_pre_stage import orientation_keep, orientation_turn

    def cls(sd, img, task):
        x = torch.from_numpy(pil_resize.pplcnet_preprocess(img, 224, 224))[None]
        with torch.no_grad():
            lg = pplcnet.pplcnet_forward(sd, x).numpy()
        return (pplcnet.table_attribute_postprocess(lg) if task == "table_attribute" else pplcnet.topk_postprocess(lg, task))[0], lg[0]
    r1, _ = cls(sd_o, page, "text_image_orientation")
    attr, alog = cls(sd_a, page, "table_attribute")
    lab = orientation_turn(r1)
    if lab is None:
        return r1, None, page, attr, alog
    k = {"90": -1, "180": 2, "270": 1}[lab]
    t = np.ascontiguousarray(np.rot90(page, k))
    r2, _ = cls(sd_o, t, "text_image_orientation")
    return r1, r2, (t if orientation_keep(r2) else page), attr, alog


def test_orientation_parity(eng):
    from pdf_table_amd.cls_stage import ClsStage
    from pdf_table_amd.page_pre_stage import ORIENT_SCORE, PagePreStage
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    sd_o, sd_a = pplcnet_state_dict(seed=6, class_num=4), pplcnet_state_dict(seed=7, class_num=6)
    eng.load_weights(L.PT_MODEL_PPLCNET + 1, pack_pplcnet(sd_o))
    eng.load_weights(L.PT_MODEL_PPLCNET + 2, pack_pplcnet(sd_a))
    up = [make_page(i)[0] for i in range(3)]
    pages = up + [np.ascontiguousarray(np.rot90(up[0], -1)), np.ascontiguousarray(up[1][::-1, ::-1]),
                  np.ascontiguousarray(np.rot90(up[2], 1))]
    eng.set_precision(L.PT_PRECISION_BF16X3)
    try:
        groups, metrics, attrs = PagePreStage(eng).orient(_dev(pages), ClsStage(eng, "text_image_orientation", 1),
                                                          ClsStage(eng, "table_attribute", 2))
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    final = {}
    for idx, t in groups:
        for k, i in enumerate(idx):
            final[i] = t[k].cpu().numpy()
    assert sorted(final) == list(range(len(pages)))
    excluded = 0
    turned = 0
    for i, pg in enumerate(pages):
        r1, r2, kept, attr, alog = _oracle_orient(sd_o, sd_a, pg)
        if abs(r1["scores"][0] - ORIENT_SCORE) <= 1e-3:
            excluded += 1
            continue
        m = metrics[i]
        assert m["angle"] == r1["label_names"][0] and abs(m["score"] - r1["scores"][0]) <= 1e-3, (i, m, r1)
        assert ("angle2" in m) == (r2 is not None), (i, m)
        if r2 is not None:
            turned += 1
            assert m["angle2"] == r2["label_names"][0] and abs(m["score2"] - r2["scores"][0]) <= 1e-3, (i, m, r2)
        assert np.array_equal(final[i], kept), i
        near = np.abs(alog - 0.5) <= 1e-3                  # an output on the 0.5 threshold may fall either way
        assert [a for a, n in zip(attrs[i]["attributes"], near) if not n] == [a for a, n in zip(attr["attributes"], near) if not n], i
    print(f"orientation parity: {len(pages) - excluded} pages compared, {excluded} excluded (first score within 1e-3 of 0.6), "
          f"{turned} turned and classified again")
    assert excluded <= 1 and turned > 0


def test_preprocess_task(eng):
    from pdf_table_amd.ocr_table_preprocess_task import OcrTablePreprocessTask
    task = OcrTablePreprocessTask(engine=eng, synthetic_seed=6)
    pg = R.warp_cubic(make_page(3)[0], R.rotation_minv(1024, 1024, 0.8))
    img, metric = task(pg)
    assert set(metric) == {"use_time", "angle_metric", "angle2", "image_name"}
    am = metric["angle_metric"]
    assert {"angle", "score", "rotate_small"} <= set(am) and set(am) <= {"angle", "score", "angle2", "score2", "rotate_small"}
    ref, ang = R.deskew(pg)
    assert am["rotate_small"] == ang == metric["angle2"] and abs(ang + 0.8) <= 0.25
    if "angle2" not in am or am["angle2"] not in ("0", "180"):
        assert np.array_equal(img, ref)                      # not turned: the deskewed page
    assert task.table_attribute is not None and len(task.table_attribute["attributes"]) == 6
