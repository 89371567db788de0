"""predict_stream(..., orientation_vote=True): the text-line orientation vote as a stage of the software pipeline yields, batch by batch, what
predict() returns for each batch -- boxes, texts, layout, tables and HTML of the pages rotated by the vote, and the vote's own fields -- with the
fitted synthetic orientation head (pplcnet_state_dict(textline_head=True)) on batches that mix upright generator pages, their 180-degree copies and a
blank page (no lines: it votes "not upright" and is rotated, as in the reference)."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.synth_pages import make_page

pytestmark = pytest.mark.gpu


def _batches():
    made = [make_page(i) for i in range(4)]
    up = [m[0] for m in made]
    fl = [np.ascontiguousarray(m[0][::-1, ::-1]) for m in made]
    size = up[0].shape[0]
    tb_up = [np.asarray(m[1]["tables"]).reshape(-1, 4) for m in made]
    tb_fl = [np.stack([size - t[:, 2], size - t[:, 3], size - t[:, 0], size - t[:, 1]], 1) for t in tb_up]
    blank = np.full_like(up[0], 255)
    pages = [[up[0], fl[1]], [fl[0], up[2]], [blank, fl[2]], [up[1], fl[3]]]
    tbs = [[tb_up[0], tb_fl[1]], [tb_fl[0], tb_up[2]], [np.zeros((0, 4), np.int64), tb_fl[2]], [tb_up[1], tb_fl[3]]]
    return pages, tbs


def _pipeline(**kw):
    from pdf_table_amd.det_stage import DetConfig
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_weights import db_resnet18_state_dict, pplcnet_state_dict
    from pdf_table_amd.weights import pack_db_resnet18, pack_pplcnet
    p = OcrTablePipeline(device=0, synthetic_seed=0, layout=True, table_structure=True, table_html=True, text_orientation=True, **kw)
    # the detector with the hand-built text channel: its boxes are the generator's lines (the plain seeded one finds one page-sized box)
    # with bench.py's PP-OCR pre / post-process flavour (the one it was built for)
    p.engine.load_weights(L.PT_MODEL_DB_RESNET18, pack_db_resnet18(db_resnet18_state_dict(seed=0, text_signal=True), fmt=p.engine.weight_fmt))
    p.text_detector._stage.cfg = DetConfig(flavour="db_pp", thresh=0.3, box_thresh=0.6, unclip_ratio=1.5).resolved()
    p.engine.load_weights(L.PT_MODEL_PPLCNET + 0, pack_pplcnet(pplcnet_state_dict(seed=5, class_num=2, textline_head=True),
                                                               fmt=p.engine.weight_fmt))
    return p


def _same(rb, gb):
    assert len(rb) == len(gb)
    for a, b in zip(rb, gb):
        assert a.rotated_180 == b.rotated_180 and a.text_upright == b.text_upright
        # the vote is over the FIRST detection's lines; a rotated page's boxes are those of the second one (as in predict())
        assert len(a.text_line_orientation) == len(b.text_line_orientation)
        assert a.rotated_180 or len(a.text_line_orientation) == len(a.det_result)
        assert [o["class_ids"] for o in a.text_line_orientation] == [o["class_ids"] for o in b.text_line_orientation]
        assert [o["scores"] for o in a.text_line_orientation] == [o["scores"] for o in b.text_line_orientation]
        assert np.array_equal(a.det_result, b.det_result)
        assert [o["text"] for o in a.ocr_result] == [o["text"] for o in b.ocr_result]
        assert all(np.array_equal(x["bbox"], y["bbox"]) for x, y in zip(a.ocr_result, b.ocr_result))
        assert len(a.layout_result) == len(b.layout_result)
        for la, lb in zip(a.layout_result, b.layout_result):
            assert la["label"] == lb["label"] and np.array_equal(la["bbox"], lb["bbox"]) and la["score"] == lb["score"]
        assert len(a.table_structure_result) == len(b.table_structure_result)
        for ta, tb_ in zip(a.table_structure_result, b.table_structure_result):
            if ta is None or tb_ is None:
                assert ta is None and tb_ is None
                continue
            assert np.array_equal(ta["polygons"], tb_["polygons"]) and np.array_equal(ta["logi"], tb_["logi"])
            assert ta.get("table_html") == tb_.get("table_html")


def test_stream_orientation_equals_predict():
    pages, tbs = _batches()
    p = _pipeline()
    try:
        ref = {given: [p.predict(b, table_boxes=tbs[k] if given else None) for k, b in enumerate(pages)] for given in (True, False)}
        rot = [r.rotated_180 for b in ref[True] for r in b]
        assert any(rot) and not all(rot), rot
        assert min(len(r.det_result) for b in ref[True] for r in b if r is not ref[True][2][0]) > 20
        assert ref[True][2][0].rotated_180 and ref[True][2][0].text_line_orientation == []      # the blank page: no lines, "not upright"
        assert sum(len(r.table_structure_result) for b in ref[True] for r in b) >= 1

        def stream(given, **attrs):
            old = {k: getattr(p, k) for k in attrs}
            for k, v in attrs.items():
                setattr(p, k, v)
            try:
                return list(p.predict_stream(pages, table_boxes=tbs if given else None, orientation_vote=True))
            finally:
                for k, v in old.items():
                    setattr(p, k, v)

        for given in (True, False):
            got = stream(given)
            assert len(got) == 4
            for rb, gb in zip(ref[given], got):
                _same(rb, gb)
            assert p.metric["host_seconds"]["orient"] > 0 and "collect.orientation" in p.metric["host_seconds"]
        for attrs in ({"aux_layout": True}, {"overlap_rec": False}, {"lookahead": 2}):
            got = stream(True, **attrs)
            for rb, gb in zip(ref[True], got):
                _same(rb, gb)
        # a single batch already on the device (the pipeline drains after one step); the caller's tensor is not rotated in place
        t = torch.from_numpy(np.stack(pages[1])).cuda()
        keep = t.clone()
        one = list(p.predict_stream([t], table_boxes=[tbs[1]], orientation_vote=True))
        assert len(one) == 1 and torch.equal(t, keep)
        _same(ref[True][1], one[0])
        # rotate_upside_down=False: the vote is reported, nothing is rotated
        p.rotate_upside_down = False
        ref_keep = [p.predict(b, table_boxes=tbs[k]) for k, b in enumerate(pages)]
        got = stream(True)
        assert not any(r.rotated_180 for b in got for r in b)
        for rb, gb in zip(ref_keep, got):
            _same(rb, gb)
        p.rotate_upside_down = True
        # still refused without the opt-in
        with pytest.raises(ValueError, match="orientation_vote"):
            next(p.predict_stream(pages))
    finally:
        p.engine.close()
