"""OcrTablePipeline(device_match=True): the Lore stage assigns every table's candidate lines to its cells on the device (TsrStage.process(match=...),
pt_op_lore_match) and _attach_html uses that map.  The HTML must be the one the same pipeline builds with the knob off (find_top1_match on the
host), in predict() and in predict_stream(), in bf16 and in the fp32 pair mode; the map itself must equal find_top1_match run on the result's own
polygons, axes and lines."""
import numpy as np
import pytest
import torch

from lore_match_ref import sorted_match_to_rows
from pdf_table_amd.synth_pages import make_page
from pdf_table_amd.table_text_match import text_boxes, texts_in_table

pytestmark = pytest.mark.gpu

PAGES = (3, 5)


def _pipe(**kw):
    from pdf_table_amd.pipeline import OcrTablePipeline
    return OcrTablePipeline(device=0, synthetic_seed=0, layout=True, table_structure=True, table_html=True, **kw)


def _check_map(table, page_boxes):
    """'matched' against find_top1_match over the table's own polygons / logi and the candidate lines' boxes"""
    lines = np.asarray(table["matched_lines"], np.int64)
    assert len(table["matched"]) == len(lines)
    if len(table["scores"]) == 0:
        assert len(lines) == 0
        return 0
    tbx = text_boxes(page_boxes) if len(page_boxes) else np.zeros((0, 4))
    want = sorted_match_to_rows(table["polygons"], table["logi"], tbx[lines])
    assert np.asarray(table["matched"]).tolist() == want.tolist()
    return len(lines)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_html_equals_the_host_route_in_predict_and_predict_stream(precision):
    pages = [make_page(i)[0] for i in PAGES]
    given = [np.asarray(make_page(i)[1]["tables"]).reshape(-1, 4) for i in PAGES]
    off = _pipe(precision=precision)
    ref = off.predict(pages)
    ref_given = off.predict(pages, table_boxes=given)
    ref_stream = list(off.predict_stream([pages[:1], pages[1:]]))
    off.engine.close()
    on = _pipe(precision=precision, device_match=True)
    got = on.predict(pages)
    got_given = on.predict(pages, table_boxes=given)
    got_stream = list(on.predict_stream([pages[:1], pages[1:]]))
    on.engine.close()
    n_tables = n_lines = 0
    for rs, gs in ((ref, got), (ref_given, got_given), ([r for b in ref_stream for r in b], [r for b in got_stream for r in b])):
        assert len(rs) == len(gs) == 2
        for a, b in zip(rs, gs):
            assert np.array_equal(a.det_result, b.det_result)
            assert len(a.table_structure_result) == len(b.table_structure_result)
            for ta, tb in zip(a.table_structure_result, b.table_structure_result):
                assert "matched" not in ta and "matched_lines" not in ta          # knob off: the dicts are what they were
                assert np.array_equal(ta["polygons"], tb["polygons"]) and np.array_equal(ta["logi"], tb["logi"])
                assert ta["table_html"] == tb["table_html"] and ta["db_table_html"] == tb["db_table_html"]
                n_lines += _check_map(tb, b.det_result)
                n_tables += 1
    assert n_tables >= 3 and n_lines >= 1


def test_html_equals_the_host_route_with_the_orientation_vote():
    """orientation_vote=True: the boxes the stage matches are those of the second detection pass (page 1 is handed in upside-down)"""
    pages = [make_page(3)[0], np.ascontiguousarray(make_page(5)[0][::-1, ::-1])]
    outs = []
    for knob in (False, True):
        p = _pipe(text_orientation=True, device_match=knob)
        outs.append([r for b in p.predict_stream([pages], orientation_vote=True) for r in b])
        outs.append(p.predict(pages))
        p.engine.close()
    for rs, gs in ((outs[0], outs[2]), (outs[1], outs[3])):
        for a, b in zip(rs, gs):
            assert a.rotated_180 == b.rotated_180 and np.array_equal(a.det_result, b.det_result)
            assert len(a.table_structure_result) == len(b.table_structure_result)
            for ta, tb in zip(a.table_structure_result, b.table_structure_result):
                assert "matched" not in ta
                assert ta["table_html"] == tb["table_html"] and ta["db_table_html"] == tb["db_table_html"]
                _check_map(tb, b.det_result)


def test_the_knob_needs_the_lore_model():
    from pdf_table_amd.pipeline import OcrTablePipeline
    with pytest.raises(ValueError, match="CenterNet"):
        OcrTablePipeline(device=0, synthetic_seed=0, table_structure=True, table_structure_model="CenterNet", device_match=True)
    from pdf_table_amd.centernet_stage import CenterNetStage
    with pytest.raises(ValueError, match="CenterNetStage"):
        OcrTablePipeline.from_engine(None, None, None, tsr_stage=CenterNetStage.__new__(CenterNetStage), device_match=True)


def _seeded_text_boxes(rng, regions, per_table):
    """integer line boxes inside and around every table region of a page -> [t, 4]"""
    out = []
    for (x1, y1, x2, y2) in np.asarray(regions).reshape(-1, 4).tolist():
        for _ in range(per_table):
            w, h = rng.uniform(20, 0.4 * (x2 - x1)), rng.uniform(8, 30)
            cx, cy = rng.uniform(x1 - 10, x2 + 10), rng.uniform(y1 - 10, y2 + 10)
            out.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    return np.trunc(np.array(out).reshape(-1, 4))


@pytest.mark.parametrize("task_type,micro_batch", [("wtw", 128), ("wtw", 2), ("wireless", 2)])
def test_stage_matches_many_seeded_lines(task_type, micro_batch):
    """TsrStage.__call__(text_boxes=...) with 40 seeded lines per table -- the seeded detector finds few: candidates are the lines
    texts_in_table chooses for the region, 'matched' is find_top1_match on the result's own cells; every other key is what the call without
    text_boxes returns.  micro_batch 2: several entries per call (the ResNet-18 variant keeps them apart), each with its own launch."""
    from pdf_table_amd.pipeline import OcrTablePipeline
    p = OcrTablePipeline(device=0, synthetic_seed=0, table_structure=True, table_structure_task_type=task_type)
    stage = p.table_structure_task._stage
    stage.micro_batch = micro_batch
    made = [make_page(i) for i in (0,) + PAGES]
    pages = torch.from_numpy(np.stack([m[0] for m in made])).to(p.engine._tdev)
    # the pages' own table regions plus one seeded region per page: five or more tables, so micro_batch 2 gives three entries
    regions = [np.concatenate([np.asarray(m[1]["tables"]).reshape(-1, 4).astype(np.int64), np.array([[90 + 40 * k, 120, 700, 560 + 60 * k]])])
               for k, m in enumerate(made)]
    assert sum(len(r) for r in regions) >= 5
    rng = np.random.default_rng(21)
    tbx = [_seeded_text_boxes(rng, r, 40) for r in regions]
    plain = stage(pages, regions, page_frame=True)
    got = stage(pages, regions, page_frame=True, text_boxes=tbx)
    again = stage(pages, regions, page_frame=True, text_boxes=tbx)
    with pytest.raises(ValueError):
        stage(pages, regions, page_frame=False, text_boxes=tbx)
    p.engine.close()
    n_lines = 0
    for k in range(len(regions)):
        for ti, (ta, tb, tc) in enumerate(zip(plain[k], got[k], again[k])):
            assert set(tb) == set(ta) | {"matched", "matched_lines"}
            for key in ta:
                assert np.array_equal(np.asarray(ta[key]), np.asarray(tb[key])), key
            assert np.array_equal(tb["matched"], tc["matched"]) and np.array_equal(tb["matched_lines"], tc["matched_lines"])
            if len(tb["scores"]) == 0:
                assert len(tb["matched"]) == 0 and len(tb["matched_lines"]) == 0
                continue
            inside = texts_in_table([float(v) for v in regions[k][ti]], tbx[k], diff=2)
            assert np.asarray(tb["matched_lines"]).tolist() == inside.tolist()
            want = sorted_match_to_rows(tb["polygons"], tb["logi"], tbx[k][inside])
            assert np.asarray(tb["matched"]).tolist() == want.tolist()
            n_lines += len(inside)
    assert n_lines >= 60
