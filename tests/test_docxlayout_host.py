"""DocXLayout without a GPU: the CPU restatement (tests/docxlayout_ref.py) against the reference's fixtures, the product's host half against
the same fixtures, known answers for the polygon overlap and the comparator sort, the checkpoint loader, the packer, the documented
refusals."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docxlayout_ref as R  # noqa: E402
import docxlayout_synth as S  # noqa: E402
from pdf_table_amd.docxlayout_stage import (DocXLayoutConfig, docx_page_result, load_checkpoint, quad_intersection_rate,  # noqa: E402
                                            sort_blocks)
from pdf_table_amd.synth_weights import centernet_dla34_state_dict, docxlayout_dla34_state_dict  # noqa: E402
from pdf_table_amd.weights import DOCX_HEADS, pack_docxlayout_dla34  # noqa: E402


@pytest.fixture(scope="module")
def post(golden_dir):
    with open(os.path.join(golden_dir, "docxlayout_post.json")) as f:
        return np.load(os.path.join(golden_dir, "docxlayout_post.npz")), json.load(f)


def _tags():
    return [(c, s) for s in S.SIZES for c in S.REF_CASES]


def _same_lists(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for g, w in zip(got, want):
        assert [float(v) for v in g["bbox"]] == w["bbox"] and g["label"] == w["label"] and g["category_id"] == w["category_id"], (what, g, w)
        assert float(g["score"]) == w["score"], (what, g, w)


def test_restated_net_matches_reference_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, "docxlayout_dla34.npz"))
    sd = docxlayout_dla34_state_dict(seed=int(gold["seed"]))
    for tag in ("a", "b"):
        with torch.no_grad():
            z = R.docx_forward(sd, torch.from_numpy(gold[f"x_{tag}"]).double())
        for k in R.HEADS:
            ref = gold[f"{k}_{tag}"]
            err = np.abs(z[k].numpy() - ref).max() / max(1.0, np.abs(ref).max())
            assert err <= 1e-5, (tag, k, err)      # float64 against float64 stored as float32


@pytest.mark.parametrize("case,size", _tags())
def test_restated_decode_and_chain_match_reference(post, case, size):
    npz, js = post
    tag = f"{case}_{size[0]}x{size[1]}"
    z = S.make_case(case, size)
    m, _ = R.branch_list(z["hm"][0], z["wh"][0], z["reg"][0], z["cls"][0], z["ftype"][0])
    s, _ = R.branch_list(z["hm_sub"][0], z["wh_sub"][0], z["reg_sub"][0])
    for name, rec, shift in (("main", m, 0), ("sub", s, 11)):
        ref = npz[f"dets_{name}_{tag}"]
        ref = ref[ref[:, 8] >= R.THR_LO]
        rec = rec.copy()
        rec[:, 9] += shift
        if name == "sub":      # the reference copies the main branch's arg-max columns of the same rank; nothing reads them
            ref, rec = ref[:, :10], rec[:, :10]
        assert np.array_equal(rec, ref), (tag, name)
        kept = npz[f"kept_{name}_{tag}"]
        mine = rec[R.pnms_keep(rec)]
        assert np.array_equal(mine, kept[:, :rec.shape[1]]), (tag, name, "pnms")
    _same_lists(R.page_result(m[R.pnms_keep(m)], s[R.pnms_keep(s)], S.page_hw(size), size), js[tag], tag)


@pytest.mark.parametrize("case,size", _tags())
def test_product_host_half_matches_reference(post, case, size):
    """the fixture's rows behind pnms -> the final lists: integers and two-decimal scores equal"""
    npz, js = post
    tag = f"{case}_{size[0]}x{size[1]}"
    main, sub = npz[f"kept_main_{tag}"].copy(), npz[f"kept_sub_{tag}"].copy()
    sub[:, 9] -= 11      # the device writes the branch's own 0-based classes
    _same_lists(docx_page_result(main, sub, S.page_hw(size), size, DocXLayoutConfig()), js[tag], tag)


def test_polygon_rate_known_answers():
    sq = [0, 0, 4, 0, 4, 4, 0, 4]
    assert quad_intersection_rate(sq, sq) == 1.0                                          # identical
    assert quad_intersection_rate(sq, [2, 0, 6, 0, 6, 4, 2, 4]) == 0.5                    # axis-aligned, half covered
    assert quad_intersection_rate(sq, [2, 2, 6, 2, 6, 6, 2, 6]) == 0.25
    assert quad_intersection_rate(sq, [5, 5, 7, 5, 7, 7, 5, 7]) == 0.0                    # disjoint
    assert quad_intersection_rate(sq, [4, 0, 8, 0, 8, 4, 4, 4]) == 0.0                    # sharing an edge only
    cw = [0, 0, 0, 4, 4, 4, 4, 0]                                                         # the same square, clockwise
    assert quad_intersection_rate(cw, sq) == 1.0 and quad_intersection_rate(sq, cw) == 1.0
    diamond = [2, 0, 4, 2, 2, 4, 0, 2]                                                    # a 45-degree square inside the square: area 8
    assert quad_intersection_rate(diamond, sq) == 1.0 and quad_intersection_rate(sq, diamond) == 0.5
    big = [2, -2, 6, 2, 2, 6, -2, 2]                                                      # a 45-degree square around it: the square is inside
    assert quad_intersection_rate(sq, big) == 1.0 and quad_intersection_rate(big, sq) == 0.5
    assert quad_intersection_rate([1, 1, 3, 1, 3, 1, 1, 1], sq) == 0.0                    # zero area: 0, not a division by zero
    bow = [0, 0, 4, 4, 4, 0, 0, 4]                                                        # not convex: both bounding boxes
    assert quad_intersection_rate(bow, [2, 0, 6, 0, 6, 4, 2, 4]) == 0.5


def test_sort_with_a_comparison_cycle():
    """three blocks that beat one another in a circle: the result is list.sort's over the given order, and differs with the order"""
    def blk(name, x0, y0, x1, y1):
        return {"name": name, "pts": [float(v) for v in (x0, y0, x1, y0, x1, y1, x0, y1)]}
    from functools import cmp_to_key
    from pdf_table_amd.docxlayout_stage import _compare_rects

    def rect(p):
        return (p["pts"][0], p["pts"][1], p["pts"][2] - p["pts"][0], p["pts"][5] - p["pts"][1])
    tall = blk("t", 0, 0, 10, 30)           # spans both rows
    up_right = blk("u", 12, 0, 22, 10)      # first row, right of t
    low_left = blk("l", -12, 18, -2, 28)    # second row, left of t
    cmp = lambda p, q: _compare_rects(rect(p), rect(q))
    assert cmp(tall, up_right) == -1 and cmp(up_right, low_left) == -1 and cmp(low_left, tall) == -1      # t < u < l < t
    for order in ([tall, up_right, low_left], [low_left, tall, up_right], [up_right, low_left, tall]):
        mine = [dict(p) for p in order]
        want = [dict(p) for p in order]
        sort_blocks(mine)
        R.sort_pts(want)
        assert [p["name"] for p in mine] == [p["name"] for p in want]
        assert [p["name"] for p in mine] == [p["name"] for p in sorted(order, key=cmp_to_key(cmp))]
    firsts = set()
    for order in ([tall, up_right, low_left], [low_left, tall, up_right], [up_right, low_left, tall]):
        mine = [dict(p) for p in order]
        sort_blocks(mine)
        firsts.add(mine[0]["name"])
    assert len(firsts) > 1


def test_checkpoint_loader_forms(tmp_path):
    sd = docxlayout_dla34_state_dict(seed=2)
    f = tmp_path / "model.pth"
    torch.save(sd, str(f))
    got = load_checkpoint(str(f))
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    d = tmp_path / "dir"
    d.mkdir()
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}}, str(d / "pytorch_model.bin"))
    got = load_checkpoint(str(d))
    assert set(got) == set(sd) and torch.equal(got["hm.2.bias"], sd["hm.2.bias"])
    d2 = tmp_path / "dir2"
    d2.mkdir()
    torch.save({"state_dict": sd}, str(d2 / "docx.pth"))
    assert set(load_checkpoint(str(d2))) == set(sd)
    torch.save(sd, str(d2 / "second.pth"))
    with pytest.raises(RuntimeError, match="single"):
        load_checkpoint(str(d2))
    short = {k: v for k, v in sd.items() if k != "wh_sub.2.weight"}
    torch.save(short, str(tmp_path / "short.pt"))
    with pytest.raises(KeyError, match="wh_sub.2.weight"):
        load_checkpoint(str(tmp_path / "short.pt"))
    with pytest.raises(RuntimeError, match="no DocXLayout checkpoint"):
        load_checkpoint(str(tmp_path / "missing.pth"))


def test_pack_names_and_rejects_centernet():
    sd = docxlayout_dla34_state_dict(seed=1)
    assert [h for h, _ in DOCX_HEADS] == sorted(R.HEADS) and dict(DOCX_HEADS) == R.HEADS
    for h, k in DOCX_HEADS:
        assert tuple(sd[f"{h}.0.weight"].shape) == (256, 64, 3, 3) and tuple(sd[f"{h}.2.weight"].shape) == (k, 256, 1, 1)
        assert tuple(sd[f"{h}.0.bias"].shape) == (256,) and tuple(sd[f"{h}.2.bias"].shape) == (k,)
    blob = pack_docxlayout_dla34({"module." + k: v for k, v in sd.items()})
    assert blob[:4] == b"PTW1" and blob == pack_docxlayout_dla34(sd)
    with pytest.raises(KeyError, match="DocXLayout DLA-34 state_dict lacks 'cls.0.weight'"):
        pack_docxlayout_dla34(centernet_dla34_state_dict(seed=1))


def test_abi_constants():
    import re
    from pdf_table_amd import lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pdftable_hip.h")).read()
    assert re.search(r"PT_MODEL_DOCX_DLA34\s*=\s*20\b", hdr) and L.PT_MODEL_DOCX_DLA34 == 20
    assert re.search(r"#define PT_DOCX_REC_FLOATS 12\b", hdr) and re.search(r"#define PT_DOCX_MAX_K 128\b", hdr)
    assert (L.PT_DOCX_REC_FLOATS, L.PT_DOCX_MAX_K) == (12, 128)


def test_pipeline_refuses_docxlayout_without_a_checkpoint():
    """before an engine exists: needs no GPU"""
    from pdf_table_amd.pipeline import OcrTablePipeline
    with pytest.raises(ValueError, match="layout_task_path"):
        OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout")
    with pytest.raises(ValueError, match="layout_precision"):
        OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path="/nowhere", layout_precision="fp32")
    with pytest.raises(ValueError, match="layout_device_decode"):
        OcrTablePipeline(synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path="/nowhere", layout_device_decode=True)


def test_task_refuses_docxlayout_without_a_checkpoint():
    """the refusal comes before the engine is created: needs no GPU"""
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    with pytest.raises(RuntimeError, match="task_path"):
        OcrLayoutTask(model="DocXLayout", synthetic_seed=0)
    with pytest.raises(RuntimeError, match="task_path"):
        OcrLayoutTask(model="DocXLayout")
    with pytest.raises(ValueError, match="device_decode"):
        OcrLayoutTask(model="DocXLayout", task_path="/nowhere", device_decode=True)
