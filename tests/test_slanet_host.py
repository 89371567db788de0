"""Host half of the SLANet door (no GPU): TableLabelDecode and the post-processor's shaping (pdf_table_amd/rec_postprocess.py) against goldens
recorded from the reference's own TableLabelDecode (tests/golden/slanet_decode.json, written by tests/golden/make_slanet_golden.py), the
pre-processing restatement of tests/slanet_ref.py on known answers, the head packer's layout, and the two refusals that need no device."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slanet_ref as R  # noqa: E402
from pdf_table_amd.rec_postprocess import TableLabelDecode, slanet_shape_result  # noqa: E402
from pdf_table_amd.slanet_stage import slanet_resized_size, slanet_shape_list  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "slanet_decode.json")) as f:
        return json.load(f)


def _decode(lang):
    return TableLabelDecode(os.path.join(GOLDEN, "slanet", "table_structure_dict%s.txt" % ("_ch" if lang == "ch" else "")), merge_no_span_structure=True)


@pytest.mark.parametrize("lang,V,L", [("en", 30, 4), ("ch", 50, 8)])
def test_table_label_decode_matches_the_reference(golden, lang, V, L):
    g = golden[lang]
    dec = _decode(lang)
    assert dec.character == g["characters"] and len(dec.character) == V == g["V"] and g["L"] == L
    assert dec.character[0] == "sos" and dec.character[-1] == "eos" and "<td>" not in dec.character and dec.character.count("<td></td>") == 1
    probs, loc, shapes = np.array(g["structure_probs"], np.float32), np.array(g["loc_preds"], np.float32), np.array(g["shape_list"], np.float32)
    ids = probs.argmax(2)
    # the cases the golden was built for
    assert ids[0, 0] == V - 1 and ids[1, 1] == V - 1 and (ids[2] != V - 1).all() and ids[3, 3] == 0 and (ids[4, 0], ids[4, 1]) == (0, V - 1)
    steps = np.array([next((t + 1 for t in range(1, ids.shape[1]) if ids[b, t] == V - 1), ids.shape[1]) for b in range(len(ids))])
    for res in (dec({"structure_probs": probs, "loc_preds": loc.copy()}, [shapes]),                    # the reference's call shape
                dec.decode_ids(ids, probs.max(2), loc.copy(), shapes),                                 # what the stage has: ids, chosen probability
                dec.decode_ids(ids, probs.max(2), loc.copy(), shapes, steps)):                         # ... and the head's step counts
        for b, (toks, score) in enumerate(g["structure_batch_list"]):
            got_toks, got_score = res["structure_batch_list"][b]
            assert got_toks == toks, (lang, b)
            if score is None:
                assert np.isnan(got_score)
            else:
                assert np.float32(got_score) == np.float32(score), (lang, b, got_score, score)
            want = np.array(g["bbox_batch_list"][b], np.float32).reshape(-1, L)
            got = np.asarray(res["bbox_batch_list"][b], np.float32).reshape(-1, L)
            assert got.shape == want.shape and np.array_equal(got, want), (lang, b)
    assert [len(s[0]) for s in g["structure_batch_list"]] == [5, 1, 10, 9, 0]


def test_post_processor_shaping():
    r = slanet_shape_result(["<tr>", "<td></td>", "</tr>"], np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]], np.float32), inputs="img")
    assert r["structure_str_list"] == ["<html>", "<body>", "<table>", "<tr>", "<td></td>", "</tr>", "</table>", "</body>", "</html>"]
    assert np.array_equal(r["polygons"], np.array([[1, 2, 3, 2, 3, 4, 1, 4], [5, 6, 7, 6, 7, 8, 5, 8]], np.float32)) and r["inputs"] == "img"
    eight = np.arange(16, dtype=np.float32).reshape(2, 8)
    assert np.array_equal(slanet_shape_result([], eight)["polygons"], eight)                           # 8-value boxes pass through
    empty = slanet_shape_result([], np.array([]))
    assert empty["polygons"].shape == (0,) and empty["structure_str_list"] == ["<html>", "<body>", "<table>", "</table>", "</body>", "</html>"]


@pytest.mark.parametrize("h,w,rh,rw", [(3, 5, 292, 488), (200, 200, 488, 488), (976, 640, 488, 320), (100, 333, 146, 488), (333, 1000, 162, 488)])
def test_resized_size_truncates(h, w, rh, rw):
    """int() truncation of the resized size: 3 x 5 -> 292.8 -> 292; 100 x 333 -> 146.5 -> 146; 333 x 1000 -> 162.504 -> 162"""
    got = slanet_resized_size(h, w)
    assert got[:2] == (rh, rw) and got[2] == 488 / max(h, w)
    assert np.array_equal(slanet_shape_list(h, w), np.array([h, w, got[2], got[2], 488, 488]))
    assert slanet_resized_size(h, w, 96)[:2] == (int(h * (96 / max(h, w))), int(w * (96 / max(h, w))))


@pytest.mark.parametrize("h,w", [(3, 5), (61, 61), (976, 640), (100, 333)])
def test_preprocess_restatement_known_answers(h, w):
    """a 3 x 5 crop, a square one, one with max(h, w) > 488 and one < 488.  A constant image has a closed form: every resized pixel is the
    constant (bilinear weights sum to one), so the tensor is ((v / 255 - mean[c]) / std[c]) with c in B, G, R order inside the resized
    rectangle and exactly zero outside"""
    img = np.empty((h, w, 3), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 200, 100, 50                                                # R, G, B
    x, shape = R.slanet_preprocess(img)
    rh, rw, ratio = slanet_resized_size(h, w)
    assert x.shape == (3, 488, 488) and x.dtype == np.float32 and np.array_equal(shape, [h, w, ratio, ratio, 488, 488])
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    for c, v in enumerate((50, 100, 200)):                                                              # channel 0 is B
        want = (np.float32(v) * np.float32(1.0 / 255.0) - mean[c]) / std[c]
        assert (x[c, :rh, :rw] == want).all()
        assert not x[c, rh:].any() and not x[c, :, rw:].any()


def test_preprocess_restatement_half_and_same_size():
    """OpenCV's two short cuts: a 488-long crop is copied, a 976-long one is 2 x 2 means (rounded half up)"""
    g = np.random.default_rng(0)
    same = g.integers(0, 256, (300, 488, 3), dtype=np.uint8)
    x, _ = R.slanet_preprocess(same)
    back = np.round((x[:, :300] * np.array([0.229, 0.224, 0.225], np.float32)[:, None, None] + np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]) * 255.0)
    assert np.array_equal(back.transpose(1, 2, 0)[..., ::-1].astype(np.uint8), same)
    big = g.integers(0, 256, (976, 400, 3), dtype=np.uint8)
    x, _ = R.slanet_preprocess(big)
    mean4 = (big.astype(np.int64).reshape(488, 2, 200, 2, 3).sum((1, 3)) + 2) >> 2
    back = np.round((x[:, :, :200] * np.array([0.229, 0.224, 0.225], np.float32)[:, None, None] + np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]) * 255.0)
    assert np.array_equal(back.transpose(1, 2, 0)[..., ::-1].astype(np.int64), mean4)


def test_pack_sla_head_layout():
    """the packed images against the sizes the library reports, and a few entries against the layout the kernel indexes"""
    from pdf_table_amd import lib as L
    from pdf_table_amd import weights as W
    H, Cc, V, Lo = 64, 40, 30, 4
    p = R.make_head(5, H, Cc, V, Lo)
    w16, vec = W.pack_sla_head(p, fmt="bf16", split=True)
    lib = L.load()
    n16, n32 = C.c_longlong(), C.c_longlong()
    assert lib.pt_op_sla_packed_elems(H, Cc, V, Lo, C.byref(n16), C.byref(n32)) == 0
    assert w16.shape == (2, n16.value) and vec.shape == (n32.value,) and w16.dtype == np.uint16
    import torch
    val = torch.from_numpy(w16.view(np.int16)).view(torch.bfloat16).double().sum(0).numpy()           # hi + lo
    A = np.concatenate([p["h2h_w"], p["w_hh"], p["s1_w"], p["l1_w"]], 0)
    for r, k in ((0, 0), (5, 9), (6 * H - 1, H - 1), (3 * H + 7, 33)):
        assert abs(val[(k // 8) * 6 * H * 8 + r * 8 + k % 8] - A[r, k]) <= 2.0 ** -16 * abs(A[r, k])
    col = 6 * H * H + 3 * H * 40
    assert abs(val[col + 11 * 3 * H + 17] - p["w_ih"][17, Cc + 11]) <= 2.0 ** -16 * abs(p["w_ih"][17, Cc + 11])
    assert np.array_equal(vec[9 * H:10 * H], p["score_w"].astype(np.float32)) and np.array_equal(vec[10 * H + 64:10 * H + 68], p["l2_b"].astype(np.float32))
    assert lib.pt_op_sla_packed_elems(48, Cc, V, Lo, C.byref(n16), C.byref(n32)) == 1 and b"hidden size 48" in lib.pt_last_error()
    with pytest.raises(ValueError):
        W.pack_sla_head(R.make_head(5, 48, Cc, V, Lo))


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pdftable_hip.h")).read()
    for name in ("pt_op_sla_decode", "pt_op_sla_packed_elems", "pt_op_sla_scratch_bytes", "pt_slanet_preprocess"):
        assert f"int {name}(" in hdr
    from pdf_table_amd import lib as L
    L.load()
    assert L.EXPECTED_ABI == 21 and {"pt_op_sla_decode", "pt_slanet_preprocess"} <= set(L.EXPORTS)    # added under ABI 19; 20 added pt_op_mtl_*, 21 the Lore processor's op entries


def test_refusals_without_a_device(tmp_path):
    from pdf_table_amd.ocr_table_structure_task import OcrTableStructureTask
    from pdf_table_amd.pipeline import OcrTablePipeline
    with pytest.raises(RuntimeError, match="ONNX-only"):
        OcrTableStructureTask(model="SLANet", synthetic_seed=0)
    with pytest.raises(RuntimeError, match="ONNX-only"):
        OcrTableStructureTask(model="SLANet", task_path=str(tmp_path))                                 # a directory without model.onnx
    with pytest.raises(ValueError, match="out of scope"):
        OcrTablePipeline(table_structure=True, table_structure_model="SLANet")                         # in the constructor, before any engine exists
