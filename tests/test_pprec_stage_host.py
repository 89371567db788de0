"""Host side of the PP-OCR recognition stage (pdf_table_amd/pprec_stage.py), no GPU: the decode-and-scatter half on hand-made ids / probabilities,
the width-bucket arithmetic of rec_pp_plan, the executor's CTC-tail plan on a layer list, and the new entry point in header, library and binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from pdf_table_amd import lib as L
from pdf_table_amd.pprec_stage import pprec_decode_host
from pdf_table_amd.rec_postprocess import CTCLabelDecode
from pdf_table_amd.rec_pp_stage import PPOcrRecConfig, rec_pp_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_scatters_to_page_and_line_order():
    """7 lines on 3 pages (3, 0, 4); lines 1 and 5 have no crop.  The 5 kept lines come width-sorted in two mini-batches (3 lines of 4 tokens,
    2 lines of 6 tokens), flat and back to back as the stage's pinned buffer holds them."""
    ctc = CTCLabelDecode(characters=list("abcd"))                       # ids: 0 blank, 1 a, 2 b, 3 c, 4 d
    kept = np.array([1, 0, 1, 1, 1, 0, 1], bool)                        # kept lines, in page order: 0, 2, 3, 4, 6
    indices = np.array([3, 0, 4, 2, 1])                                 # processing order over the KEPT lines -> page-batch lines 4, 0, 6, 3, 2
    mb0 = np.array([[1, 1, 0, 2], [0, 0, 0, 0], [3, 0, 3, 3]])          # "ab", "", "cc"
    pb0 = np.array([[0.5, 0.9, 0.1, 0.7], [0.3, 0.3, 0.3, 0.3], [1.0, 0.2, 0.5, 0.25]], np.float32)
    mb1 = np.array([[4, 4, 4, 0, 0, 1], [2, 0, 2, 0, 2, 0]])            # "da", "bbb"
    pb1 = np.array([[0.25, 0.5, 0.75, 0.1, 0.1, 1.0], [0.5, 0.1, 0.25, 0.1, 0.75, 0.1]], np.float32)
    ids = np.concatenate([mb0.reshape(-1), mb1.reshape(-1)]).astype(np.int32)
    conf = np.concatenate([pb0.reshape(-1), pb1.reshape(-1)])
    spans = [(0, 3, 4, 0), (3, 2, 6, 12)]
    texts, scores = pprec_decode_host(ctc, ids, conf, spans, indices, kept, [3, 0, 4])
    assert texts == [["", "", "bbb"], [], ["da", "ab", "", "cc"]]
    #            line 0: all blank -> [0] -> 0; line 1 dropped; line 2: mean(0.5, 0.25, 0.75)
    want = [[0.0, 0.0, 0.5], [], [np.mean([0.25, 1.0]), np.mean([0.5, 0.7]), 0.0, np.mean([1.0, 0.5])]]
    assert [len(s) for s in scores] == [3, 0, 4]
    for got, w in zip(scores, want):
        assert np.allclose(got, w, rtol=1e-6, atol=0)
    assert all(isinstance(s, float) for pg in scores for s in pg)
    # nothing kept (every quad degenerate, or no box at all): empty strings, zero scores, no ids needed
    texts, scores = pprec_decode_host(ctc, np.zeros(0, np.int32), np.zeros(0, np.float32), [], None, np.zeros(2, bool), [2, 0])
    assert texts == [["", ""], []] and scores == [[0.0, 0.0], []]
    with pytest.raises(ValueError):
        pprec_decode_host(ctc, ids, conf, spans, indices, kept, [3, 3])


def test_width_bucket_plan():
    rng = np.random.default_rng(3)
    w = rng.integers(8, 900, 23)
    h = rng.integers(8, 60, 23)
    for cfg_kw in ({}, {"rec_image_shape": "3, 48, 320", "limited_max_width": 320}, {"rec_batch_num": 64}, {"limited_max_width": 1000}):
        items0, batches0, total0 = rec_pp_plan(w, h, PPOcrRecConfig(**cfg_kw))
        same = rec_pp_plan(w, h, PPOcrRecConfig(rec_width_bucket=None, **cfg_kw))
        assert np.array_equal(items0, same[0]) and batches0 == same[1] and total0 == same[2]      # the default: the reference's plan, unchanged
        cfg = PPOcrRecConfig(rec_width_bucket=32, **cfg_kw)
        items, batches, total = rec_pp_plan(w, h, cfg)
        assert np.array_equal(items["line"], items0["line"]) and np.array_equal(items["resized_w"], items0["resized_w"])   # same crops, same pixels
        assert [(b[0], b[1]) for b in batches] == [(b[0], b[1]) for b in batches0]
        off = 0
        for (beg, n, img_w, o), (_, _, img_w0, _) in zip(batches, batches0):
            assert img_w == max(img_w0, min(-(-img_w0 // 32) * 32, cfg.limited_max_width)) and img_w0 <= img_w < img_w0 + 32
            assert img_w % 32 == 0 or img_w == cfg.limited_max_width
            assert o == off and (items["img_w"][beg:beg + n] == img_w).all() and (items["resized_w"][beg:beg + n] <= img_w).all()
            assert list(items["out_off"][beg:beg + n]) == [off + i * 3 * 48 * img_w for i in range(n)]
            off += n * 3 * 48 * img_w
        assert total == off
    assert len({b[2] for b in rec_pp_plan(w, h, PPOcrRecConfig(rec_width_bucket=256))[1]}) <= 5      # a bucket bounds the distinct widths
    with pytest.raises(ValueError):
        PPOcrRecConfig(rec_width_bucket=0)


def test_ctc_tail_plan_on_layer_lists():
    """the planner alone, on hand-made layer lists: the one Softmax that is the single output and unread -> its index; anything else -> None"""
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    from pdf_table_amd.onnx_import import Layer

    def plan(layers, outputs):
        ex = HipGraphExecutor.__new__(HipGraphExecutor)
        ex.layers, ex.outputs = layers, outputs
        return ex._plan_ctc_tail()
    fc = Layer("gemm", "fc", ["h"], ["logits"], {})
    sm = Layer("act", "sm", ["logits"], ["y"], {"kind": "softmax", "axis": -1})
    assert plan([fc, sm], ["y"]) == 1
    assert plan([fc], ["logits"]) is None                                                      # logits out
    assert plan([fc, sm], ["y", "logits"]) is None                                             # a second output
    assert plan([fc, sm, Layer("act", "r", ["y"], ["z"], {"kind": "relu"})], ["y"]) is None    # something else reads the Softmax
    assert plan([fc, Layer("act", "r", ["logits"], ["y"], {"kind": "relu"})], ["y"]) is None


def test_new_entry_point_in_header_library_and_binding():
    from pdf_table_amd.build import build
    hdr = open(os.path.join(REPO, "include", "pdftable_hip.h")).read()
    assert re.search(r"\bint pt_op_ctc_greedy\(pt_engine\* e, const uint16_t\* d_in, long long rows, int c_pad, int c, int32_t\* d_ids, float\* d_conf, "
                     r"int split, pt_stream stream\);", hdr)
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "pt_op_ctc_greedy")
    bound = L.load()
    assert "pt_op_ctc_greedy" in L.EXPORTS and L.EXPECTED_ABI == 21 == lib.pt_abi_version()     # added under ABI 19; 20 added pt_op_mtl_*, 21 pt_op_lore_tok_prepare .. scatter4
    # bad arguments are refused before anything is launched (no device needed: the engine pointer is checked first)
    assert bound.pt_op_ctc_greedy(None, None, 1, 8, 1, None, None, 0, None) != 0
    assert b"pt_op_ctc_greedy" in bound.pt_last_error()
