"""Host side of the ONNX layout stage (pdf_table_amd/layout_stage.py: OnnxLayoutStage), no GPU: the decode of candidate records as
pt_op_pico_candidates writes them (class PROBABILITIES, arrival order undefined) against the dense route on the arrays they were taken from, and
the stage's decision -- from host-known shapes alone -- between the device tail, the host route and a refusal."""
import types

import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.layout_stage import LayoutStage, OnnxLayoutStage, PicodetConfig
from pdf_table_amd.onnx_import import UnsupportedOnnxGraph

ANCHORS = (100 * 76, 50 * 38, 25 * 19, 13 * 10)        # 800 x 608 at strides 8 / 16 / 32 / 64


def _outputs(ncls, seed):
    """per level class probabilities [A_l, ncls] and distribution logits [A_l, 32]: a few clusters of anchors above the score threshold"""
    rng = np.random.default_rng(seed)
    scores, dists = [], []
    for A in ANCHORS:
        sc = rng.uniform(0.0, 0.45, (A, ncls)).astype(np.float32)
        hot = rng.choice(A, size=min(A // 4, 60), replace=False)
        sc[hot, rng.integers(0, ncls, len(hot))] = rng.uniform(0.45, 1.0, len(hot)).astype(np.float32)       # some land between thr_lo and 0.5
        scores.append(sc)
        dists.append((rng.standard_normal((A, 32)) * 2.0).astype(np.float32))
    return scores, dists


@pytest.mark.parametrize("task_type, ncls", [("en", 5), ("ch", 10)])
def test_decode_page_of_shuffled_records_equals_decode_outputs(task_type, ncls):
    cfg = PicodetConfig(task_type=task_type)
    assert len(cfg.labels) == ncls
    st = LayoutStage(None, cfg)
    org = (1024, 1024)
    scores, dists = _outputs(ncls, 7 + ncls)
    want = st.decode_outputs(scores, dists, org)
    recs = []
    for l, (sc, bd) in enumerate(zip(scores, dists)):
        keep = np.nonzero(sc.max(1) > np.float32(cfg.score_threshold - 1e-3))[0]
        r = np.zeros((len(keep), L.PT_LAYOUT_CAND_FLOATS), np.float32)          # the kernel's record: zeros up to 48 floats
        r[:, 0] = np.full(len(keep), l, np.int32).view(np.float32)
        r[:, 1] = keep.astype(np.int32).view(np.float32)
        r[:, 2:2 + ncls], r[:, 2 + ncls:2 + ncls + 32] = sc[keep], bd[keep]
        recs.append(r)
    rec = np.concatenate(recs, 0)
    rec = rec[np.random.default_rng(1).permutation(len(rec))]                    # arrival order
    got = st.decode_page(rec, org, probs=True)
    assert len(got) == len(want) >= 3
    for g, w in zip(got, want):
        assert g["label"] == w["label"] and g["category_id"] == w["category_id"]
        assert np.float64(g["score"]).tobytes() == np.float64(w["score"]).tobytes()
        assert g["bbox"].dtype == w["bbox"].dtype and g["bbox"].tobytes() == w["bbox"].tobytes()
    # the stage's own decode of landed records is the probs=True one (the in-tree stage's is not)
    onnx_stage = OnnxLayoutStage(None, types.SimpleNamespace(adt=torch.bfloat16, split=False), cfg)
    again = onnx_stage._decode_record_page(rec, org)
    assert [(g["label"], g["bbox"].tobytes()) for g in again] == [(w["label"], w["bbox"].tobytes()) for w in want]
    assert [g["bbox"].tobytes() for g in st._decode_record_page(rec, org)] != [w["bbox"].tobytes() for w in want]


def _act(b, a, c, cp, dtype=torch.bfloat16, seq=True):
    t = torch.zeros((b, 1, a, cp), dtype=dtype)
    return types.SimpleNamespace(t=t, c=c, seq=seq, shape=lambda: (b, a, c) if seq else (b, c, 1, a))


def test_output_check_picks_the_route():
    cfg = PicodetConfig(task_type="en")
    st = OnnxLayoutStage(None, types.SimpleNamespace(adt=torch.bfloat16, split=False), cfg)
    good = [_act(2, A, 5, 64) for A in ANCHORS] + [_act(2, A, 32, 64) for A in ANCHORS]
    assert st._check_outputs(good) is True
    # an fp32 output (a graph that ends in an fp32 Softmax), or more levels than a launch takes: the host route, not a refusal
    f32 = list(good)
    f32[0] = _act(2, ANCHORS[0], 5, 5, dtype=torch.float32)
    assert st._check_outputs(f32) is False
    five = [_act(2, 7, 5, 64)] * 5 + [_act(2, 7, 32, 64)] * 5
    assert st._check_outputs(five) is False
    # the synchronous route's refusals, same texts
    with pytest.raises(UnsupportedOnnxGraph, match=r"\[B, anchors, channels\] tensors are expected"):
        st._check_outputs([_act(2, 7, 5, 64, seq=False), _act(2, 7, 32, 64)])
    with pytest.raises(UnsupportedOnnxGraph, match="5 class scores and 32 distribution bins per anchor are expected for task_type 'en'"):
        st._check_outputs([_act(2, 7, 10, 64), _act(2, 7, 32, 64)])
    with pytest.raises(UnsupportedOnnxGraph, match="5 class scores and 32 distribution bins"):
        st._check_outputs([_act(2, 7, 5, 64), _act(2, 7, 16, 64)])
    # a ticket of the host route passes through finish() as it is
    assert st.finish(1, ("host", [[{"label": "text"}]]), (10, 10)) == [[{"label": "text"}]]
