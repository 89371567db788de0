"""The text-line orientation vote on the host (no GPU): ClsStage.page_votes -- predict_stream(orientation_vote=True)'s vectorised vote -- decides
exactly as orientation_vote() over topk_postprocess's per-line dicts, also where the top-1 score lands on the 0.9 threshold after rounding; and the
fitted synthetic head (pplcnet_state_dict(textline_head=True), tools/fit_textline_head.py) makes the fp32 oracle vote a generator page upright and
its 180-degree copy upside-down."""
import importlib.util
import os

import numpy as np
import torch

from pdf_table_amd.cls_stage import ClsStage, topk_postprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dict_votes(stage, logits, counts):
    res = topk_postprocess(logits, "textline_orientation")
    out, o = [], 0
    for c in counts:
        out.append(stage.orientation_vote(res[o:o + c]))
        o += c
    return out


def _boundary_logits(rng, n):
    """logit pairs whose soft-max top-1 probability sits within a few float32 ulps of 0.9 and 0.899995 / 0.900005 (the 5-decimal rounding edges)"""
    target = np.array([0.9, 0.899995, 0.900005, 0.8999949, 0.9000051], np.float64)
    p = rng.choice(target, n) + rng.integers(-8, 9, n) * 2.0 ** -24
    d = np.log(p / (1 - p)).astype(np.float32)              # l0 - l1
    sign = rng.choice([-1.0, 1.0], n).astype(np.float32)
    base = rng.normal(0, 3, n).astype(np.float32)
    return np.stack([base + sign * d / 2, base - sign * d / 2], 1).astype(np.float32)


def test_page_votes_equal_dict_votes_on_the_rounding_boundary():
    stage = ClsStage(None, "textline_orientation")
    rng = np.random.default_rng(7)
    checked = differs_f32 = 0
    for _ in range(200):
        counts = rng.integers(0, 9, rng.integers(1, 6))
        lg = _boundary_logits(rng, int(counts.sum()))
        got = stage.page_votes(lg, counts)
        assert got.tolist() == _dict_votes(stage, lg, counts)
        checked += len(counts)
        if len(lg):       # top1() rounds in float32: other score values than the dicts' on these lines -- the case the vote must not depend on
            ids, sc32 = stage.top1(torch.from_numpy(lg))
            sc64 = [r["scores"][0] for r in topk_postprocess(lg, "textline_orientation")]
            differs_f32 += int(np.sum(sc32 != np.array(sc64)))
    assert checked > 300 and differs_f32 > 0
    # ties, empty pages and a page with no line above the threshold
    lg = np.array([[0.0, 0.0], [5.0, 0.0], [0.0, 5.0], [0.1, 0.0]], np.float32)
    for counts in ([4], [1, 0, 3], [0, 0, 2, 2], [2, 2]):
        assert stage.page_votes(lg, counts).tolist() == _dict_votes(stage, lg, counts)
    assert stage.page_votes(np.zeros((0, 2), np.float32), [0, 0]).tolist() == [False, False]


def test_fitted_head_votes_as_recorded():
    spec = importlib.util.spec_from_file_location("fit_textline_head", os.path.join(ROOT, "tools", "fit_textline_head.py"))
    fit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fit)
    from pdf_table_amd.synth_pages import make_page
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    sd = {k: torch.as_tensor(np.asarray(v)).float() for k, v in pplcnet_state_dict(seed=5, class_num=2, textline_head=True).items()}
    plain = pplcnet_state_dict(seed=5, class_num=2)
    assert not torch.equal(plain["fc.weight"], sd["fc.weight"])          # the overlay is opt-in: the default weights are untouched
    assert all(torch.equal(plain[k], sd[k]) for k in plain if not k.startswith("fc."))
    img, meta = make_page(1)
    for flipped in (False, True):
        im = np.ascontiguousarray(img[::-1, ::-1]) if flipped else img
        q = fit.rect_quads(meta["lines"], img.shape[0], flipped)     # the generator's lines (the DB oracle's boxes are slower to get)
        up, n_up, n_down = fit.oracle_votes(sd, im, q)
        assert up == (not flipped), (flipped, n_up, n_down)
