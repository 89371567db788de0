"""Lore's heat-map head in one launch (conv3x3_pipe_persist_hm_kernel, pt_op_lore_hm_head): hm.0 (3x3 64 -> 256 + ReLU) with hm.2 (1x1 256 -> 2) in its
epilogue against the two launches it replaces.

The hidden values are the same bits in both forms (bias, ReLU, rounding to the 16-bit format -- saturating in f16 --), and each of the 256 products
hidden * w2 is exact in fp32 (two 16-bit significands), so the two forms add the same 256 numbers in different orders.  Bound per output, from the
standard error bound of a sum of n = 256 terms (+ bias) in any order, gamma_n <= 257 u with u = 2^-24, once for each form:

    |fused - two launches| <= 2 * 257 * 2^-24 * sum_ch |hidden_ch * w2_ch|  +  one fp32 ulp of |b2|

with the sum taken from the hidden map the two launches wrote.  Channels 2 .. 7 of the logit layout (zero weight rows: 0 + bias) are equal bits.
Shapes: one 16 x 32 tile; ragged last tile row and column (8 live rows / columns); 45 pixel tiles on the persistent form with runs of unequal length
(a run boundary must never split the two 128-channel halves of a pixel tile)."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.weights import tile_conv_weight

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _operands(n, H, W, seed, dtype, feat_scale=1.0, w1_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    fmt = "f16" if dtype == torch.float16 else "bf16"
    dev = torch.device("cuda", 0)
    feat = (torch.randn(n, H, W, 64, generator=g) * feat_scale).clamp(-6.0e4, 6.0e4)      # (the map itself stays inside the half format)
    w1 = torch.randn(256, 64, 3, 3, generator=g) * (2.0 / (9 * 64)) ** 0.5 * w1_scale     # zero-mean responses, small bias: about half of them below zero
    b1 = torch.randn(256, generator=g) * 0.1 * feat_scale * w1_scale
    w2 = torch.zeros(64, 256, 1, 1)
    w2[:2] = torch.randn(2, 256, 1, 1, generator=g) * 0.1
    b2 = torch.zeros(64)
    b2[:8] = torch.randn(8, generator=g)                                         # channels 2 .. 7: what a padded row leaves is 0 + bias
    w2r = w2[:2, :, 0, 0].to(dtype).double()                                     # the weights as both forms multiply them
    tile = lambda w: torch.from_numpy(tile_conv_weight(w, fmt).view(np.int16)).to(dev)
    return dict(feat=feat.to(dtype).to(dev), w1=tile(w1), b1=b1.to(dev), w2=tile(w2), b2=b2.to(dev), w2r=w2r, b2h=b2.numpy().astype(np.float32))


def _both(eng, ops, **kw):
    two = eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=False, logits_fill=7.5)
    one = eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=True, logits_fill=7.5, **kw)
    torch.cuda.synchronize()
    return one, two


def _check(one, two, ops, what):
    hid = two["hid"].cpu().double()                                               # [n, H, W, 256]
    a, b = one["logits"].cpu().numpy(), two["logits"].cpu().numpy()
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(hid.numpy()).all(), what
    cut = float((hid == 0).double().mean())
    s = torch.einsum("nhwc,oc->nhwo", hid.abs(), ops["w2r"].abs()).numpy()        # sum_ch |hidden_ch * w2_ch|
    bound = 2 * 257 * U * s + np.spacing(np.abs(ops["b2h"][:2])).astype(np.float64)
    diff = np.abs(a[..., :2].astype(np.float64) - b[..., :2].astype(np.float64))
    ratio = float((diff / bound).max())
    print(f"hm head {what}: ReLU cuts {cut:.2f} of the hidden values; max |fused - two| {diff.max():.3e}, worst ratio to the bound {ratio:.4f}; "
          f"{int((a[..., :2] != b[..., :2]).sum())} of {diff.size} logits differ")
    assert 0.2 < cut < 0.8, cut
    assert ratio <= 1.0, ratio
    assert np.array_equal(a[..., 2:].view(np.int32), b[..., 2:].view(np.int32)), what
    assert np.array_equal(b[..., 2:], np.broadcast_to(np.float32(0) + ops["b2h"][2:8], b[..., 2:].shape)), what


SHAPES = [
    pytest.param(1, 16, 32, {}, id="one_tile"),
    pytest.param(2, 24, 40, {}, id="ragged"),
    pytest.param(5, 48, 96, {"PT_CONV_PIPE": "5"}, id="45_tiles"),
    pytest.param(5, 48, 96, {"PT_CONV_PIPE": "5", "PT_CONV_PERSIST_GRID": "7"}, id="45_tiles_7_runs"),      # runs of 6 and 7 pixel tiles
]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("n,H,W,env", SHAPES)
def test_fused_head_against_the_two_launches(eng, fmt, n, H, W, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng.set_precision(L.PT_PRECISION_F16 if fmt == "f16" else L.PT_PRECISION_BF16)
    try:
        ops = _operands(n, H, W, seed=1000 * n + H + W, dtype=eng.act_dtype)
        one, two = _both(eng, ops)
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    _check(one, two, ops, f"[{fmt}] {n}x{H}x{W} {env}")


def test_f16_saturated_hidden_values(eng):
    """hidden values beyond 65504 are stored as 65504 by the two launches (MODE.FP16_OVFL); the fused epilogue rounds the same way"""
    eng.set_precision(L.PT_PRECISION_F16)
    try:
        ops = _operands(2, 24, 40, seed=5, dtype=eng.act_dtype, feat_scale=1.0e4, w1_scale=8.0)      # responses of sigma ~ 1.1e5
        one, two = _both(eng, ops)
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    hid = two["hid"].cpu().float()
    sat = float((hid == 65504.0).float().mean())
    print(f"saturated hidden values: {sat:.3f} of the map")
    assert sat > 0.01 and bool(torch.isfinite(hid).all())
    _check(one, two, ops, "[f16] saturated")


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_fused_head_is_deterministic(eng, fmt, monkeypatch):
    monkeypatch.setenv("PT_CONV_PIPE", "5")
    eng.set_precision(L.PT_PRECISION_F16 if fmt == "f16" else L.PT_PRECISION_BF16)
    try:
        ops = _operands(5, 48, 96, seed=11, dtype=eng.act_dtype)
        runs = []
        for _ in range(2):
            r = eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=True, want_sig=True)
            torch.cuda.synchronize()
            runs.append((r["logits"].cpu().numpy().view(np.int32), r["sig"].cpu().numpy().view(np.int32)))
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.abs(runs[0][0]).max() > 0


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("with_logits", [True, False], ids=["logits_and_scores", "scores_only"])
def test_fused_scores_are_the_sigmoid_launch_on_the_fused_logits(eng, fmt, with_logits):
    """the score map the sparse decode reads ([pixel][2]): the epilogue's value == lore_sigmoid_kernel's on the same logit, bit for bit -- also when the
    launch writes the scores alone, as pt_lore_forward_decode's does"""
    eng.set_precision(L.PT_PRECISION_F16 if fmt == "f16" else L.PT_PRECISION_BF16)
    try:
        ops = _operands(2, 24, 40, seed=21, dtype=eng.act_dtype)
        r = eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=True, want_sig=True, want_sig_ref=True)
        sig = r["sig"]
        if not with_logits:
            B, H, W, _ = ops["feat"].shape
            sig = torch.zeros((B, H, W, 2), dtype=torch.float32, device=ops["feat"].device)
            from pdf_table_amd.engine import _ptr
            L.check(eng.lib.pt_op_lore_hm_head(eng._h, _ptr(ops["feat"]), B, H, W, _ptr(ops["w1"]), _ptr(ops["b1"]), _ptr(ops["w2"]), _ptr(ops["b2"]), 1,
                                               None, None, _ptr(sig), None, eng._stream()), "pt_op_lore_hm_head")
        torch.cuda.synchronize()
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    a, b = sig.cpu().numpy(), r["sig_ref"].cpu().numpy()
    lg = r["logits"].cpu().numpy()[..., :2]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.allclose(b, 1.0 / (1.0 + np.exp(-lg.astype(np.float64))), rtol=0, atol=1e-6)
    assert 0.0 < b.min() and b.max() < 1.0 and b.std() > 0.01


def test_switch_and_bad_arguments(eng, monkeypatch):
    from pdf_table_amd.lib import PtError
    ops = _operands(1, 16, 32, seed=3, dtype=torch.bfloat16)
    with pytest.raises(ValueError):          # the two launches have no score output of their own
        eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=False, want_sig=True)
    monkeypatch.setenv("PT_LORE_HM_FUSE", "0")
    with pytest.raises(PtError):             # switched off: an error, not a quiet pair of launches
        eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=True)
    monkeypatch.delenv("PT_LORE_HM_FUSE")
    monkeypatch.setenv("PT_CONV_PIPE", "3")  # the kernel families before the persistent tile: the two launches
    with pytest.raises(PtError):
        eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=True)
    monkeypatch.delenv("PT_CONV_PIPE")
    assert eng.op_lore_hm_head(ops["feat"], ops["w1"], ops["b1"], ops["w2"], ops["b2"], fused=True)["logits"].shape == (1, 16, 32, 8)


# ---- net level ------------------------------------------------------------------------------------------------------------------------------

def _input():
    n, H, W = 3, 64, 96            # maps of 16 x 24 (test_gpu_ida_fused_up.py's input)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, H, W, 3, generator=g) * 0.7
    x4 = torch.zeros(n, H, W, 4)
    x4[..., :3] = x.to(torch.bfloat16).float()
    return x4.to(torch.bfloat16).cuda()


@pytest.fixture(scope="module")
def lore_net():
    """(engine with the detector, per-pixel logit bound of the fused head on _input()).  The bound's sum_ch |hidden_ch * w2_ch| = sum_ch hidden_ch *
    |w2_ch| (hidden >= 0 behind the ReLU) is the hm logit of the same net with hm.2's weights replaced by their magnitudes and its bias by zero: taken
    from the two-launch path of a second engine loaded that way, widened by that GEMM's own rounding (257 u, relative)."""
    import os
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_weights import lore_dla34_state_dict
    from pdf_table_amd.weights import pack_lore_dla34
    sd = lore_dla34_state_dict(seed=2, hm_bias=(-1.2, -0.6))      # head biases near the thresholds: cells and corners on noise input
    mag = dict(sd)
    mag["hm.2.weight"] = sd["hm.2.weight"].to(torch.bfloat16).float().abs()
    mag["hm.2.bias"] = torch.zeros_like(sd["hm.2.bias"])
    e = HipEngine(0)
    e.load_weights(L.PT_MODEL_LORE_DLA34, pack_lore_dla34(mag))
    old = os.environ.get("PT_LORE_HM_FUSE")
    os.environ["PT_LORE_HM_FUSE"] = "0"
    try:
        s = e.tsr_forward_net(_input())["hm"].cpu().numpy().astype(np.float64)
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ["PT_LORE_HM_FUSE"]
        else:
            os.environ["PT_LORE_HM_FUSE"] = old
        e.close()
    assert s.min() >= 0 and s.max() > 0
    b2 = np.abs(sd["hm.2.bias"].numpy().astype(np.float32))
    bound = 2 * 257 * U * s * (1 + 257 * U) + np.spacing(b2).astype(np.float64)      # [n, h, w, 2]
    e = HipEngine(0)
    e.load_weights(L.PT_MODEL_LORE_DLA34, pack_lore_dla34(sd))
    yield e, bound
    e.close()


def test_net_logit_map_within_the_bound(lore_net, monkeypatch):
    e, bound = lore_net
    on = e.tsr_forward_net(_input())
    on = {k: v.cpu().numpy().copy() for k, v in on.items()}
    monkeypatch.setenv("PT_LORE_HM_FUSE", "0")
    off = {k: v.cpu().numpy().copy() for k, v in e.tsr_forward_net(_input()).items()}
    diff = np.abs(on["hm"].astype(np.float64) - off["hm"].astype(np.float64))
    print(f"net hm logits: max |fused - two| {diff.max():.3e}, worst ratio to the bound {(diff / bound).max():.4f}")
    assert np.isfinite(on["hm"]).all() and (diff <= bound).all()
    for k in ("st", "wh", "ax", "cr", "reg"):      # the other five heads keep their two launches
        assert np.array_equal(on[k].view(np.int32), off[k].view(np.int32)), k


def test_net_decode_with_the_switch_on_and_off(lore_net, monkeypatch):
    e, bound = lore_net
    xd = _input()
    c1, d1, l1 = e.tsr_forward_decode(xd, wiz_rev=True, vis_thresh=0.2, sync=True)
    c1, d1, l1 = np.asarray(c1).copy(), d1.cpu().numpy().copy(), l1.cpu().numpy().copy()
    monkeypatch.setenv("PT_LORE_HM_FUSE", "0")
    c0, d0, l0 = e.tsr_forward_decode(xd, wiz_rev=True, vis_thresh=0.2, sync=True)
    c0, d0, l0 = np.asarray(c0), d0.cpu().numpy(), l0.cpu().numpy()
    print("cells per table:", c0.tolist())
    assert np.array_equal(c0, c1) and c0.sum() > 0, (c0, c1)
    # a score is sigmoid(logit) (times 0.4 when the snap demotes it): |d sigmoid| <= 1/4 |d logit|
    sb = 0.25 * bound.max()
    worst = 0.0
    for b in range(len(c0)):          # rows beyond a table's count are unspecified
        k = int(c0[b])
        assert np.array_equal(d0[b, :k, :8].view(np.int32), d1[b, :k, :8].view(np.int32)), b      # the quads
        assert np.array_equal(l0[b, :k].view(np.int32), l1[b, :k].view(np.int32)), b              # the logical-location features
        if k:
            worst = max(worst, float(np.abs(d0[b, :k, 8].astype(np.float64) - d1[b, :k, 8].astype(np.float64)).max()))
    print(f"scores: max |fused - two| {worst:.3e}, bound {sb:.3e}")
    assert worst <= sb
