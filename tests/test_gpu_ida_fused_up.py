"""IDAUp's `up(proj) + node output` in the node DCN's epilogue (dcn_fused64_kernel's UPF, pt_op_dcn_up_add) and the DLA base that pools a level's
input once (dla_net.h): both must give the bits of the launches they replace.

Operator level: pt_op_dcn_up_add == pt_op_dcn followed by pt_op_dwconvt_up_add, bit for bit, in bf16 and f16, on multi-pixel offset fields; maps
with partial 8 x 16 tiles in both directions (every border of the low-resolution map then falls inside a tile), one exact tile, both up factors,
both channel widths.  Net level: the Lore detector with each switch off against the defaults, head maps and decoded cells."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.weights import tile_conv_weight

pytestmark = pytest.mark.gpu

HEADS = ("hm", "st", "wh", "ax", "cr", "reg")


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _operands(C, H, W, f, seed, dtype):
    from test_gpu_dcn_op import _om
    B, N = 2, C
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g).abs()
    w = torch.randn(N, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    off = (torch.rand(B, 18, H, W, generator=g) * 2.0 - 1.0) * 3.0          # offsets up to +-3 px: samples leave the map near every border
    mlog = torch.randn(B, 9, H, W, generator=g) * 2.0
    p = torch.randn(B, H // f, W // f, N, generator=g)                       # the next step's projection (signed here: both signs of every product)
    taps = torch.randn(4 * f * f, N, generator=g) * 0.3
    dev = torch.device("cuda", 0)
    w1 = w.to(dtype).float().permute(0, 2, 3, 1).reshape(N, 9 * C, 1, 1).contiguous()
    wt = torch.from_numpy(tile_conv_weight(w1, "f16" if dtype == torch.float16 else "bf16").view(np.int16)).to(dev)
    return x.to(dtype).to(dev), _om(off, mlog).to(dev), wt, b.to(dev), p.to(dtype).to(dev), taps.to(dev)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("C,H,W,f", [
    (64, 12, 20, 2),       # p' 6 x 10: partial tiles in both directions, every map border inside a tile
    (64, 12, 20, 4),       # p' 3 x 5
    (64, 8, 16, 2),        # p' 4 x 8: exactly one tile
    (128, 10, 18, 2),      # p' 5 x 9: the 128-wide block
])
def test_dcn_up_add_equals_the_two_launches(eng, fmt, C, H, W, f):
    eng.set_precision(L.PT_PRECISION_F16 if fmt == "f16" else L.PT_PRECISION_BF16)
    try:
        x, om, wt, b, p, taps = _operands(C, H, W, f, seed=C * 100 + H * 10 + f, dtype=eng.act_dtype)
        node = eng.op_dcn(x, om, wt, b, relu=True)
        two = eng.op_dwconvt_up_add(p, taps, node, f)
        one = eng.op_dcn_up_add(x, om, wt, b, p, taps, f, relu=True)
        torch.cuda.synchronize()
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    a, c = one.cpu().view(torch.int16), two.cpu().view(torch.int16)
    ndiff = int((a != c).sum())
    print(f"dcn + up [{fmt}] {C} @{H}x{W} f={f}: {ndiff} of {a.numel()} values differ; |sum| max {two.float().abs().max().item():.2f}")
    assert tuple(one.shape) == (2, H, W, C)
    assert bool((node.float() > 0).any()) and bool((two.float() != node.float()).any())
    assert ndiff == 0


def test_dcn_up_add_rejects_bad_arguments(eng):
    from pdf_table_amd.lib import PtError
    x, om, wt, b, p, taps = _operands(64, 12, 20, 2, seed=1, dtype=torch.bfloat16)
    dev = x.device
    with pytest.raises(PtError):         # 5 x 10 times 2 is not 12 x 20
        eng.op_dcn_up_add(x, om, wt, b, torch.zeros(2, 5, 10, 64, dtype=torch.bfloat16, device=dev), taps, 2)
    with pytest.raises(PtError):         # 6 x 10 times 4 is not 12 x 20
        eng.op_dcn_up_add(x, om, wt, b, p, torch.zeros(64, 64, device=dev), 4)
    with pytest.raises(PtError):         # factor 3
        eng.op_dcn_up_add(x, om, wt, b, torch.zeros(2, 4, 7, 64, dtype=torch.bfloat16, device=dev), taps, 3)
    with pytest.raises(PtError):         # the (hi | lo) layout keeps the two launches
        eng.op_dcn_up_add(torch.cat([x, x], -1).contiguous(), om, wt, b, p, taps, 2, split=1)
    assert eng.op_dcn_up_add(x, om, wt, b, p, taps, 2).shape == (2, 12, 20, 64)      # and the engine still runs


# ---- net level ------------------------------------------------------------------------------------------------------------------------------

SWITCHES = [{"PT_IDA_FUSE_UP": "0"}, {"PT_DLA_POOL_ONCE": "0"}, {"PT_IDA_FUSE_UP": "0", "PT_DLA_POOL_ONCE": "0"}]


@pytest.fixture(scope="module")
def lore_eng():
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_weights import lore_dla34_state_dict
    from pdf_table_amd.weights import pack_lore_dla34
    e = HipEngine(0)
    # head biases near the thresholds: cells and corners on noise input, so the decode has something to return
    e.load_weights(L.PT_MODEL_LORE_DLA34, pack_lore_dla34(lore_dla34_state_dict(seed=2, hm_bias=(-1.2, -0.6))))
    yield e
    e.close()


def _input(split):
    n, H, W = 3, 64, 96            # maps of 16 x 24, 8 x 12, 4 x 6 and 2 x 3
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, H, W, 3, generator=g) * 0.7
    x4 = torch.zeros(n, H, W, 8 if split else 4)
    hi = x.to(torch.bfloat16).float()
    x4[..., :3] = hi
    if split:
        x4[..., 4:7] = (x - hi).to(torch.bfloat16).float()
    return x4.to(torch.bfloat16).cuda()


def _heads(e, xd):
    out = {k: v.cpu().numpy().copy() for k, v in e.tsr_forward_net(xd).items()}
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def default_heads(lore_eng):
    return _heads(lore_eng, _input(False))


@pytest.mark.parametrize("env", SWITCHES, ids=["no_fused_up", "pool_twice", "neither"])
def test_net_head_maps_do_not_depend_on_the_switches(lore_eng, default_heads, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    off = _heads(lore_eng, _input(False))
    assert set(off) == set(HEADS) == set(default_heads)
    assert np.abs(default_heads["hm"]).max() > 0 and np.isfinite(default_heads["hm"]).all()
    for k in HEADS:
        assert np.array_equal(default_heads[k].view(np.int32), off[k].view(np.int32)), k


@pytest.mark.parametrize("env", SWITCHES, ids=["no_fused_up", "pool_twice", "neither"])
def test_net_decode_does_not_depend_on_the_switches(lore_eng, env, monkeypatch):
    xd = _input(False)
    c0, d0, l0 = lore_eng.tsr_forward_decode(xd, wiz_rev=True, vis_thresh=0.2, sync=True)
    c0, d0, l0 = np.asarray(c0).copy(), d0.cpu().numpy().copy(), l0.cpu().numpy().copy()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c1, d1, l1 = lore_eng.tsr_forward_decode(xd, wiz_rev=True, vis_thresh=0.2, sync=True)
    c1, d1, l1 = np.asarray(c1), d1.cpu().numpy(), l1.cpu().numpy()
    print("cells per table:", c0.tolist())
    assert np.array_equal(c0, c1) and c0.sum() > 0, (c0, c1)
    for b in range(len(c0)):          # rows beyond a table's count are unspecified
        k = int(c0[b])
        assert np.array_equal(d0[b, :k].view(np.int32), d1[b, :k].view(np.int32)), b
        assert np.array_equal(l0[b, :k].view(np.int32), l1[b, :k].view(np.int32)), b


def test_net_bf16x3_declines_the_fused_path(lore_eng, monkeypatch):
    """the (hi | lo) mode keeps the two launches (pt_dcn_fuses_up): with the switches on, its head maps are those of its own switch-off run"""
    lore_eng.set_precision(L.PT_PRECISION_BF16X3)
    try:
        xd = _input(True)
        on = _heads(lore_eng, xd)
        monkeypatch.setenv("PT_IDA_FUSE_UP", "0")
        monkeypatch.setenv("PT_DLA_POOL_ONCE", "0")
        off = _heads(lore_eng, xd)
    finally:
        lore_eng.set_precision(L.PT_PRECISION_BF16)
    assert np.isfinite(on["hm"]).all() and np.abs(on["hm"]).max() > 0
    for k in HEADS:
        assert np.array_equal(on[k].view(np.int32), off[k].view(np.int32)), k
