"""The 1x1 layers that now run on conv1x1_wide_kernel (row-limited launches, Cin % 64 != 0, the staged fp32-residual epilogue) give every output
bit of the chunk-per-stage kernel they replaced (PT_CONV1_WIDE=0, read at every call): same tiles, same chunk order inside the accumulators."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.weights import tile_conv_weight

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _layer(Cin, N, seed):
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda", 0)
    w = (torch.randn(N, Cin, 1, 1, generator=g) * (2.0 / Cin) ** 0.5).to(torch.bfloat16).float()
    wt = torch.from_numpy(tile_conv_weight(w).view(np.int16)).to(dev)
    bd = (torch.randn(N, generator=g) * 0.1).to(dev)
    return g, w, wt, bd


def _both(monkeypatch, fn):
    outs = []
    for sw in ("1", "0"):
        monkeypatch.setenv("PT_CONV1_WIDE", sw)
        o = fn()
        torch.cuda.synchronize()
        outs.append(o.cpu())
    monkeypatch.setenv("PT_CONV1_WIDE", "1")
    return outs


def _bits(t):
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)).numpy()


@pytest.mark.parametrize("case", [
    dict(rows=301, Cin=576, N=256, relu=1, lim=77),                           # Lore head .0: mosaic im2col, 9 two-chunk stages; limit inside a tile
    dict(rows=301, Cin=576, N=256, relu=1, lim=301),                          # limit = the whole map (every tile of every walk)
    dict(rows=2050, Cin=576, N=256, relu=1, lim=1203),                        # walks of more than one tile per workgroup
    dict(rows=301, Cin=256, N=64, out_f32=True, n_valid=8, lim=150),         # Lore head .2: fp32 out, 8 stored channels
    dict(rows=301, Cin=256, N=256, out_f32=True, lim=0),                      # nothing live
    dict(rows=97, Cin=96, N=64, relu=1, lim=61),                              # Cin % 64 != 0 and a row limit
])
def test_row_limited_wide_equals_chunk_kernel(eng, case, monkeypatch):
    rows, Cin, N = case["rows"], case["Cin"], case["N"]
    g, w, wt, bd = _layer(Cin, N, rows + Cin + N)
    x = torch.randn(1, rows, 32, Cin, generator=g).to(torch.bfloat16).cuda()
    lim = torch.tensor([case["lim"]], dtype=torch.int32).cuda()
    kw = dict(relu=case.get("relu", 0), out_f32=case.get("out_f32", False), n_valid=case.get("n_valid", 0), ylimit=lim)
    o1, o0 = _both(monkeypatch, lambda: eng.op_conv1x1_ex(x, wt, bd, **kw))
    assert np.array_equal(_bits(o1), _bits(o0))
    live = (case["lim"] + 3) // 4 * 4      # whole 4-row tiles below the limit are computed, the rest is not touched
    assert float(o1[:, live:].abs().max() if live < rows else 0.0) == 0.0
    if case["lim"] > 0:
        nv = case.get("n_valid", 0) or N
        ref = torch.einsum("bhwc,nc->bhwn", x[:, :live].float().cpu(), w[:, :, 0, 0]) + bd.cpu()
        if case.get("relu"):
            ref = ref.clamp_min(0)
        err = float((o1[:, :live].float() - ref[..., :nv]).abs().max())
        assert err <= 2e-2 * max(1.0, float(ref.abs().max())), err


@pytest.mark.parametrize("case", [
    dict(B=2, H=21, W=35, Cin=224, N=64, relu=True),                # three full stages and a padded one
    dict(B=1, H=7, W=70, Cin=96, N=128, res_mode=1),                # a full and a padded stage
    dict(B=3, H=9, W=13, Cin=160, N=64, relu=True),                 # two full stages and a padded one
    dict(B=1, H=26, W=38, Cin=96, N=256, res_mode=2),               # four output tiles, half-res residual
    dict(B=1, H=26, W=38, Cin=32, N=64),                            # one chunk: stays on the chunk kernel
])
def test_cin_not_multiple_of_64_wide_equals_chunk_kernel(eng, case, monkeypatch):
    B, H, W, Cin, N = case["B"], case["H"], case["W"], case["Cin"], case["N"]
    g, w, wt, bd = _layer(Cin, N, Cin * 3 + N)
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.bfloat16).cuda()
    rm = case.get("res_mode", 0)
    rd = None
    if rm == 1:
        rd = torch.randn(B, H, W, N, generator=g).to(torch.bfloat16).cuda()
    elif rm == 2:
        rd = torch.randn(B, H // 2, W // 2, N, generator=g).to(torch.bfloat16).cuda()
    o1, o0 = _both(monkeypatch, lambda: eng.op_conv2d(x, wt, bd, 1, 1, relu=case.get("relu", False), res=rd, res_mode=rm))
    assert np.array_equal(_bits(o1), _bits(o0))
    assert float(o1.float().abs().max()) > 0


@pytest.mark.parametrize("case", [
    dict(B=1, H=344, W=32, Cin=2048, N=256),        # the Lore processor's FFN down-projection + fp32 residual stream
    dict(B=1, H=344, W=32, Cin=256, N=256),         # attention output projection
    dict(B=2, H=9, W=45, Cin=96, N=128, relu=1),    # padded stage on the staged epilogue
])
def test_fp32_residual_staged_wide_equals_chunk_kernel(eng, case, monkeypatch):
    B, H, W, Cin, N = case["B"], case["H"], case["W"], case["Cin"], case["N"]
    g, w, wt, bd = _layer(Cin, N, Cin + 5 * N)
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.bfloat16).cuda()
    r = torch.randn(B, H, W, N, generator=g).cuda()
    o1, o0 = _both(monkeypatch, lambda: eng.op_conv1x1_ex(x, wt, bd, relu=case.get("relu", 0), out_f32=True, res_f32=r))
    assert np.array_equal(_bits(o1), _bits(o0))
    ref = torch.einsum("bhwc,nc->bhwn", x.float().cpu(), w[:, :, 0, 0]) + bd.cpu() + r.cpu()
    if case.get("relu"):
        ref = ref.clamp_min(0)
    assert float((o1 - ref).abs().max()) <= 1e-3 * max(1.0, float(ref.abs().max()))


def test_lore_sparse_heads_on_real_mosaics(monkeypatch):
    """pt_tsr_forward_decode (the ax / cr / wh / reg / st heads on patch mosaics, row-limited launches; the processor's fp32-residual GEMMs are
    not part of it): counts, boxes and logic features bit-identical between the wide and the chunk kernel"""
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_weights import lore_dla34_state_dict
    from pdf_table_amd.weights import pack_lore_dla34
    e = HipEngine(0)
    try:
        e.load_weights(L.PT_MODEL_LORE_DLA34, pack_lore_dla34(lore_dla34_state_dict(seed=2, hm_bias=(-1.2, -0.6))))
        g = torch.Generator().manual_seed(77)
        x = torch.randn(3, 256, 320, 3, generator=g) * 0.7
        x4 = torch.zeros(3, 256, 320, 4)
        x4[..., :3] = x.to(torch.bfloat16).float()
        xd = x4.to(torch.bfloat16).cuda()
        res = []
        for sw in ("1", "0"):
            monkeypatch.setenv("PT_CONV1_WIDE", sw)
            c, d, lg = e.tsr_forward_decode(xd, wiz_rev=True, vis_thresh=0.2, sync=True)
            res.append((np.asarray(c).copy(), d.cpu().numpy(), lg.cpu().numpy()))
        monkeypatch.setenv("PT_CONV1_WIDE", "1")
    finally:
        e.close()
    (c1, d1, l1), (c0, d0, l0) = res
    assert np.array_equal(c1, c0) and c1.sum() > 0, (c1, c0)
    for b in range(len(c1)):
        k = int(c1[b])
        assert np.array_equal(d1[b, :max(k, 1)], d0[b, :max(k, 1)])
        assert np.array_equal(l1[b, :k], l0[b, :k]), b
