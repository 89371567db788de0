"""The per-axis operators of csrc/rect_ops.hip (ABI 18) -- pt_op_conv2d_rect, pt_op_dwconv_rect, pt_op_pool_rect -- against a float64 reference that
reads exactly the stored input values, in the three storage modes (conventions, ``Mode`` helper and relative terms of tests/test_gpu_graph_ops.py:
2^-8 bf16, 2^-10 f16, 2^-14 bf16x3 with the normalisation and "hi alone fails" checks).

Absolute terms, derived, not measured:
  conv2d_rect   K = kh kw Cin products of magnitude <= S = max|x| max|w| summed in fp32 in some order: eps = 4 K 2^-24 S; the pair mode's three passes
                drop the lo x lo products, each lo at most 2^-9 of its hi: + K 2^-18 S.  The reference multiplies the tile values the kernel reads
                (w rounded to the storage format; w_hi + w_lo in the pair mode).
  dwconv_rect   as test_dwconv: 2 (k k + 1) 2^-24 max|w| max|x|
  pool_rect     max: bit for bit; average: (kh kw + 1) 2^-24 max|x|
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdf_table_amd import lib as L

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_graph_ops_conventions", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_graph_ops.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

engines, m = G.engines, G.m          # the module-scope engines (one per storage mode) and the per-mode fixture
DEV, U = G.DEV, G.U

GEOMS = [(3, 3, 2, 1), (3, 3, 1, 2), (1, 3, 1, 1), (3, 1, 1, 1), (1, 1, 2, 1), (1, 3, 1, 2), (3, 1, 2, 1), (3, 3, 1, 1), (3, 3, 2, 2)]
MAPS = [(1, 40), (3, 37), (6, 80), (7, 33)]
CHANS = [(32, 64), (96, 192)]


def _tiles(m, w):
    """fp32 [N, Cin, kh, kw] -> (device tiles in this mode's format, the float64 values those tiles hold)"""
    from pdf_table_amd.weights import split_bf16, tile_conv_weight, tile_conv_weight_x3
    if m.split:
        hi, lo = split_bf16(w)
        t, wv = tile_conv_weight_x3(w), hi.double() + lo.double()
    else:
        fmt = "f16" if m.name == "f16" else "bf16"
        t, wv = tile_conv_weight(w, fmt), w.to(m.dt).double()
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int16)).to(DEV), wv


def _act_ref(v, act):
    return v * (v + 3).clamp(0, 6) / 6 if act == 2 else (v.clamp(min=0) if act == 1 else v)


def _conv_ref(xv, wv, b, kh, kw, sh, sw, act):
    ref = F.conv2d(G._nchw(xv), wv, b.double(), (sh, sw), (kh // 2, kw // 2))
    return G._nhwc(_act_ref(ref, act))


def _conv_eps(m, K, xv, wv):
    S = float(xv.abs().max()) * float(wv.abs().max())
    return 4 * K * U * S + (K * 2.0 ** -18 * S if m.split else 0.0)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "k%dx%d_s%d%d" % g)
def test_conv2d_rect(m, geom):
    """every geometry on the one-row map, odd sizes under stride 2, widths that are no multiple of a tile; 32 -> 64 (one K chunk, one channel tile)
    and 96 -> 192 (three of each); B = 2; the activation rotates over the cases, so each appears in every geometry; the two square geometries are
    also compared with pt_op_conv2d on the same operands"""
    kh, kw, sh, sw = geom
    case = 0
    for (H, W) in MAPS:
        for (Cin, N) in CHANS:
            act = (GEOMS.index(geom) + case) % 3
            case += 1
            g = G._gen(H * 1000 + W * 10 + Cin + kh * 7 + kw * 3 + sh * 2 + sw)
            xd, xv = m.put(torch.randn(2, H, W, Cin, generator=g, dtype=torch.float64))
            w = torch.randn(N, Cin, kh, kw, generator=g) * (1.0 / (kh * kw * Cin) ** 0.5)
            b = torch.randn(N, generator=g) * 0.2
            wt, wv = _tiles(m, w)
            out = m.eng.op_conv2d_rect(xd, wt, b.to(DEV), kh, kw, sh, sw, act=act, split=int(m.split))
            ref = _conv_ref(xv, wv, b, kh, kw, sh, sw, act)
            eps = _conv_eps(m, kh * kw * Cin, xv, wv)
            what = f"conv2d_rect {geom} on {H}x{W}, {Cin}->{N}, act {act}"
            got = m.check(out, ref, eps, what)
            err = float(((got - ref).abs() / (m.rel * ref.abs() + eps)).max())
            print(f"{what} [{m.name}]: worst err / tol = {err:.3f}")
            if kh == kw and sh == sw:
                sq = m.eng.op_conv2d(xd, wt, b.to(DEV), kh, sh, relu=act, split=int(m.split))
                m.check(sq, ref, eps, what + " (pt_op_conv2d)")


def test_conv2d_rect_exact(m):
    """small-integer inputs and asymmetric small-integer weights: every product and partial sum is exact in every format, so the result must EQUAL
    the reference -- a swapped tap, a wrong pad or a row taken from the other image of the batch shows independently of any tolerance.  Geometry
    (3,3,2,1) on 7 x 33, B = 2; sparse inputs keep |sum| <= 256, the integers bf16 stores exactly (asserted on the reference)"""
    kh, kw, sh, sw, H, W, Cin, N = 3, 3, 2, 1, 7, 33, 32, 64
    g = G._gen(77)
    x = torch.randint(-3, 4, (2, H, W, Cin), generator=g).double() * (torch.rand(2, H, W, Cin, generator=g) < 0.2)
    w = torch.randint(-2, 3, (N, Cin, kh, kw), generator=g).float()
    assert not torch.equal(w, w.flip(2)) and not torch.equal(w, w.flip(3)) and not torch.equal(w, w.transpose(2, 3)) and not torch.equal(x[0], x[1])
    b = torch.randint(-4, 5, (N,), generator=g).float()
    xd, xv = m.put(x)
    wt, wv = _tiles(m, w)
    assert torch.equal(xv, x) and torch.equal(wv, w.double())
    ref = _conv_ref(xv, wv, b, kh, kw, sh, sw, 0)
    assert float(ref.abs().max()) <= 256 and float(ref.abs().max()) >= 16
    out = m.eng.op_conv2d_rect(xd, wt, b.to(DEV), kh, kw, sh, sw, split=int(m.split))
    torch.cuda.synchronize()
    hi, lo = m.halves(out)
    got = hi if lo is None else hi + lo
    assert got.shape == ref.shape
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} exact outputs differ"


def test_conv2d_rect_channel_slice(m):
    """out= a channel slice (out_coff > 0) of a wider sentinel-filled tensor: the slice holds the result, every other channel keeps the sentinel"""
    kh, kw, sh, sw, H, W, Cin, N, CW, coff = 1, 3, 1, 1, 3, 37, 32, 64, 192, 64
    g = G._gen(91)
    xd, xv = m.put(torch.randn(2, H, W, Cin, generator=g, dtype=torch.float64))
    w = torch.randn(N, Cin, kh, kw, generator=g) * 0.1
    b = torch.randn(N, generator=g) * 0.2
    wt, wv = _tiles(m, w)
    halves = 2 if m.split else 1
    out = torch.full((2, H, W, CW * halves), -77.5, dtype=m.dt, device=DEV)
    before = G._bits(out).clone()
    res = m.eng.op_conv2d_rect(xd, wt, b.to(DEV), kh, kw, sh, sw, act=1, out=out, out_coff=coff, split=int(m.split))
    assert res is out
    torch.cuda.synchronize()
    bits = G._bits(out)
    keep = torch.ones(CW * halves, dtype=torch.bool)
    for h0 in range(halves):
        keep[h0 * CW + coff:h0 * CW + coff + N] = False
    assert torch.equal(bits[..., keep], before[..., keep]), "channels outside the slice were written"
    sl = torch.cat([out[..., h0 * CW + coff:h0 * CW + coff + N] for h0 in range(halves)], -1).contiguous()
    m.check(sl, _conv_ref(xv, wv, b, kh, kw, sh, sw, 1), _conv_eps(m, kh * kw * Cin, xv, wv), "conv2d_rect into a channel slice")


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("sh,sw", [(2, 1), (1, 2)])
@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_rect(m, k, sh, sw, act):
    """maps smaller than the kernel (1 x 3), two rows, odd sizes; C = 8 (one channel group) and 40; B = 2"""
    for (H, W) in [(1, 3), (2, 34), (5, 9)]:
        for C in (8, 40):
            g = G._gen(H * 31 + W * 7 + C + k + sh * 2 + sw)
            xd, xv = m.put(torch.randn(2, H, W, C, generator=g, dtype=torch.float64))
            w = torch.randn(k * k, C, generator=g) * 0.3
            b = torch.randn(C, generator=g) * 0.1
            out = m.eng.op_dwconv_rect(xd, w.to(DEV), b.to(DEV), k, sh, sw, act, split=m.split)
            ref = F.conv2d(G._nchw(xv), w.t().double().reshape(C, 1, k, k), b.double(), (sh, sw), k // 2, groups=C)
            ref = G._nhwc(_act_ref(ref, act))
            eps = 2 * U * (k * k + 1) * float(w.abs().max()) * float(xv.abs().max())
            m.check(out, ref, eps, f"dwconv_rect k{k} s({sh},{sw}) on {H}x{W}x{C}")


def _windows(v, kh, kw):
    """[B, H, W, C] -> [B, H // kh, W // kw, C, kh kw], window elements in (dy, dx) order; trailing rows / columns dropped"""
    B, H, W, C = v.shape
    Ho, Wo = H // kh, W // kw
    return v[:, :Ho * kh, :Wo * kw].reshape(B, Ho, kh, Wo, kw, C).permute(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, C, kh * kw)


@pytest.mark.parametrize("sign", ["mixed", "negative"])
@pytest.mark.parametrize("kh,kw", [(2, 1), (1, 2), (3, 2), (2, 2), (4, 1)])
def test_pool_rect(m, kh, kw, sign):
    """3 x 11 (floor: a row / a column is dropped; the 4 x 1 window does not fit and the result is empty) and 8 x 6 (exact division except 4 x 1 ... 8 / 4);
    max bit for bit -- the winning (hi, lo) pair in the pair mode, an all-negative input catches a zero identity; average within its fp32 noise"""
    for (H, W) in [(3, 11), (8, 6)]:
        C = 24
        x = torch.randn(2, H, W, C, generator=G._gen(H * W + kh * 5 + kw), dtype=torch.float64) * 3
        if sign == "negative":
            x = -x.abs() - 0.5
        xd, xv = m.put(x)
        Ho, Wo = H // kh, W // kw
        win = _windows(xv, kh, kw)
        out = m.eng.op_pool_rect(xd, 0, kh, kw, split=m.split)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (2, Ho, Wo, C * (2 if m.split else 1))
        pick = torch.from_numpy(np.argmax(win.numpy(), axis=-1))[..., None]          # the first maximum in window order, as the kernel
        bits = G._bits(xd)
        halves = [bits[..., :C], bits[..., C:]] if m.split else [bits]
        want = torch.cat([_windows(hb, kh, kw).gather(-1, pick)[..., 0] for hb in halves], -1)
        assert torch.equal(G._bits(out), want), f"max {kh}x{kw} on {H}x{W}"
        if sign == "mixed":
            avg = m.eng.op_pool_rect(xd, 1, kh, kw, split=m.split)
            eps = (kh * kw + 1) * U * float(xv.abs().max())
            if avg.numel():
                m.check(avg, win.mean(-1), eps, f"average {kh}x{kw} on {H}x{W}")
            else:
                assert tuple(avg.shape) == tuple(out.shape)


def test_rejected_arguments(engines):
    """unsupported arguments come back as an error whose text names the argument and its value"""
    m = engines("bf16")
    e = m.eng
    x = torch.zeros(1, 4, 8, 32, dtype=m.dt, device=DEV)
    w = torch.zeros(64 * 32 * 25, dtype=torch.int16, device=DEV)
    b = torch.zeros(64, device=DEV)
    with pytest.raises(L.PtError, match="kh=5"):
        e.op_conv2d_rect(x, w, b, 5, 3, 1, 1)
    with pytest.raises(L.PtError, match="sh=3"):
        e.op_conv2d_rect(x, w, b, 3, 3, 3, 1)
    with pytest.raises(L.PtError, match="Cin=40"):
        e.op_conv2d_rect(torch.zeros(1, 4, 8, 40, dtype=m.dt, device=DEV), w, b, 3, 3, 2, 1)
    with pytest.raises(L.PtError, match="kh=5"):
        e.op_pool_rect(x, 0, 5, 1)
    with pytest.raises(L.PtError, match="kind=2"):
        e.op_pool_rect(x, 2, 2, 1)
    with pytest.raises(L.PtError, match="sw=3"):
        e.op_dwconv_rect(x, torch.zeros(9, 32, device=DEV), torch.zeros(32, device=DEV), 3, 1, 3)
