"""pt_op_conv2d_large (csrc/large_conv.hip) -- dense stride-1 convolutions with a kernel side of 5, 7 or 9 -- against a float64 reference that reads
exactly the stored input values and the tile values the kernel reads, in the three storage modes (conventions, ``Mode`` helper and relative terms of
tests/test_gpu_graph_ops.py: 2^-8 bf16, 2^-10 f16, 2^-14 bf16x3 with the normalisation and "hi alone fails" checks).

Absolute term, derived as in tests/test_gpu_rect_ops.py, not measured: K = kh kw Cin products of magnitude <= S = max|x| max|w| summed in fp32 in some
order: eps = 4 K 2^-24 S; the pair mode's three passes drop the lo x lo products, each lo at most 2^-9 of its hi: + K 2^-18 S.

The residual route (a residual Add folded into such a convolution runs as the convolution, pt_op_add and the activation): the convolution's result is
rounded to the storage format before the sum, so the sum is compared with one more relative term on the convolution's reference, eps + rel max|conv|.
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

GEOMS = [(9, 9), (7, 7), (5, 5), (7, 1), (1, 7), (5, 1), (1, 5), (9, 3)]
MAPS = [(1, 40), (3, 4), (5, 33), (12, 37)]          # one row; smaller than every kernel; one column past a 32-column tile; two row blocks of 8
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


def _conv_ref(xv, wv, b, kh, kw, act):
    ref = F.conv2d(G._nchw(xv), wv, b.double(), 1, (kh // 2, kw // 2))
    return G._nhwc(_act_ref(ref, act))


def _conv_eps(m, K, xv, wv):
    S = float(xv.abs().max()) * float(wv.abs().max())
    return 4 * K * U * S + (K * 2.0 ** -18 * S if m.split else 0.0)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "k%dx%d" % g)
def test_conv2d_large(m, geom):
    """every geometry on the one-row map, on a map smaller than every kernel (padding on both sides of every tap row), one column past a column tile and
    on two row blocks; 32 -> 64 (one K chunk, one channel tile) and 96 -> 192 (three of each); B = 2, so a row taken from the other image shows; the
    activation rotates over the cases"""
    kh, kw = geom
    case = 0
    for (H, W) in MAPS:
        for (Cin, N) in CHANS:
            act = (GEOMS.index(geom) + case) % 3
            case += 1
            g = G._gen(H * 1000 + W * 10 + Cin + kh * 7 + kw * 3)
            xd, xv = m.put(torch.randn(2, H, W, Cin, generator=g, dtype=torch.float64))
            w = torch.randn(N, Cin, kh, kw, generator=g) * (1.0 / (kh * kw * Cin) ** 0.5)
            b = torch.randn(N, generator=g) * 0.2
            wt, wv = _tiles(m, w)
            out = m.eng.op_conv2d_large(xd, wt, b.to(DEV), kh, kw, act=act, split=int(m.split))
            ref = _conv_ref(xv, wv, b, kh, kw, act)
            eps = _conv_eps(m, kh * kw * Cin, xv, wv)
            what = f"conv2d_large {geom} on {H}x{W}, {Cin}->{N}, act {act}"
            # the helper's "hi alone fails" check of the pair mode can only hold where the tolerance is below the rounding of hi (up to 2^-9 |ref|):
            # at K = 81 x 96 the derived absolute term alone is above that, so the check is asked for where half of that rounding exceeds the tolerance
            R = float(ref.abs().max())
            got = m.check(out, ref, eps, what, sensitive=m.rel * R + eps < 2.0 ** -10 * R)
            err = float(((got - ref).abs() / (m.rel * ref.abs() + eps)).max())
            print(f"{what} [{m.name}]: worst err / tol = {err:.3f}")


def test_conv2d_large_exact(m):
    """small-integer inputs and asymmetric small-integer weights: every product and partial sum is exact in every format, so the result must EQUAL the
    reference -- a swapped tap, a wrong pad or a row taken from the other image of the batch shows independently of any tolerance.  9x9 on 5 x 33,
    32 -> 64, B = 2; sparse inputs and weights keep |sum| <= 256, the integers bf16 stores exactly (asserted on the reference)"""
    kh, kw, H, W, Cin, N = 9, 9, 5, 33, 32, 64
    g = G._gen(78)
    x = torch.randint(-3, 4, (2, H, W, Cin), generator=g).double() * (torch.rand(2, H, W, Cin, generator=g) < 0.1)
    w = torch.randint(-2, 3, (N, Cin, kh, kw), generator=g).float() * (torch.rand(N, Cin, kh, kw, generator=g) < 0.25)
    assert not torch.equal(w, w.flip(2)) and not torch.equal(w, w.flip(3)) and not torch.equal(w, w.transpose(2, 3)) and not torch.equal(x[0], x[1])
    b = torch.randint(-4, 5, (N,), generator=g).float()
    xd, xv = m.put(x)
    wt, wv = _tiles(m, w)
    assert torch.equal(xv, x) and torch.equal(wv, w.double())
    ref = _conv_ref(xv, wv, b, kh, kw, 0)
    assert float(ref.abs().max()) <= 256 and float(ref.abs().max()) >= 16
    out = m.eng.op_conv2d_large(xd, wt, b.to(DEV), kh, kw, split=int(m.split))
    torch.cuda.synchronize()
    hi, lo = m.halves(out)
    got = hi if lo is None else hi + lo
    assert got.shape == ref.shape
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} exact outputs differ"


def test_conv2d_large_channel_slice(m):
    """out= a channel slice (out_coff > 0) of a wider sentinel-filled tensor: the slice holds the result, every other channel keeps the sentinel"""
    kh, kw, H, W, Cin, N, CW, coff = 7, 5, 3, 37, 32, 64, 192, 64
    g = G._gen(92)
    xd, xv = m.put(torch.randn(2, H, W, Cin, generator=g, dtype=torch.float64))
    w = torch.randn(N, Cin, kh, kw, generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.2
    wt, wv = _tiles(m, w)
    halves = 2 if m.split else 1
    out = torch.full((2, H, W, CW * halves), -77.5, dtype=m.dt, device=DEV)
    before = G._bits(out).clone()
    res = m.eng.op_conv2d_large(xd, wt, b.to(DEV), kh, kw, act=1, out=out, out_coff=coff, split=int(m.split))
    assert res is out
    torch.cuda.synchronize()
    bits = G._bits(out)
    keep = torch.ones(CW * halves, dtype=torch.bool)
    for h0 in range(halves):
        keep[h0 * CW + coff:h0 * CW + coff + N] = False
    assert torch.equal(bits[..., keep], before[..., keep]), "channels outside the slice were written"
    sl = torch.cat([out[..., h0 * CW + coff:h0 * CW + coff + N] for h0 in range(halves)], -1).contiguous()
    m.check(sl, _conv_ref(xv, wv, b, kh, kw, 1), _conv_eps(m, kh * kw * Cin, xv, wv), "conv2d_large into a channel slice")


def test_conv2d_large_residual_route(m):
    """what the executor runs for a residual Add folded into a large convolution: the convolution without activation, pt_op_add with the residual,
    the activation behind the Add -- against the same float64 reference plus the residual"""
    kh, kw, H, W, Cin, N = 9, 9, 5, 33, 32, 64
    g = G._gen(93)
    xd, xv = m.put(torch.randn(2, H, W, Cin, generator=g, dtype=torch.float64))
    rd, rv = m.put(torch.randn(2, H, W, N, generator=g, dtype=torch.float64))
    w = torch.randn(N, Cin, kh, kw, generator=g) * (1.0 / (kh * kw * Cin) ** 0.5)
    b = torch.randn(N, generator=g) * 0.2
    wt, wv = _tiles(m, w)
    y = m.eng.op_conv2d_large(xd, wt, b.to(DEV), kh, kw, act=0, split=int(m.split))
    out = m.eng.op_act(m.eng.op_add(y, rd, split=m.split), 1, 0.0, 0.0, split=m.split)
    conv = _conv_ref(xv, wv, b, kh, kw, 0)
    eps = _conv_eps(m, kh * kw * Cin, xv, wv) + m.rel * float(conv.abs().max())
    m.check(out, (conv + rv).clamp(min=0), eps, "conv2d_large + add + ReLU", sensitive=False)


def test_rejected_arguments(engines):
    """unsupported arguments come back as an error whose text names the argument and its value"""
    m = engines("bf16")
    e = m.eng
    x = torch.zeros(1, 4, 8, 32, dtype=m.dt, device=DEV)
    w = torch.zeros(64 * 32 * 121, dtype=torch.int16, device=DEV)
    b = torch.zeros(64, device=DEV)
    with pytest.raises(L.PtError, match="kh=3 kw=3"):
        e.op_conv2d_large(x, w, b, 3, 3)
    with pytest.raises(L.PtError, match="kh=11"):
        e.op_conv2d_large(x, w, b, 11, 11)
    with pytest.raises(L.PtError, match="kw=4"):
        e.op_conv2d_large(x, w, b, 5, 4)
    with pytest.raises(L.PtError, match="Cin=40"):
        e.op_conv2d_large(torch.zeros(1, 4, 8, 40, dtype=m.dt, device=DEV), w, b, 5, 5)
    with pytest.raises(L.PtError, match="act=3"):
        e.op_conv2d_large(x, w, b, 5, 5, act=3)
