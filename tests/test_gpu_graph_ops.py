"""Single-operator entry points of the generic ONNX executor (csrc/graph_ops.hip, and the launchers it shares with the dedicated networks:
depthwise conv, pooling, channel mean, add) against a float64 reference computed on the CPU, in the three storage modes the executor offers:
PT_PRECISION_BF16, PT_PRECISION_BF16X3 ((hi | lo) pairs) and PT_PRECISION_F16.

The reference reads exactly the values the kernel read: the bf16 / f16 rounded inputs, or hi + lo of a pair.  Tolerances follow the storage
format of the result, not its scale (one round-to-nearest store is half an ulp; the rest is room for the fp32 arithmetic):
  bf16     |err| <= 2^-8  |ref| + eps     (8 significant bits: a store is within 2^-9)
  f16      |err| <= 2^-10 |ref| + eps     (11 bits: 2^-11; eps also holds half the f16 subnormal spacing, 2^-25)
  bf16x3   |err| <= 2^-14 |ref| + eps     on hi + lo (a normalised pair carries at least 16 bits: 2^-17)
eps is stated per op: the fp32 summation noise of that op at the data's scale (a term count times 2^-24 times the magnitude of the terms).
Copies (maxpool, upsample, copy_channels) are compared bit for bit.  Every bf16x3 result is also checked to be normalised (|lo| <= ulp(hi) / 2)
and the case to be sensitive: the same comparison on hi alone fails, so a kernel that dropped or misplaced lo could not pass it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdf_table_amd import lib as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MODES = {"bf16": L.PT_PRECISION_BF16, "bf16x3": L.PT_PRECISION_BF16X3, "f16": L.PT_PRECISION_F16}
REL = {"bf16": 2.0 ** -8, "bf16x3": 2.0 ** -14, "f16": 2.0 ** -10}
EPS_FMT = {"bf16": 2.0 ** -126, "bf16x3": 2.0 ** -126, "f16": 2.0 ** -25}     # spacing of the format's smallest values
F16_MAX = 65504.0
U = 2.0 ** -24                                                                  # fp32 unit round-off


def _ulp_bf16(h):
    """ulp of bf16 values held as float64 (subnormal spacing 2^-133 below 2^-126, and for 0)"""
    e = torch.frexp(h)[1].double()                         # h = m 2^e, 0.5 <= |m| < 1: ulp = 2^(e - 8)
    return torch.where(h == 0, torch.full_like(h, 2.0 ** -133), torch.pow(2.0, torch.clamp(e, min=-125.0) - 8.0))


class Mode:
    """one engine in one storage mode: builds inputs, reads results, compares them with the float64 reference"""

    def __init__(self, name, eng):
        self.name, self.eng = name, eng
        self.split = name == "bf16x3"
        self.dt = torch.float16 if name == "f16" else torch.bfloat16
        self.rel = REL[name]

    def put(self, x):
        """logical values [..., C] (CPU) -> (device tensor in this mode's storage, [hi(C) | lo(C)] when split; float64 values it holds)"""
        x = x.double()
        hi = x.to(self.dt)
        if not self.split:
            return hi.to(DEV), hi.double()
        lo = (x - hi.double()).to(self.dt)
        return torch.cat([hi, lo], -1).contiguous().to(DEV), hi.double() + lo.double()

    def halves(self, t):
        """device result -> (hi, lo) as float64 CPU tensors (lo is None outside the pair mode)"""
        t = t.cpu()
        if not self.split:
            return t.double(), None
        c = t.shape[-1] // 2
        return t[..., :c].double(), t[..., c:].double()

    def check(self, out, ref, eps, what="", sensitive=True):
        """out: device result in this mode's storage; ref: float64 reference of the logical values; eps: the op's absolute term"""
        torch.cuda.synchronize()
        hi, lo = self.halves(out)
        got = hi if lo is None else hi + lo
        ref = ref.double()
        assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
        assert bool(torch.isfinite(got).all()), f"{what} [{self.name}]: Inf / NaN stored"
        tol = self.rel * ref.abs() + (eps + EPS_FMT[self.name])
        err = (got - ref).abs()
        bad = err > tol
        worst = int((err / tol).flatten().argmax())
        assert not bool(bad.any()), (f"{what} [{self.name}]: {int(bad.sum())} of {bad.numel()} values off; worst err {err.flatten()[worst].item():.3e} "
                                     f"at ref {ref.flatten()[worst].item():.6g} (tol {tol.flatten()[worst].item():.3e})")
        if lo is not None:
            assert bool((lo.abs() <= _ulp_bf16(hi) / 2).all()), f"{what}: (hi | lo) result not normalised"
            if sensitive:
                assert bool(((hi - ref).abs() > tol).any()), f"{what}: hi alone passes -- the case cannot tell a pair result from a bf16 one"
        return got

    def check_f32(self, out, ref, rel, eps, what=""):
        """an fp32 output (no storage rounding): relative fp32 noise of the op"""
        torch.cuda.synchronize()
        got = out.cpu().double()
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
        err = (got - ref).abs()
        tol = rel * ref.abs() + eps
        assert bool((err <= tol).all()), f"{what} [{self.name}]: worst err/tol {float((err / tol).max()):.3g}"


@pytest.fixture(scope="module")
def engines():
    """module-scope engines, one per storage mode, made on first use"""
    from pdf_table_amd.engine import HipEngine
    made = {}

    def get(name):
        if name not in made:
            e = HipEngine(0)
            e.set_precision(MODES[name])
            made[name] = Mode(name, e)
            assert made[name].dt == e.act_dtype and made[name].split == e.split
        return made[name]
    yield get
    for m in made.values():
        m.eng.close()


@pytest.fixture(params=list(MODES))
def m(request, engines):
    return engines(request.param)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


# ---- element-wise ------------------------------------------------------------------------------------------------------------------------------

def _act_ref(x, kind, alpha, beta):
    if kind == 1:
        return x.clamp(min=0)
    if kind == 2:
        return x * (x + 3).clamp(0, 6) / 6
    if kind == 4:
        return torch.sigmoid(x)
    if kind == 5:
        return (alpha * x + beta).clamp(0, 1)
    if kind == 6:
        return x.clamp(0, 6)
    if kind == 7:
        return x * 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
    return x * torch.sigmoid(x)


@pytest.mark.parametrize("kind", [1, 2, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("C", [24, 40])
def test_act(m, kind, C):
    """the kinks and tails: +-3 (hardswish), 0 and 6 (relu6), the hardsigmoid corners, |x| >= 20 (sigmoid / swish), each also a
    pair-width step off; 37 pixels: a partial last workgroup"""
    alpha, beta = (0.3, 0.4) if kind == 5 else (0.0, 0.0)         # ONNX HardSigmoid defaults are 0.2 / 0.5
    a32, b32 = float(np.float32(alpha)), float(np.float32(beta))  # the kernel's fp32 parameters
    kinks = torch.tensor([-3.0, 3.0, 0.0, 6.0, -6.0, 2.0, -4.0 / 3.0, 20.0, -20.0, 35.0, -35.0, 100.0, -100.0, 1.0, -1.0])
    kinks = torch.cat([kinks, kinks + 2.0 ** -11, kinks - 2.0 ** -11])
    npix = 37
    x = torch.randn(npix * C, generator=_gen(kind * 100 + C), dtype=torch.float64) * 4
    x[:kinks.numel()] = kinks
    xd, xv = m.put(x.reshape(npix, C))
    out = m.eng.op_act(xd, kind, alpha, beta, split=m.split)
    eps = 8 * U * (1 + xv.abs())                                  # one exp / erf and a few fp32 operations on x (GELU's 1 + erf cancels)
    m.check(out, _act_ref(xv, kind, a32, b32), eps, f"act {kind}")


def _pair_inputs(m, shape, seed):
    g = _gen(seed)
    return m.put(torch.randn(shape, generator=g, dtype=torch.float64) * 2), m.put(torch.randn(shape, generator=g, dtype=torch.float64) * 2)


@pytest.mark.parametrize("npix,C", [(37 * 29, 24), (1, 8), (523, 40), (300, 64)])
def test_mul_add(m, npix, C):
    """pixel counts that leave a partial last workgroup"""
    (ad, av), (bd, bv) = _pair_inputs(m, (npix, C), npix + C)
    m.check(m.eng.op_mul(ad, bd, split=m.split), av * bv, 4 * U, "mul")
    m.check(m.eng.op_add(ad, bd, split=m.split), av + bv, 4 * U * 8, "add")     # |a| + |b| <= 16: one rounding of an fp32 sum


def test_mul_grid_stride_beyond_block_cap(engines):
    """more than 65 536 x 256 x 8 values: mul_kernel's grid is capped at 65 536 workgroups of 256 threads (8 values each), so the
    grid-stride loop covers the rest.  A product of two bf16 values is exact in fp32 (8 + 8 significant bits), so the fp32 product
    rounded once to bf16 -- computed here by torch on the device to keep ~300 MB tensors off the CPU -- is the correctly rounded
    float64 product, and the kernel must match it bit for bit."""
    m = engines("bf16")
    C = 64
    npix = 65536 * 256 * 8 // C + 37
    g = torch.Generator(device=DEV).manual_seed(11)
    a = torch.randn(npix, C, generator=g, device=DEV).to(torch.bfloat16)
    b = torch.randn(npix, C, generator=g, device=DEV).to(torch.bfloat16)
    out = m.eng.op_mul(a, b)
    ref = (a.float() * b.float()).to(torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("B,HW,C", [(3, 1, 24), (3, 37, 40), (2, 50, 64)])
def test_scale_channels(m, B, HW, C):
    """x [B, HW, C] * gate [B, C]: a different gate per batch, a single pixel"""
    g = _gen(B * 1000 + HW + C)
    xd, xv = m.put(torch.randn(B, HW, 1, C, generator=g, dtype=torch.float64) * 3)
    gd, gv = m.put(torch.rand(B, 1, 1, C, generator=g, dtype=torch.float64) * 2 - 0.5)
    assert not torch.equal(gv[0], gv[1])
    m.check(m.eng.op_scale_channels(xd, gd, split=m.split), xv * gv, 4 * U, "scale_channels")


# ---- reductions ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,C", [(2, 1, 1, 8), (3, 37, 1, 24), (2, 1, 37, 40), (1, 96, 96, 1000), (2, 5, 7, 2048), (1, 64, 64, 8)])
def test_chan_mean(m, B, H, W, C):
    """HW of 1 and 37 (fewer pixels than PT_SE_CHUNKS = 64 chunks) and large maps; C = 8 (256 slots of one 8-channel group), 24 / 40 / 1000
    (group counts that do not divide 256: chan_partial_sum_kernel's slot math), 2048 (one slot); B > 1; deterministic: a second call
    gives the same bits"""
    g = _gen(B + H * 7 + W * 13 + C)
    xd, xv = m.put(torch.randn(B, H, W, C, generator=g, dtype=torch.float64) + 0.5)
    out = m.eng.op_chan_mean(xd, split=m.split)
    eps = U * (H * W / 64 + 320) * float(xv.abs().max())                     # per-slot run + slot sum (<= 256) + 64 chunks, fp32
    m.check(out, xv.mean(dim=(1, 2), keepdim=True), eps, "chan_mean")
    again = m.eng.op_chan_mean(xd, split=m.split)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(again)), "chan_mean is not deterministic"


@pytest.mark.parametrize("k", [2, 3, 4])
def test_avgpool(m, k):
    B, H, W, C = 2, 12, 24, 40
    xd, xv = m.put(torch.randn(B, H, W, C, generator=_gen(50 + k), dtype=torch.float64) * 2)
    ref = _nhwc(F.avg_pool2d(_nchw(xv), k))
    m.check(m.eng.op_avgpool(xd, k, split=m.split), ref, 2 * U * k * k * float(xv.abs().max()), f"avgpool {k}")


def _maxpool_ref_bits(m, xd, k, s, p):
    """the stored bits of the winning input (hi and lo of the winning PAIR) for every output"""
    hi, lo = m.halves(xd)
    v = hi if lo is None else hi + lo
    B, H, W, Cc = v.shape
    _, idx = F.max_pool2d(_nchw(v), k, s, p, return_indices=True)        # first maximum in window order on ties, as the kernels
    Ho, Wo = idx.shape[2:]
    idx = idx.reshape(B, Cc, -1)
    bits = _nchw(_bits(xd)).reshape(B, 2 * Cc if lo is not None else Cc, H * W)
    pick = lambda b: _nhwc(b.gather(2, idx).reshape(B, Cc, Ho, Wo))
    if lo is None:
        return pick(bits)
    return torch.cat([pick(bits[:, :Cc]), pick(bits[:, Cc:])], -1)


@pytest.mark.parametrize("sign", ["mixed", "negative"])
@pytest.mark.parametrize("B,H,W,C,k,s,p", [(2, 9, 13, 24, 3, 2, 1), (1, 8, 10, 40, 3, 2, 1), (3, 1, 1, 8, 3, 2, 1), (2, 8, 6, 24, 2, 2, 0),
                                           (1, 9, 6, 40, 3, 3, 0)])
def test_maxpool(m, sign, B, H, W, C, k, s, p):
    """MaxPool(3, 2, 1) on odd and even sizes and a 1 x 1 map, non-overlapping k x k for k = 2 and 3; all-negative inputs catch a zero
    identity; bit for bit, the pair mode copying the winning (hi, lo) pair"""
    x = torch.randn(B, H, W, C, generator=_gen(H * W + C + k), dtype=torch.float64) * 3
    if sign == "negative":
        x = -x.abs() - 0.5
    xd, _ = m.put(x)
    out = m.eng.op_maxpool(xd, k, s, p, split=m.split)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _maxpool_ref_bits(m, xd, k, s, p))


@pytest.mark.parametrize("f", [1, 2, 4])
def test_upsample(m, f):
    """nearest neighbour by 1, 2, 4, bit for bit; the pair mode moves the full [hi | lo] width as channels"""
    B, H, W, C = 2, 5, 3, 24
    xd, _ = m.put(torch.randn(B, H, W, C, generator=_gen(f), dtype=torch.float64))
    out = m.eng.op_upsample(xd, f)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(xd).repeat_interleave(f, 1).repeat_interleave(f, 2))


@pytest.mark.parametrize("scs,soff,dcs,doff,n", [(24, 3, 40, 5, 13), (17, 0, 32, 9, 17), (40, 11, 24, 1, 21), (8, 1, 64, 31, 7)])
def test_copy_channels(m, scs, soff, dcs, doff, n):
    """odd offsets, n not a multiple of 8; the destination is sentinel-filled: nothing outside [doff, doff + n) is written"""
    npix = 301
    src = torch.randn(npix, scs, generator=_gen(scs + dcs + n), dtype=torch.float64).to(m.dt).to(DEV)
    dst = torch.full((npix, dcs), -77.5, dtype=m.dt, device=DEV)
    ref = _bits(dst).clone()
    ref[:, doff:doff + n] = _bits(src)[:, soff:soff + n]
    m.eng.op_copy_channels(src, dst, n, soff, doff)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), ref)


# ---- sequence operators -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cp,c,offset", [(7, 24, 20, 0.0), (5, 8, 1, 0.0), (9, 200, 192, 0.0), (6, 96, 96, 256.0), (13, 72, 67, 0.0)])
def test_layernorm(m, rows, cp, c, offset):
    """c < c_pad (padded channels exact zeros), c = 1, c > 64, rows with a large common offset (mean >> std), row counts that are not a
    multiple of the 4 rows of a workgroup"""
    g = _gen(rows * 100 + c)
    x = torch.randn(rows, cp, generator=g, dtype=torch.float64) + offset
    x[:, c:] = 0.0
    xd, xv = m.put(x)
    gamma = (torch.rand(cp, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(cp, generator=g) * 0.5).to(DEV)
    eps = 1e-5
    out = m.eng.op_layernorm(xd, c, gamma, beta, eps, split=m.split)
    gv, bv = gamma.cpu().double(), beta.cpu().double()
    ref = torch.zeros(rows, cp, dtype=torch.float64)
    ref[:, :c] = F.layer_norm(xv[:, :c], (c,), gv[:c], bv[:c], float(np.float32(eps)))
    # fp32 noise: the mean's rounding (~(c / 64 + 6) U |mean|) and the fp32 rounding of x itself, both relative to the row's std
    mean, std = xv[:, :c].mean(1).abs(), xv[:, :c].std(1, unbiased=False)
    cond = float((mean / std.clamp(min=1e-3)).max()) if c > 1 else 0.0
    tol_eps = U * (c / 64 + 8) * (1 + cond) * 2 * float(gv.max())
    got = m.check(out, ref, tol_eps, "layernorm", sensitive=True)
    assert bool((got[:, c:] == 0).all()) and bool((_bits(out)[:, c:cp] == 0).all()), "padded channels are not exact zeros"


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("rows,cp,c,big", [(7, 24, 20, False), (5, 8, 1, False), (3, 6632, 6625, False), (6, 40, 37, True), (9, 64, 64, False)])
def test_softmax(m, f32, rows, cp, c, big):
    """fp32 and 16-bit outputs; c < c_pad (16-bit padding zeros); c = 1; a PP-OCR dictionary (6625); logits around +-1e4 (overflow-safe:
    the max is subtracted first); rows that leave a tail in the last workgroup"""
    g = _gen(rows * 10 + c)
    if big:
        # +-(1e4 + j / 8): exact in fp32 (17 bits) and as a pair, so the fp32 differences x - max are exact and the probabilities non-trivial
        x = (10000.0 + torch.randint(0, 64, (rows, cp), generator=g).double() / 8) * torch.where(torch.arange(rows)[:, None] % 2 == 0, 1.0, -1.0)
    else:
        x = torch.randn(rows, cp, generator=g, dtype=torch.float64) * 3
    x[:, c:] = -5.0                                               # padding the kernel must not read
    xd, xv = m.put(x)
    ref = torch.softmax(xv[:, :c], -1)
    out = m.eng.op_softmax(xd, c, f32=f32, split=m.split)
    noise = U * (c / 64 + 16)                                     # relative: the row sum (per-lane runs + wave tree), exp, one product
    if f32:
        m.check_f32(out, ref, noise, 2.0 ** -126, "softmax f32")
        return
    full = torch.zeros(rows, cp, dtype=torch.float64)
    full[:, :c] = ref
    m.check(out, full, noise * float(ref.max()), "softmax", sensitive=c > 1)    # c = 1: every probability is exactly 1 in any format
    assert bool((_bits(out)[:, c:cp] == 0).all()), "padded probabilities are not exact zeros"
    if m.split:
        assert bool((_bits(out)[:, cp + c:] == 0).all())


def _attn_ref(xv, heads, d, scale, out_c):
    """xv float64 [B, 1, T, >= 3 heads d] rows of [q | k | v] -> [B, 1, T, out_c]"""
    B, _, T, _ = xv.shape
    hd = heads * d
    part = lambda i: xv[:, 0, :, i * hd:(i + 1) * hd].reshape(B, T, heads, d).transpose(1, 2)
    q, k, v = part(0), part(1), part(2)
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, -1)
    out = torch.zeros(B, 1, T, out_c, dtype=torch.float64)
    out[:, 0, :, :hd] = (p @ v).transpose(1, 2).reshape(B, T, hd)
    return out, (q.abs() @ k.abs().transpose(-1, -2)).max() * abs(scale), v.abs().max()


def _attn_inputs(m, B, T, heads, d, qcs, seed):
    g = _gen(seed)
    x = torch.randn(B, 1, T, qcs, generator=g, dtype=torch.float64)
    x[..., 2 * heads * d:3 * heads * d] = x[..., 2 * heads * d:3 * heads * d] * 0.5 + 1.0      # values around 1: the output is not a small difference
    x[..., 3 * heads * d:] = 77.0                                                             # padding of a wider qkv_cstride: never read
    return m.put(x)


@pytest.mark.parametrize("B,T,heads,d,qcs,out_c,scale", [
    (1, 1, 1, 24, 72, 24, None), (2, 63, 8, 8, 192, 64, None), (1, 64, 1, 64, 192, 64, None), (3, 65, 2, 24, 160, 56, 0.3),
    (1, 1024, 2, 16, 96, 32, None), (2, 40, 8, 1, 32, 16, 1.7)])
def test_attention(m, B, T, heads, d, qcs, out_c, scale):
    """T = 1, 63, 64, 65 and the 1024 limit; d = 1, 8, 16, 24, 64; heads 1, 2, 8; a padded qkv_cstride; out_c > heads d (the extra channels
    stay zero); B = 3 and non-default scales"""
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    xd, xv = _attn_inputs(m, B, T, heads, d, qcs, B * 1000 + T + d)
    out = m.eng.op_attention(xd, heads, d, scale, out_c, split=m.split)
    ref, smax, vmax = _attn_ref(xv, heads, d, float(np.float32(scale)), out_c)
    # fp32 noise: the score dot products (d terms, |score| sums up to smax) move every weight by ~2 d smax U relative; the weighted sum
    # over T keys adds T U of max |v|
    eps = U * float(vmax) * (T + 2 * d * float(smax) + 16)
    m.check(out, ref, eps, "attention")
    hi, lo = m.halves(out)
    assert bool((hi[..., heads * d:] == 0).all()) and (lo is None or bool((lo[..., heads * d:] == 0).all())), "channels past heads * d written"


def test_attention_batch_invariant(m):
    """one sequence run alone gives the same bits as its slice of the B = 3 run"""
    B, T, heads, d, qcs, out_c = 3, 65, 2, 24, 160, 56
    xd, _ = _attn_inputs(m, B, T, heads, d, qcs, 4242)
    full = m.eng.op_attention(xd, heads, d, 0.3, out_c, split=m.split)
    one = m.eng.op_attention(xd[1:2].contiguous(), heads, d, 0.3, out_c, split=m.split)
    torch.cuda.synchronize()
    assert torch.equal(_bits(one), _bits(full)[1:2])


# ---- depthwise convolution (pt_launch_dwconv's three branches) ---------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,C,k,stride,act", [
    (2, 9, 20, 32, 3, 1, 1), (1, 7, 13, 64, 5, 1, 2),             # C % 32 == 0, stride 1: dwconv_tile_kernel
    (2, 11, 9, 24, 3, 1, 0), (1, 6, 10, 40, 5, 1, 2),             # stride 1, C % 32 != 0: dwconv2_kernel
    (2, 9, 13, 24, 3, 2, 1), (1, 10, 12, 64, 5, 2, 0), (1, 8, 8, 32, 3, 2, 2), (1, 7, 11, 40, 5, 2, 1),     # dwconv_kernel<k, 2>, odd / even
    (2, 1, 11, 24, 3, 1, 1), (1, 1, 6, 40, 5, 1, 0)])             # stride 1, Ho == 1, C % 32 != 0: dwconv_kernel<k, 1>
def test_dwconv(m, B, H, W, C, k, stride, act):
    g = _gen(H * 31 + W * 7 + C + k + stride)
    xd, xv = m.put(torch.randn(B, H, W, C, generator=g, dtype=torch.float64))
    w = torch.randn(k * k, C, generator=g) * 0.3
    b = torch.randn(C, generator=g) * 0.1
    out = m.eng.op_dwconv(xd, w.to(DEV), b.to(DEV), k, stride, act, split=m.split)
    ref = F.conv2d(_nchw(xv), w.t().double().reshape(C, 1, k, k), b.double(), stride, k // 2, groups=C)
    ref = _nhwc(ref * (ref + 3).clamp(0, 6) / 6 if act == 2 else (ref.clamp(min=0) if act == 1 else ref))
    eps = 2 * U * (k * k + 1) * float(w.abs().max()) * float(xv.abs().max())
    m.check(out, ref, eps, f"dwconv k{k} s{stride}")


# ---- the half format's range -------------------------------------------------------------------------------------------------------------------

def test_f16_saturating_stores(engines):
    """scale_channels and layernorm (large gamma) can produce values past 65 504: they are stored as +-65 504, never Inf; below the edge
    the usual comparison holds"""
    m = engines("f16")
    g = _gen(5)
    xd, xv = m.put((torch.rand(2, 6, 5, 16, generator=g, dtype=torch.float64) * 800 - 400))
    gd, gv = m.put(torch.rand(2, 1, 1, 16, generator=g, dtype=torch.float64) * 800 - 400)
    _check_saturated(m, m.eng.op_scale_channels(xd, gd), xv * gv, 4 * U, "scale_channels")
    rows, cp, c = 9, 24, 20
    x = torch.randn(rows, cp, generator=g, dtype=torch.float64)
    x[:, c:] = 0
    xd, xv = m.put(x)
    gamma = torch.full((cp,), 60000.0, device=DEV)
    beta = torch.zeros(cp, device=DEV)
    out = m.eng.op_layernorm(xd, c, gamma, beta, 1e-5)
    ref = torch.zeros(rows, cp, dtype=torch.float64)
    ref[:, :c] = F.layer_norm(xv[:, :c], (c,), None, None, float(np.float32(1e-5))) * 60000.0
    _check_saturated(m, out, ref, U * 64 * 60000.0, "layernorm")


def _check_saturated(m, out, ref, eps, what):
    big = ref.abs() > F16_MAX * (1 + 2.0 ** -10)
    assert bool(big.any()) and bool((ref.abs() < F16_MAX).any()), what
    got = m.check(out, ref.clamp(-F16_MAX, F16_MAX), eps, what)
    assert bool((got[big] == F16_MAX * ref[big].sign()).all()), f"{what}: a value past the edge is not stored as +-65504"


def test_f16_full_range_inputs(engines):
    """act, softmax, attention, avgpool and chan_mean cannot exceed their inputs' range: fed values at +-65 504 they return finite values
    that match the reference"""
    m = engines("f16")
    g = _gen(9)
    sgn = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0).double()
    xd, xv = m.put(sgn(2, 4, 6, 16) * F16_MAX)
    for kind in (1, 2, 4, 5, 6, 7, 8):
        m.check(m.eng.op_act(xd, kind, 0.2, 0.5), _act_ref(xv, kind, float(np.float32(0.2)), 0.5), 0.0, f"act {kind}")
    m.check(m.eng.op_avgpool(xd, 2), _nhwc(F.avg_pool2d(_nchw(xv), 2)), 0.0, "avgpool")
    m.check(m.eng.op_chan_mean(xd), xv.mean(dim=(1, 2), keepdim=True), U * 400 * F16_MAX, "chan_mean")
    # rows of +-65504 logits with ties at the maximum: exp(x - max) is 1 or 0
    xd2, xv2 = m.put(sgn(8, 24) * F16_MAX)
    m.check(m.eng.op_softmax(xd2, 24), torch.softmax(xv2, -1), 0.0, "softmax")
    m.check_f32(m.eng.op_softmax(xd2, 24, f32=True), torch.softmax(xv2, -1), 2.0 ** -20, 0.0, "softmax f32")
    # q, k, v at +-65504: scores ~ 1e10 in fp32, one-hot (or tied) weights, outputs averages of +-65504
    heads, d, T = 2, 4, 9
    qd, qv = m.put(sgn(2, 1, T, 3 * heads * d) * F16_MAX)
    ref, _, _ = _attn_ref(qv, heads, d, 0.5, heads * d)
    m.check(m.eng.op_attention(qd, heads, d, 0.5, heads * d), ref, 0.0, "attention")


# ---- rejected arguments --------------------------------------------------------------------------------------------------------------------------

def _p(t):
    return C.c_void_p(t.data_ptr())


def _refused(m, fn, args, outs, match):
    """a call the entry point must refuse: a non-zero status with pt_last_error() text naming the problem, and no output written"""
    keep = [_bits(o) if o.element_size() == 2 else o.cpu().clone() for o in outs]
    rc = getattr(m.eng.lib, fn)(m.eng._h, *args, m.eng._stream())
    torch.cuda.synchronize()
    with pytest.raises(L.PtError, match=match):
        L.check(rc, fn)
    for o, k in zip(outs, keep):
        assert torch.equal(_bits(o) if o.element_size() == 2 else o.cpu(), k), f"{fn} wrote its output although it refused the call"


def test_rejected_arguments(m):
    sp = int(m.split)
    w = 2 if m.split else 1                                       # a pair tensor is twice as wide

    def sent(*shape):
        return torch.full(shape, -3.5, dtype=m.dt, device=DEV)

    x, o = sent(1, 1, 1025, 3 * 8 * w), sent(1, 1, 1025, 8 * w)
    _refused(m, "pt_op_attention", [_p(x), 1, 1025, 1, 8, 24, 0.3, _p(o), 8, sp], [o], "pt_op_attention")          # T = 1025
    x, o = sent(1, 1, 4, 3 * 65 * w), sent(1, 1, 4, 65 * w)
    _refused(m, "pt_op_attention", [_p(x), 1, 4, 1, 65, 195, 0.3, _p(o), 65, sp], [o], "pt_op_attention")          # d = 65
    x, o, o32 = sent(6, 16 * w), sent(6, 16 * w), torch.full((6, 24), -3.5, device=DEV)
    _refused(m, "pt_op_softmax", [_p(x), 6, 16, 24, None, _p(o), sp], [o], "pt_op_softmax")                         # c > c_pad
    _refused(m, "pt_op_softmax", [_p(x), 6, 16, 24, _p(o32), None, sp], [o32], "pt_op_softmax")
    gamma = torch.ones(24, device=DEV)
    _refused(m, "pt_op_layernorm", [_p(x), 6, 16, 24, _p(gamma), _p(gamma), 1e-5, _p(o), sp], [o], "pt_op_layernorm")
    x, o = sent(1, 8, 8, 8 * w), sent(1, 8, 8, 8 * w)
    _refused(m, "pt_op_maxpool", [_p(x), 1, 8, 8, 8, 3, 1, 1, _p(o), sp], [o], "pt_op_maxpool")                     # k 3, stride 1
    x, o = sent(1, 7, 8, 8 * w), sent(1, 3, 4, 8 * w)
    _refused(m, "pt_op_avgpool", [_p(x), 1, 7, 8, 8, 2, _p(o), sp], [o], "pt_op_avgpool")                           # H % k != 0
    o = sent(1, 7, 8, 8 * w)
    _refused(m, "pt_op_act", [_p(x), 7 * 8 * 8, 3, 0.0, 0.0, _p(o), 8, sp], [o], "pt_op_act.*kind 3")
    x, o = sent(2, 4, 2056 * w), sent(2, 2056 * w)
    scratch = torch.full((m.eng.lib.pt_op_chan_mean_scratch_floats(2, 2056),), -3.5, device=DEV)
    _refused(m, "pt_op_chan_mean", [_p(x), 2, 4, 2056, _p(scratch), _p(o), sp], [o, scratch], "pt_op_chan_mean")    # C = 2056
    o = sent(2, 24 * w)
    _refused(m, "pt_op_chan_mean", [_p(x), 2, 0, 24, _p(scratch), _p(o), sp], [o, scratch], "pt_op_chan_mean")      # HW = 0: 0 / 0
    src, dst = sent(10, 24), sent(10, 16)
    _refused(m, "pt_op_copy_channels", [_p(src), 10, 24, 20, _p(dst), 16, 0, 8], [dst], "pt_op_copy_channels")       # 20 + 8 > 24
    _refused(m, "pt_op_copy_channels", [_p(src), 10, 24, 0, _p(dst), 16, 9, 8], [dst], "pt_op_copy_channels")        # 9 + 8 > 16
