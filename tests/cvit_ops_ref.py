"""Plain float64 references of the ConvNextViT recogniser's kernels (csrc/cvit_model.hip), one operation each, with the error bounds the GPU tests
assert.  No GPU, no engine: tests/test_cvit_ops_host.py ties every function here to something independent (torch.nn.functional in float64, the
oracle's stitching and down-sampling), tests/test_gpu_cvit_ops.py compares the kernels with them.

Storage formats: "bf16" / "f16".  U[fmt] is the format's half-ulp relative to the value (one round-to-nearest store): 2^-8 for bf16 (8
significant bits), 2^-11 for f16 (11 bits)."""
import math
import os
import re

import numpy as np
import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
CV_T, LINE_T = 75, 201
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(x, fmt):
    """values -> float64 values of their round-to-nearest-even image in the storage format"""
    return x.to(DT[fmt]).double()


def split_pair(x):
    """float64 values -> (hi, lo) bf16 tensors of the pair modes: hi = bf16(x), lo = bf16(x - hi)"""
    hi = x.to(torch.bfloat16)
    lo = (x.double() - hi.double()).to(torch.bfloat16)
    return hi, lo


# ---- GELU ---------------------------------------------------------------------------------------------------------------------------------
def gelu_erf(x):
    """0.5 x (1 + erf(x / sqrt 2)) in float64"""
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_delta(x):
    """The contract of the fused MLP's GELU approximation against gelu_erf: an approximation error below a quarter of the bf16 half-ulp cannot be
    seen after the rounding that follows.  On [-4, 4]: relative 2^-11 where |GELU| >= 2^-6, absolute 2^-15 (the bf16 half-ulp at 2^-6) elsewhere;
    x > 4: relative 2^-11 (the clamp of Phi alone costs 1 - Phi(4) = 3.2e-5); x < -4: absolute 2^-12 (the clamp costs up to 4 Phi(-4) = 1.27e-4)."""
    x = x.double()
    g = gelu_erf(x).abs()
    inner = torch.where(g >= 2.0 ** -6, 2.0 ** -11 * g, torch.full_like(g, 2.0 ** -15))
    return torch.where(x > 4, 2.0 ** -11 * g, torch.where(x < -4, torch.full_like(g, 2.0 ** -12), inner))


def gelu_poly_coefficients():
    """the ten coefficients of gelu_pair as committed in csrc/cvit_model.hip"""
    with open(os.path.join(REPO, "pdf_table_amd", "csrc", "cvit_model.hip")) as f:
        src = f.read()
    body = re.search(r"gelu_pair\(mlp_f2 x\) \{.*?constexpr float A\[10\] = \{(.*?)\};", src, flags=re.S).group(1)
    a = [float(t.strip().rstrip("f")) for t in body.split(",")]
    assert len(a) == 10
    return a


def gelu_poly(x, dtype=torch.float64):
    """gelu_pair as written (clamps, Horner in t = x^2, the final product) evaluated in `dtype`; float32: every step rounded like the kernel's
    fused multiply-adds up to the double rounding of a product held in float64"""
    a = gelu_poly_coefficients()
    x = x.to(dtype)
    xp = torch.clamp(x, min=-4.0)
    xc = torch.clamp(xp, max=4.0)
    t = xc * xc
    q = torch.full_like(x, a[9])
    for k in range(8, -1, -1):
        q = (q.double() * t.double() + np.float32(a[k]).item()).to(dtype)
    return (xp.double() * (xc.double() * q.double() + 0.5).to(dtype).double()).to(dtype).double()


# ---- fused MLP ------------------------------------------------------------------------------------------------------------------------------
def mlp_ref(xb, w1, b1, w2, b2, x, fmt):
    """x + W2 GELU_erf(W1 xb + b1) + b2 in float64 on the given (already rounded) operands -> (ref, tol).
    tol[row, o] = sum_k |W2[o, k]| (u |h_k| + delta(pre_k)) + 2^-22 (|x| + sum_k |W2[o, k] h_k|) + 1e-6: the hidden value is stored in the 16-bit
    format once (u), its GELU may be off by the contract (delta), and the two products accumulate in fp32."""
    xb, w1, b1, w2, b2, x = (t.double() for t in (xb, w1, b1, w2, b2, x))
    pre = xb @ w1.t() + b1
    h = gelu_erf(pre)
    ref = x + h @ w2.t() + b2
    tol = (U[fmt] * h.abs() + gelu_delta(pre)) @ w2.abs().t() + 2.0 ** -22 * (x.abs() + h.abs() @ w2.abs().t()) + 1e-6
    return ref, tol, pre


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
def attention_ref(qkv):
    """qkv float64 [nchunks * 75, 576] = [q | k | v], 3 heads of 64, q already scaled -> (out [nchunks * 75, 192], sum_k p_k |v_k| of the same
    shape, scores [nchunks, 3, 75, 75]); every chunk attends to itself only"""
    n = qkv.shape[0] // CV_T
    t = qkv.double().reshape(n, CV_T, 3, 3, 64)                      # [chunk, token, part, head, d]
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))    # [chunk, head, token, d]
    s = q @ k.transpose(-1, -2)
    p = torch.softmax(s, dim=-1)
    out = (p @ v).permute(0, 2, 1, 3).reshape(n * CV_T, 192)
    pav = (p @ v.abs()).permute(0, 2, 1, 3).reshape(n * CV_T, 192)
    return out, pav, s


# ---- depthwise 7x7 + LayerNorm ---------------------------------------------------------------------------------------------------------------
def layernorm_parts(v, eps):
    """rows [.., C] float64 -> (centred values, rstd [.., 1], biased variance [.., 1])"""
    d = v - v.mean(-1, keepdim=True)
    q = (d * d).mean(-1, keepdim=True)
    return d, 1.0 / torch.sqrt(q + eps), q


def dwconv_ln_ref(x, w49, bias, g, beta, u_out):
    """x [B, H, W, C], w49 [49, C] (tap dy * 7 + dx), zero padding 3 -> (LayerNorm(conv + bias, eps 1e-6) * g + beta, tol), float64, by explicit
    shifted sums.  tol = |g| rstd 2 gamma_49 sum|w||x| + u_out |y| + 1e-6 with gamma_49 = 49 * 2^-24: the 49-term fp32 sum of a pixel and the
    same again for the fp32 statistics, carried through the normalisation, plus the store."""
    x, w49, bias, g, beta = (t.double() for t in (x, w49, bias, g, beta))
    B, H, W, C = x.shape
    xp = torch.zeros(B, H + 6, W + 6, C, dtype=torch.float64)
    xp[:, 3:3 + H, 3:3 + W] = x
    v = torch.zeros_like(x)
    mag = torch.zeros_like(x)
    for dy in range(7):
        for dx in range(7):
            win = xp[:, dy:dy + H, dx:dx + W]
            v += win * w49[dy * 7 + dx]
            mag += win.abs() * w49[dy * 7 + dx].abs()
    v = v + bias
    d, rstd, q = layernorm_parts(v, 1e-6)
    y = d * rstd * g + beta
    tol = g.abs() * rstd * 2 * 49 * 2.0 ** -24 * mag + u_out * y.abs() + 1e-6
    return y, tol, q


def ln_ref(x, g, beta, eps, u_out):
    """LayerNorm of float64 rows -> (y, tol).  tol = |g| rstd 2 gamma_16 (mean|x| + |x_c|) + u_out |y| + 1e-6, gamma_16 = 16 * 2^-24: the kernel's
    mean is a sum at most 14 additions deep (8 values in the lane, six butterfly steps) and a division, so it is off by at most gamma_16 mean|x|;
    the centred value adds one rounding of its own; the same again for the variance's effect; all of it is scaled by rstd |g| on the way out."""
    x, g, beta = x.double(), g.double(), beta.double()
    d, rstd, q = layernorm_parts(x, eps)
    y = d * rstd * g + beta
    tol = g.abs() * rstd * 2 * 16 * 2.0 ** -24 * (x.abs().mean(-1, keepdim=True) + x.abs()) + u_out * y.abs() + 1e-6
    return y, tol, q


# ---- index maps of cvit_ln_kernel ------------------------------------------------------------------------------------------------------------
def stitch_source_rows(nlines, cmap=None):
    """mode 2: for every output row (line, pos) of the 201-token lines, the input row chunk * 75 + token it is gathered from (modeling_vit.py:
    133-138: tokens 0..68 of chunk 0, 6..68 of chunk 1, 6..74 of chunk 2); cmap[3 line + j]: the compact chunk that holds chunk j of the line"""
    src = np.empty(nlines * LINE_T, np.int64)
    for line in range(nlines):
        for pos in range(LINE_T):
            j, t = (0, pos) if pos < 69 else ((1, pos - 63) if pos < 132 else (2, pos - 126))
            chunk = 3 * line + j if cmap is None else int(cmap[3 * line + j])
            src[line * LINE_T + pos] = chunk * CV_T + t
    return src


def pair_rows(x, B, H, W):
    """mode 1: rows (b, y, x) of [B, H, W] maps, C channels -> [B * H/2 * W, 2C]: rows 2y and 2y + 1 side by side (the K layout of the (2,1)-kernel,
    (2,1)-stride conv as a 1x1 GEMM over K = row * C + c)"""
    C = x.shape[-1]
    return x.reshape(B, H // 2, 2, W, C).permute(0, 1, 3, 2, 4).reshape(B * (H // 2) * W, 2 * C)


# ---- operand generators shared by the host and the GPU tests -----------------------------------------------------------------------------------
def mlp_case(C, rows, gain, fmt, seed):
    """operands of the fused MLP, already rounded to the storage format (float64 values): pre-activations of standard deviation `gain`
    (1.3: within about +-5; 4.1: to about +-18, a third beyond +-4), a per-unit b1, non-zero x and b2"""
    g = torch.Generator().manual_seed(seed)
    xb = rnd(torch.randn(rows, C, generator=g, dtype=torch.float64), fmt)
    w1 = rnd(torch.randn(4 * C, C, generator=g, dtype=torch.float64) * (gain / math.sqrt(C)), fmt)
    b1 = (torch.rand(4 * C, generator=g, dtype=torch.float64) * 2 - 1).float().double()
    w2 = rnd(torch.randn(C, 4 * C, generator=g, dtype=torch.float64) / math.sqrt(4 * C), fmt)
    b2 = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5).float().double()
    x = torch.randn(rows, C, generator=g, dtype=torch.float64).float().double()
    return xb, w1, b1, w2, b2, x


ATT_FAMILIES = ("normal", "peaked", "planted", "equal")


def attention_case(nchunks, family, seed):
    """float64 [nchunks * 75, 576] rows of [q | k | v] before rounding; the chunk under test is the middle one (chunk 0 when alone).
    normal: N(0,1)-ish scores.  peaked: one key per query scores 5 .. 12 above the rest, everything shifted by a common +-3.
    planted: the keys of the first two 32-key tiles lie along -u, those of the 11-key tail tile along +u; queries i % 3 == 0 look along +u with
    key 74 (the last valid key) on top, i % 3 == 1 along -u with key 0 on top, i % 3 == 2 along +u with a tail key (64 + i % 11) on top: for the
    +u queries the running maximum jumps by about 17 at the last tile.  equal: q = 0, every score equal, the output is the mean of v.
    With three chunks, chunks 0 and 2 hold keys that are the middle chunk's own queries scaled to a score of 25 and values of +-40: a kernel
    that read another chunk's keys would be dominated by them.  The three heads draw different data."""
    g = torch.Generator().manual_seed(seed)
    n, T = nchunks, CV_T
    t = torch.randn(n, T, 3, 3, 64, generator=g, dtype=torch.float64)          # [chunk, token, part, head, d]
    mid = n // 2
    q, k = t[mid, :, 0], t[mid, :, 1]                                            # [token, head, d] views
    u = torch.randn(3, 64, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    if family == "normal":
        q *= 0.125
    elif family == "peaked":
        tgt = torch.randint(0, T, (T, 3), generator=g)
        top = 5 + 7 * torch.rand(T, 3, generator=g, dtype=torch.float64)
        for h in range(3):
            kt = k[tgt[:, h], h]                                                 # [T, 64]
            q[:, h] = q[:, h] * 0.06 + kt * (top[:, h] / (kt * kt).sum(-1))[:, None]
            k[:, h] += 8 * u[h]
            q[:, h] += (3.0 / 8) * u[h] * torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0)[:, None]
    elif family == "planted":
        side = torch.where(torch.arange(T) < 64, -1.0, 1.0)[:, None]
        i = torch.arange(T)
        tgt = torch.where(i % 3 == 0, torch.full_like(i, 74), torch.where(i % 3 == 1, torch.zeros_like(i), 64 + i % 11))
        look = torch.where(i % 3 == 1, -1.0, 1.0)[:, None]
        for h in range(3):
            k[:, h] = 0.4 * k[:, h] + 4.0 * side * u[h]
            kt = k[tgt, h] - 4.0 * side[tgt] * u[h]                              # the planted key's own part, across u
            q[:, h] = q[:, h] * 0.05 + 2.2 * look * u[h] + kt * (6.0 / (kt * kt).sum(-1))[:, None]
    else:
        q.zero_()
    if n == 3:
        for c in (0, 2):
            t[c, :, 0] *= 0.05
            qq = t[mid, :, 0]
            nrm = (qq * qq).sum(-1, keepdim=True).clamp_min(1e-3)
            t[c, :, 1] = qq * (25.0 / nrm)
            t[c, :, 2] = 40.0 * torch.sign(t[c, :, 2])
    return t.reshape(n * T, 576)
