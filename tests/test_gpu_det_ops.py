"""The two operators of csrc/det_ops.hip -- pt_op_affine_act, pt_op_db_tail -- through the C ABI against a float64 reference that reads exactly
the stored input values, in the three storage modes (conventions, ``Mode`` helper and relative terms of tests/test_gpu_graph_ops.py: 2^-8 bf16, 2^-10
f16, 2^-14 bf16x3 with the normalisation and "hi alone fails" checks).

Absolute terms:
  affine_act   y = s2 act(s1 x + b1) + b2 in fp32 without contraction: the product and the sum in front of the activation (2 roundings of at most
               M1 = |s1 x| + |b1|), through an activation whose slope is at most 1.5 (hardswish at 3) -> 3 U M1; the activation's own three
               operations, each relative to a result of at most M1 -> 3 U M1; the second product and sum -> 2 U (|s2| M1 + |b2|):
               eps = 8 U (|s2| (|s1 x| + |b1|) + |b2|), derived, not measured.
  db_tail      logits: an fp32 sum of n + 1 terms, in any order and with fused multiply-adds, is within (n + 1) U of the sum of their magnitudes.  With A1 = |b1| + sum_c |W1 x| the
               hidden value is within (C + 1) U A1, and with S = max over the outputs of |b2| + sum_c1 |W2| A1 the logit is within
               (C + 1) U S + (C1 + 1) U S <= 4 (C + C1) U S (the bound the operator's description states); the sigmoid's slope is at most 1 / 4.
               The device exponential and division: not derivable.  MEASURED on gfx950 against float64 on the 384 exact logits in [-2.75, 3.22] of
               test_db_tail_structure (which prints it), the same in all three modes: worst |p - sigmoid64(logit)| = 7.2e-8 (the fp32 rounding of p
               alone is up to 3e-8); allowed EXP_ERR = 4 x that.  The three random shapes then measure 1.4e-7 at the most against 2.3e-5 .. 3.6e-4.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_graph_ops_conventions", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_graph_ops.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

engines, m = G.engines, G.m          # the module-scope engines (one per storage mode) and the per-mode fixture
DEV, U = G.DEV, G.U

EXP_ERR = 4 * 7.2e-8                 # see the module docstring


def _pad(x, cp):
    """logical [..., C] -> [..., cp] with zeros in the padding"""
    out = torch.zeros(x.shape[:-1] + (cp,), dtype=x.dtype)
    out[..., :x.shape[-1]] = x
    return out


def _act_ref(v, act):
    return v * (v + 3).clamp(0, 6) / 6 if act == 2 else (v.clamp(min=0) if act == 1 else v)


def _vec(v, C, cp, junk):
    """fp32 [cp]: v (a scalar or [C]) in the real channels, `junk` in the padding (the kernel must not let it through)"""
    out = torch.full((cp,), float(junk), dtype=torch.float32)
    out[:C] = torch.as_tensor(v, dtype=torch.float32)
    return out


AFFINE_CASES = ["per_channel", "pre_identity", "post_identity", "scalars"]


@pytest.mark.parametrize("case", AFFINE_CASES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("C", [24, 96])
def test_affine_act(m, C, act, case):
    """[2, 3, 5, C] with C = 24 (rows of 64) and 96 (rows of 128): 30 pixels x 8 or 16 groups, a partial workgroup; non-zero junk in the padded entries of
    all four vectors, and the padded output channels must be exactly zero (both halves)"""
    cp = (C + 63) // 64 * 64
    g = G._gen(C * 10 + act + 100 * AFFINE_CASES.index(case))
    x = torch.randn(2, 3, 5, C, generator=g, dtype=torch.float64) * 3
    x.view(-1)[:6] = torch.tensor([-3.0, 3.0, 0.0, -3.0 - 2.0 ** -7, 3.0 + 2.0 ** -7, 1e-3])        # the hardswish kinks (for s1 = 1, b1 = 0)
    rnd = lambda sc, off=0.0: off + sc * torch.randn(C, generator=g)                                 # noqa: E731
    s1, b1, s2, b2 = rnd(0.3, 1.0), rnd(0.5), rnd(0.3, -1.0), rnd(0.5)
    if case == "pre_identity":
        s1, b1 = torch.ones(C), torch.zeros(C)
    elif case == "post_identity":
        s2, b2 = torch.ones(C), torch.zeros(C)
    elif case == "scalars":
        s1, b1, s2, b2 = (v[:1].expand(C) for v in (s1, b1, s2, b2))
    vs = [_vec(v, C, cp, 7.0) for v in (s1, b1, s2, b2)]
    xd, xv = m.put(_pad(x, cp))
    out = m.eng.op_affine_act(xd, C, vs[0].to(DEV), vs[1].to(DEV), act, vs[2].to(DEV), vs[3].to(DEV), split=m.split)
    S1, B1, S2, B2 = (v[:C].double() for v in vs)
    xr = xv[..., :C]
    ref = _pad(S2 * _act_ref(S1 * xr + B1, act) + B2, cp)
    eps = _pad(8 * U * (S2.abs() * ((S1 * xr).abs() + B1.abs()) + B2.abs()), cp)
    m.check(out, ref, eps, f"affine_act C={C} act={act} {case}")
    hi, lo = m.halves(out)
    assert bool((hi[..., C:] == 0).all()) and (lo is None or bool((lo[..., C:] == 0).all())), "padded channels are not zero"


def test_affine_act_exact(m):
    """small integers everywhere: every product and sum is exact in every format, so the result must EQUAL the reference -- a vector read at the wrong
    channel, or s1 / s2 or b1 / b2 swapped, shows independently of any tolerance"""
    C, cp = 24, 64
    g = G._gen(5)
    x = torch.randint(-4, 5, (2, 3, 5, C), generator=g).double()
    s1, b1 = torch.randint(1, 4, (C,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (C,), generator=g)).float(), torch.randint(-5, 6, (C,), generator=g).float()
    s2, b2 = torch.randint(2, 5, (C,), generator=g).float(), torch.randint(-7, 8, (C,), generator=g).float()
    assert not torch.equal(s1, s2) and not torch.equal(b1, b2) and len(set(s1.tolist())) > 2
    xd, xv = m.put(_pad(x, cp))
    assert torch.equal(xv[..., :C], x)
    vs = [_vec(v, C, cp, 3.0) for v in (s1, b1, s2, b2)]
    out = m.eng.op_affine_act(xd, C, vs[0].to(DEV), vs[1].to(DEV), 1, vs[2].to(DEV), vs[3].to(DEV), split=m.split)
    torch.cuda.synchronize()
    ref = _pad(s2.double() * (s1.double() * x + b1.double()).clamp(min=0) + b2.double(), cp)
    assert 64 <= float(ref.abs().max()) <= 256             # integers every format stores exactly
    hi, lo = m.halves(out)
    got = hi if lo is None else hi + lo
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} exact outputs differ"


# ---- the DB head's tail ------------------------------------------------------------------------------------------------------------------------

def _tail_ref(xv, w1, b1, w2, b2):
    """float64: x [B, H, W, C] (the stored values) -> (probability [B, 4H, 4W], logit, S = the largest sum of absolute products of a logit)"""
    xn = G._nchw(xv)
    h = F.conv_transpose2d(xn, w1.double(), b1.double(), stride=2).clamp(min=0)
    logit = F.conv_transpose2d(h, w2.double(), b2.double(), stride=2)[:, 0]
    a1 = F.conv_transpose2d(xn.abs(), w1.double().abs(), b1.double().abs(), stride=2)
    S = float(F.conv_transpose2d(a1, w2.double().abs(), b2.double().abs(), stride=2).max())
    return torch.sigmoid(logit), logit, S


def _tiles(m, w):
    from pdf_table_amd.weights import split_bf16, tile_conv_weight, tile_conv_weight_x3
    t = tile_conv_weight_x3(w) if m.split else tile_conv_weight(w, "f16" if m.name == "f16" else "bf16")
    return torch.from_numpy(np.ascontiguousarray(t).view(np.int16)).to(DEV)


def _layered(m, xd, w1, b1, w2, b2):
    """the route without the fused kernel: two pixel-shuffle GEMMs (pt_op_conv2d, shuffle_cout), a stand-alone sigmoid, channel 0 -- packed as the
    executor's _convT packs them"""
    def convT(x, w, b, relu):
        ci, co = w.shape[:2]
        cip = x.shape[-1] // (2 if m.split else 1)
        wq = torch.zeros(2, 2, 64, cip)
        wq[:, :, :co, :ci] = w.permute(2, 3, 1, 0)
        bq = torch.zeros(64)
        bq[:co] = b
        return m.eng.op_conv2d(x, _tiles(m, wq.reshape(256, cip, 1, 1)), bq.repeat(4).to(DEV), 1, 1, relu=relu, shuffle_cout=64, split=int(m.split))
    y = m.eng.op_act(convT(convT(xd, w1, b1, 1), w2, b2, 0), 4, split=m.split)
    torch.cuda.synchronize()
    hi, lo = m.halves(y)
    return (hi if lo is None else hi + lo)[..., 0]


@pytest.mark.parametrize("shape", [(2, 5, 7, 24, 24), (1, 1, 1, 64, 64), (2, 3, 33, 8, 16)], ids=lambda s: "x".join(map(str, s)))
def test_db_tail(m, shape):
    """the shipped head's 24 -> 24 -> 1 on an odd map; one pixel with the widest channels (64 KB of LDS); a 33-wide map with 8 -> 16 (one channel group,
    rows that are no multiple of anything).  Against float64, and against the layered route on the same operands"""
    B, H, W, C, C1 = shape
    g = G._gen(sum(shape))
    xd, xv = m.put(_pad(torch.randn(B, H, W, C, generator=g, dtype=torch.float64), 64))
    w1 = torch.randn(C, C1, 2, 2, generator=g) * (1.0 / C) ** 0.5
    b1 = torch.randn(C1, generator=g) * 0.2
    w2 = torch.randn(C1, 1, 2, 2, generator=g) * (2.0 / C1) ** 0.5
    b2 = torch.randn(1, generator=g) * 0.2
    out = m.eng.op_db_tail(xd, C, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), split=m.split)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 4 * H, 4 * W, 1)
    got = out.cpu().double()[..., 0]
    ref, logit, S = _tail_ref(xv[..., :C], w1, b1, w2, b2)
    tol = 4 * (C + C1) * U * S / 4 + EXP_ERR
    err = float((got - ref).abs().max())
    print(f"db_tail {shape} [{m.name}]: max|dp| = {err:.3e} (tol {tol:.3e}; logit bound {4 * (C + C1) * U * S:.3e}, S = {S:.2f}, logits in "
          f"[{float(logit.min()):.2f}, {float(logit.max()):.2f}])")
    assert bool(torch.isfinite(got).all()) and err <= tol
    # the layered route rounds x W1 (16-bit weight tiles), the hidden map, the W2 tiles and the probability to the storage format: each a relative
    # perturbation of at most m.rel of terms whose magnitudes sum to at most S per logit (three of them, slope 1 / 4), and of p itself
    lay = _layered(m, xd, w1, b1, w2, b2)
    d = float((got - lay).abs().max())
    print(f"db_tail {shape} [{m.name}]: max|fused - layered| = {d:.3e} (allowed {m.rel * (1 + 3 * S / 4):.3e})")
    assert tuple(lay.shape) == tuple(got.shape) and d <= m.rel * (1 + 3 * S / 4) + tol


def test_db_tail_structure(m):
    """exact logits, a different one at every output position: input channel 0 is 1, channel 1 the pixel's number v = 1 .. 12 (over both images); W1 sends
    them to hidden units q and 4 + q at sub-position q = 2 dy + dx only; W2 gives unit q the weight (4 q + e) / 32 at e = 2 ey + ex and unit 4 + q
    the weight 1 / 2, a third pair of units is driven negative (ReLU must clear it): logit = (4 q + e) / 32 + v / 2 - 3.25, exact in fp32.  Swapped
    (dy, dx) / (ey, ex), a row of the other image or a missing ReLU move a logit by at least 1 / 32 -- at least 7e-4 in p, against a bound of 1e-6."""
    B, H, W, C, C1 = 2, 2, 3, 2, 12
    x = torch.zeros(B, H, W, C, dtype=torch.float64)
    x[..., 0] = 1.0
    x[..., 1] = torch.arange(1, B * H * W + 1, dtype=torch.float64).reshape(B, H, W)
    w1, w2 = torch.zeros(C, C1, 2, 2), torch.zeros(C1, 1, 2, 2)
    for q in range(4):
        dy, dx = q >> 1, q & 1
        w1[0, q, dy, dx] = 1.0
        w1[1, 4 + q, dy, dx] = 1.0
        w1[1, 8 + q, dy, dx] = -1.0                       # hidden unit 8 + q = -v < 0
        for e in range(4):
            w2[q, 0, e >> 1, e & 1] = (4 * q + e) / 32.0
            w2[4 + q, 0, e >> 1, e & 1] = 0.5
            w2[8 + q, 0, e >> 1, e & 1] = 1.0              # would subtract v if the ReLU were missing
    b1, b2 = torch.zeros(C1), torch.tensor([-3.25])
    xd, xv = m.put(_pad(x, 64))
    assert torch.equal(xv[..., :C], x)
    out = m.eng.op_db_tail(xd, C, w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), split=m.split)
    torch.cuda.synchronize()
    got = out.cpu().double()[..., 0]
    ref, logit, _ = _tail_ref(x, w1, b1, w2, b2)
    yy, xx = torch.meshgrid(torch.arange(4 * H), torch.arange(4 * W), indexing="ij")
    q, e = ((yy % 4) >> 1) * 2 + ((xx % 4) >> 1), (yy % 2) * 2 + (xx % 2)
    v = x[..., 1][:, yy // 4, xx // 4]
    assert torch.equal(logit, (4 * q + e).double() / 32 + v / 2 - 3.25) and logit.unique().numel() == logit.numel()
    err = float((got - ref).abs().max())
    print(f"db_tail structure [{m.name}]: exact logits in [{float(logit.min()):.3f}, {float(logit.max()):.3f}], device sigmoid max|dp| = {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(got.flatten().argsort(), logit.flatten().argsort())       # monotone: the same order as the exact logits


def test_db_tail_refuses_what_it_does_not_hold(engines):
    from pdf_table_amd import lib as L
    m = engines("bf16")
    x = torch.zeros(1, 2, 2, 128, dtype=m.dt, device=DEV)
    with pytest.raises(L.PtError, match="C=65"):
        m.eng.op_db_tail(x, 65, torch.zeros(65, 8, 2, 2, device=DEV), torch.zeros(8, device=DEV), torch.zeros(8, 1, 2, 2, device=DEV), torch.zeros(1, device=DEV))
    with pytest.raises(L.PtError, match="C1=65"):
        m.eng.op_db_tail(x, 8, torch.zeros(8, 65, 2, 2, device=DEV), torch.zeros(65, device=DEV), torch.zeros(65, 1, 2, 2, device=DEV), torch.zeros(1, device=DEV))
