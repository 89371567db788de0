"""The ConvNextViT recogniser's kernels (csrc/cvit_model.hip) one at a time, through pt_op_cvit_mlp / attention / dwconv_ln / ln, against the
float64 references of tests/cvit_ops_ref.py (tied to torch and the oracle by tests/test_cvit_ops_host.py).  No model is loaded and no network runs.

Every operand is generated already rounded to the storage format, so the reference reads what the kernel reads; u is the format's half-ulp relative
to the value (2^-8 bf16, 2^-11 f16).  The bounds are stated with the references; every test prints its worst error / tolerance ratio."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvit_ops_ref as R  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd import weights as Wt  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MODES = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "bf16x3": L.PT_PRECISION_BF16X3}
SINGLE = ["bf16", "f16"]


class Mode:
    def __init__(self, name, eng):
        self.name, self.eng = name, eng
        self.split = name == "bf16x3"
        self.fmt = "f16" if name == "f16" else "bf16"
        self.dt = R.DT[self.fmt]
        self.u_out = 2.0 ** -15 if self.split else R.U[self.fmt]          # a normalised (hi | lo) pair carries 16 bits

    def put(self, v):
        """float64 values [.., C] -> (device tensor in this mode's storage ([hi C | lo C] when split), the float64 values it holds)"""
        if not self.split:
            t = v.to(self.dt)
            return t.to(DEV), t.double()
        hi, lo = R.split_pair(v)
        return torch.cat([hi, lo], -1).contiguous().to(DEV), hi.double() + lo.double()

    def get(self, t):
        t = t.cpu()
        assert bool(torch.isfinite(t.float()).all()), "Inf / NaN stored"
        if not self.split:
            return t.double()
        c = t.shape[-1] // 2
        return t[..., :c].double() + t[..., c:].double()


@pytest.fixture(scope="module")
def engines():
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


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a kernel fault poisons the process's context: end the session instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after a cvit op test, not continuing: {e}", returncode=3)


def _ratio(what, got, ref, tol):
    err = (got - ref).abs()
    r = err / tol
    i = int(r.flatten().argmax())
    worst = float(r.flatten()[i])
    print(f"{what}: worst err/tol {worst:.3f} (err {float(err.flatten()[i]):.3e} at ref {float(ref.flatten()[i]):.5g})")
    assert worst <= 1.0, f"{what}: {int((r > 1).sum())} of {r.numel()} values out of tolerance, worst err/tol {worst:.3f}"
    return worst


def _bits(a):
    """uint16 patterns -> a 2-byte device tensor"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def _f32(v):
    return v.float().contiguous().to(DEV)


# ---- fused MLP ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
@pytest.mark.parametrize("rows", [1, 37, 128, 200])
@pytest.mark.parametrize("Cc", [96, 192, 256])
def test_mlp_against_fp64(engines, Cc, rows, name):
    """rows: a partial wave; dead waves; exactly one workgroup; a second, ragged one.  Gain 1.3: pre-activations within about +-5; 4.1: to about
    +-18 with a third beyond the +-4 clamp of the polynomial GELU.  The residual stream is updated in place and only in its first `rows` rows."""
    m = engines(name)
    for gain in (1.3, 4.1):
        xb, w1, b1, w2, b2, x = R.mlp_case(Cc, rows, gain, m.fmt, 1000 * Cc + 10 * rows + int(gain))
        ref, tol, _ = R.mlp_ref(xb, w1, b1, w2, b2, x, m.fmt)
        w1b, w2pb = Wt.pack_cvit_mlp(w1.float(), w2.float(), m.fmt)
        xd = torch.full((rows + 5, Cc), 7.5, dtype=torch.float32, device=DEV)       # a sentinel tail past the last row
        xd[:rows] = _f32(x)
        ret = m.eng.op_cvit_mlp(xb.to(m.dt).to(DEV), _bits(w1b), _f32(b1), _bits(w2pb), _f32(b2), xd, rows=rows)
        torch.cuda.synchronize()
        assert ret.data_ptr() == xd.data_ptr()
        out = xd.cpu().double()
        assert bool((out[rows:] == 7.5).all()), "rows past `rows` were written"
        assert bool(((out[:rows] - x).abs() > 0).any()), "the stream was not updated in place"
        _ratio(f"cvit mlp C={Cc} rows={rows} gain={gain} [{name}]", out[:rows], ref, tol)


@pytest.mark.parametrize("name", SINGLE)
@pytest.mark.parametrize("Cc", [96, 192, 256])
def test_gelu_probe(engines, Cc, name):
    """The kernel's GELU read directly: W1 routes channel k mod C to hidden unit k with weight 1, W2 routes hidden unit L C + o to output o in launch
    L (four launches: every hidden chunk and every slot of the W2 permutation carries a value once), b2 = 0, x = 0 -- the output is the stored
    GELU(xb + b1) itself.  Pre-activations sweep [-12, 12], dense near +-4 (the clamps), 0 and -0.75 (the minimum).  Asserted:
    |got - GELU_erf64| <= u |GELU| + delta(x), delta = the contract of cvit_ops_ref.gelu_delta."""
    m = engines(name)
    rows = 128
    g = torch.Generator().manual_seed(Cc)
    n = rows * Cc
    parts = [(0.40, -12.0, 12.0), (0.10, -4.0, 4.0), (0.10, 3.7, 4.3), (0.10, -4.3, -3.7), (0.15, -0.1, 0.1), (0.15, -0.95, -0.55)]
    pts = torch.cat([lo + (hi - lo) * torch.rand(int(round(f * n)), generator=g, dtype=torch.float64) for f, lo, hi in parts])
    assert pts.numel() == n
    xb = R.rnd(pts[torch.randperm(n, generator=g)].reshape(rows, Cc), m.fmt)
    xb[0, :4] = torch.tensor([4.0, -4.0, 0.0, -0.75], dtype=torch.float64)
    w1 = torch.zeros(4 * Cc, Cc, dtype=torch.float64)
    w1[torch.arange(4 * Cc), torch.arange(4 * Cc) % Cc] = 1.0
    w1b = Wt.to_bf16_bits(w1.float(), m.fmt)
    b1 = ((torch.rand(4 * Cc, generator=g, dtype=torch.float64) * 2 - 1) * 2.0 ** -7).float()
    b1[:4] = 0
    zeros_c = torch.zeros(Cc, dtype=torch.float32, device=DEV)
    stats = {"abs_in": 0.0, "rel_in": 0.0, "abs_neg": 0.0, "rel_pos": 0.0}
    worst = 0.0
    for launch in range(4):
        w2 = torch.zeros(Cc, 4 * Cc, dtype=torch.float64)
        w2[torch.arange(Cc), launch * Cc + torch.arange(Cc)] = 1.0
        _, w2pb = Wt.pack_cvit_mlp(w1.float(), w2.float(), m.fmt)
        xd = torch.zeros((rows, Cc), dtype=torch.float32, device=DEV)
        m.eng.op_cvit_mlp(xb.to(m.dt).to(DEV), _bits(w1b), b1.to(DEV), _bits(w2pb), zeros_c, xd)
        torch.cuda.synchronize()
        got = xd.cpu()
        assert torch.equal(got, got.to(m.dt).float()), "the output is one stored hidden value: exactly representable in the storage format"
        pre = (xb.float() + b1[launch * Cc:(launch + 1) * Cc][None, :]).double()          # the kernel's one fp32 addition
        ref = R.gelu_erf(pre)
        err = (got.double() - ref).abs()
        tol = R.U[m.fmt] * ref.abs() + R.gelu_delta(pre)
        worst = max(worst, float((err / tol).max()))
        inside, big = pre.abs() <= 4, ref.abs() >= 2.0 ** -6
        stats["abs_in"] = max(stats["abs_in"], float(err[inside].max()))
        stats["rel_in"] = max(stats["rel_in"], float((err / ref.abs())[inside & big].max()))
        stats["abs_neg"] = max(stats["abs_neg"], float(err[pre < -4].max()))
        stats["rel_pos"] = max(stats["rel_pos"], float((err / ref.abs())[pre > 4].max()))
    print(f"cvit gelu probe C={Cc} [{name}]: worst err/tol {worst:.3f}; stored GELU against erf in fp64: max abs err on [-4, 4] {stats['abs_in']:.3e}, "
          f"max rel err where |GELU| >= 2^-6 {stats['rel_in']:.3e}, max abs err for x < -4 {stats['abs_neg']:.3e}, max rel err for x > 4 {stats['rel_pos']:.3e}")
    assert worst <= 1.0


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("family", R.ATT_FAMILIES)
@pytest.mark.parametrize("nchunks", [1, 3])
def test_attention_against_fp64(engines, nchunks, family, name):
    """Families as described with cvit_ops_ref.attention_case.  Single pass: |got - ref| <= u |ref| + u sum_k p_k |v_k| + 1e-6 (the output's store, and
    the probabilities' store into the second product's operand while the normaliser sums them unrounded).  BF16X3: the project's contract,
    1e-3 max(1, max|ref|), on exact (hi, lo) operands with |score| <= 20."""
    m = engines(name)
    dev, qkv = m.put(R.attention_case(nchunks, family, 100 * nchunks + R.ATT_FAMILIES.index(family)))
    ref, pav, s = R.attention_ref(qkv)
    assert float(s.abs().max()) <= 20.0
    got = m.get(m.eng.op_cvit_attention(dev, split=m.split))
    torch.cuda.synchronize()
    if m.split:
        tol = torch.full_like(ref, 1e-3 * max(1.0, float(ref.abs().max())))
    else:
        tol = R.U[m.fmt] * ref.abs() + R.U[m.fmt] * pav + 1e-6
    _ratio(f"cvit attention nchunks={nchunks} {family} [{name}]", got, ref, tol)
    if family == "equal":
        mid = slice(75 * (nchunks // 2), 75 * (nchunks // 2) + 75)
        mean_v = qkv[mid, 384:].mean(0, keepdim=True)
        assert bool(((got[mid] - mean_v).abs() <= tol[mid]).all()), "equal scores: the output is the mean of v"


# ---- depthwise 7x7 + LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _dw_case(H, Cc, W, shared, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, H, W, Cc, generator=g)
    if shared:
        # near-zero variance: image 0 is constant across the channels and every channel has the same taps and bias, so the convolution's output is
        # constant across the channels too (exactly, in exact arithmetic)
        x[0] = x[0, :, :, :1].clone()
        w49 = (torch.randn(49, 1, generator=g) * 0.15).expand(49, Cc).contiguous()
        bias = torch.full((Cc,), 0.25)
    else:
        x[0, :, W // 2:W // 2 + 3] += 100.0                                        # a common offset on all channels of some pixels
        x[1, :, W // 3] = x[1, :, W // 3, :1].clone()                                    # pixels constant across the channels
        w49 = torch.randn(49, Cc, generator=g) * 0.15
        bias = torch.randn(Cc, generator=g) * 0.1
    ga = 1 + 0.3 * torch.randn(Cc, generator=g)
    be = 0.5 * torch.randn(Cc, generator=g)
    return x, w49, bias, ga, be


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("H,Cc,W,shared", [(8, 96, 75, False), (4, 192, 75, False), (2, 256, 75, False), (1, 512, 75, False), (8, 96, 5, False),
                                           (8, 96, 8, False), (8, 96, 75, True)])
def test_dwconv_ln_against_fp64(engines, H, Cc, W, shared, name):
    """W = 75: nine full 8-column tiles and one of three columns; 5 and 8: less than / exactly one tile.  Every row is within three rows of a border
    (vertical padding) and the first / last three columns see the horizontal one; C = 96 runs 128 threads (one wave partly past C).  Two images
    with different data.  Bound: cvit_ops_ref.dwconv_ln_ref."""
    m = engines(name)
    x, w49, bias, ga, be = _dw_case(H, Cc, W, shared, 7 * H + Cc + W)
    ref, tol, q = R.dwconv_ln_ref(x, w49, bias, ga, be, m.u_out)
    if shared:
        assert float(q[0].max()) < 1e-20 and float(q[1].min()) > 1e-3              # image 0: nothing but rounding noise to normalise
    got = m.get(m.eng.op_cvit_dwconv_ln(x.to(DEV), w49.to(DEV), bias.to(DEV), ga.to(DEV), be.to(DEV), split=m.split))
    torch.cuda.synchronize()
    _ratio(f"cvit dwconv7+ln H={H} C={Cc} W={W}{' shared taps' if shared else ''} [{name}]", got, ref, tol)


# ---- the LayerNorm kernel: indexing bit for bit -----------------------------------------------------------------------------------------------------
def _coded_rows(rows, Cc):
    """fp32 rows whose every value is an integer below 251 (exact in bf16 and f16) that encodes the row: channels 0..2 hold its base-128 digits, the
    others a hash of (row, channel)"""
    r, c = torch.meshgrid(torch.arange(rows), torch.arange(Cc), indexing="ij")
    x = (r * 31 + c * 17) % 251
    for d in range(3):
        x[:, d] = (torch.arange(rows) >> (7 * d)) & 127
    return x.float()


def _expect_bits(m, v):
    """the device image of exactly representable values: the values, and zeros in the lo half"""
    t = v.to(m.dt)
    return torch.cat([t, torch.zeros_like(t)], -1) if m.split else t


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("Cc", [96, 192, 256, 512])
def test_ln_mode0_rows_bit_exact(engines, Cc, name):
    m = engines(name)
    rows, w = 203, Cc * (2 if m.split else 1)                                       # not a multiple of the four rows of a workgroup
    x = _coded_rows(rows, Cc)
    out = torch.full((rows + 3, w), -3.5, dtype=m.dt, device=DEV)
    m.eng.op_cvit_ln(x.to(DEV), out, rows, None, None, 0.0, mode=0, split=m.split)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:rows], _expect_bits(m, x)) and bool((got[rows:] == -3.5).all())


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("H,Cc", [(8, 96), (4, 192), (2, 256)])
def test_ln_mode1_pairs_rows_bit_exact(engines, H, Cc, name):
    """every output row (b, y / 2, x) holds its two source rows (b, 2y', x) and (b, 2y' + 1, x) at channel offsets 0 and C"""
    m = engines(name)
    B, W = 2, 75
    rows = B * H * W
    x = _coded_rows(rows, Cc)
    out = torch.full((rows // 2, 2 * Cc * (2 if m.split else 1)), -3.5, dtype=m.dt, device=DEV)
    m.eng.op_cvit_ln(x.to(DEV), out, rows, None, None, 0.0, mode=1, H=H, W=W, split=m.split)
    torch.cuda.synchronize()
    want = R.pair_rows(x, B, H, W)
    assert torch.equal(out.cpu(), _expect_bits(m, want))
    first = want[W + 3]                                                             # b = 0, y' = 1, x = 3: rows (2, 3) and (3, 3) of image 0
    assert torch.equal(first[:Cc], x[(2 * W) + 3]) and torch.equal(first[Cc:], x[(3 * W) + 3])


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("shared", [False, True])
def test_ln_mode2_stitches_lines_bit_exact(engines, shared, name):
    """two lines from their own six chunks; three lines through a chunk map in which several line-chunks share one compact chunk.  All 201
    positions of every line, the 68 | 69 and 131 | 132 borders by name."""
    m = engines(name)
    Cc = 192
    if shared:
        nlines, cmap, nchunks = 3, np.array([0, 1, 4, 2, 4, 4, 3, 4, 4], np.int32), 5
    else:
        nlines, cmap, nchunks = 2, None, 6
    x = _coded_rows(nchunks * 75, Cc)
    rows = nlines * 201
    out = torch.full((rows + 2, Cc * (2 if m.split else 1)), -3.5, dtype=m.dt, device=DEV)
    m.eng.op_cvit_ln(x.to(DEV), out, rows, None, None, 0.0, mode=2, cmap=None if cmap is None else torch.from_numpy(cmap).to(DEV), split=m.split)
    torch.cuda.synchronize()
    src = R.stitch_source_rows(nlines, cmap)
    got = out.cpu()
    assert torch.equal(got[:rows], _expect_bits(m, x[torch.from_numpy(src)])) and bool((got[rows:] == -3.5).all())
    half = got[:rows, :Cc].float()
    for line in range(nlines):
        ch = [3 * line + j if cmap is None else int(cmap[3 * line + j]) for j in range(3)]
        for pos, (j, t) in {0: (0, 0), 68: (0, 68), 69: (1, 6), 131: (1, 68), 132: (2, 6), 200: (2, 74)}.items():
            assert torch.equal(half[line * 201 + pos], x[ch[j] * 75 + t]), (line, pos)


# ---- the LayerNorm kernel: numerics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("eps", [1e-6, 1e-12])
@pytest.mark.parametrize("Cc", [96, 192, 256, 512])
def test_ln_numerics_against_fp64(engines, Cc, eps, name):
    """modes 0 and (C = 192, the ViT's width) 2 with real gamma / beta: ordinary rows, rows with a common offset of +256, a nearly constant row.
    Bound: cvit_ops_ref.ln_ref."""
    m = engines(name)
    g = torch.Generator().manual_seed(Cc)
    rows = 6 * 75 - 1 if Cc != 192 else 6 * 75
    x = torch.randn(rows, Cc, generator=g) * (0.5 + 2 * torch.rand(rows, 1, generator=g))
    x[5::7] += 256.0
    x[3] = 3.0 + 1e-4 * torch.randn(Cc, generator=g)
    x[80] = 3.0 + 1e-4 * torch.randn(Cc, generator=g)
    ga, be = 1 + 0.3 * torch.randn(Cc, generator=g), 0.5 * torch.randn(Cc, generator=g)
    ref, tol, _ = R.ln_ref(x, ga, be, eps, m.u_out)
    w = Cc * (2 if m.split else 1)
    out = torch.zeros((rows, w), dtype=m.dt, device=DEV)
    m.eng.op_cvit_ln(x.to(DEV), out, rows, ga.to(DEV), be.to(DEV), eps, mode=0, split=m.split)
    torch.cuda.synchronize()
    _ratio(f"cvit ln mode 0 C={Cc} eps={eps:g} [{name}]", m.get(out), ref, tol)
    if Cc == 192:
        src = torch.from_numpy(R.stitch_source_rows(2))
        out2 = torch.zeros((402, w), dtype=m.dt, device=DEV)
        m.eng.op_cvit_ln(x.to(DEV), out2, 402, ga.to(DEV), be.to(DEV), eps, mode=2, split=m.split)
        torch.cuda.synchronize()
        _ratio(f"cvit ln mode 2 C={Cc} eps={eps:g} [{name}]", m.get(out2), ref[src], tol[src])


# ---- refused calls --------------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _refused(m, fn, args, outs, match):
    keep = [o.cpu().clone() for o in outs]
    rc = getattr(m.eng.lib, fn)(m.eng._h, *args, m.eng._stream())
    torch.cuda.synchronize()
    with pytest.raises(L.PtError, match=match):
        L.check(rc, fn)
    for o, k in zip(outs, keep):
        assert torch.equal(o.cpu(), k), f"{fn} wrote its output although it refused the call"


@pytest.mark.parametrize("name", list(MODES))
def test_rejected_arguments(engines, name):
    m = engines(name)
    sp = int(m.split)
    a16 = torch.full((256, 1152), 0.5, dtype=m.dt, device=DEV)
    f = torch.full((256, 1024), 0.5, dtype=torch.float32, device=DEV)
    o16 = torch.full((256, 1152), -3.5, dtype=m.dt, device=DEV)
    o32 = torch.full((256, 256), -3.5, dtype=torch.float32, device=DEV)
    mlp = lambda Cc, **kw: [_p(kw.get("xb", a16)), 4, Cc, _p(kw.get("w1", a16)), _p(f), _p(a16), _p(f), _p(kw.get("x", o32))]
    if m.split:
        _refused(m, "pt_op_cvit_mlp", mlp(96), [o32], "single-pass modes only")
    else:
        _refused(m, "pt_op_cvit_mlp", mlp(128), [o32], "C = 128")
        _refused(m, "pt_op_cvit_mlp", mlp(96, w1=None), [o32], "null argument")
        _refused(m, "pt_op_cvit_mlp", mlp(96, x=None), [o32], "null argument")
        _refused(m, "pt_op_cvit_mlp", [_p(a16), 0, 96, _p(a16), _p(f), _p(a16), _p(f), _p(o32)], [o32], "rows = 0")
    _refused(m, "pt_op_cvit_attention", [_p(None), 1, _p(o16), sp], [o16], "null argument")
    _refused(m, "pt_op_cvit_attention", [_p(a16), 1, _p(None), sp], [o16], "null argument")
    _refused(m, "pt_op_cvit_attention", [_p(a16), 0, _p(o16), sp], [o16], "nchunks = 0")
    dw = lambda H, Cc, **kw: [_p(kw.get("x", f)), 1, H, 8, Cc, _p(f), _p(f), _p(kw.get("g", f)), _p(f), _p(o16), sp]
    _refused(m, "pt_op_cvit_dwconv_ln", dw(3, 96), [o16], "H = 3")
    _refused(m, "pt_op_cvit_dwconv_ln", dw(8, 520), [o16], "C=520")
    _refused(m, "pt_op_cvit_dwconv_ln", dw(8, 512), [o16], "64 KB of LDS")
    _refused(m, "pt_op_cvit_dwconv_ln", dw(8, 96, g=None), [o16], "null argument")
    ln = lambda mode, H, **kw: [_p(kw.get("x", f)), 16, 96, _p(kw.get("g", f)), _p(kw.get("beta", f)), 1e-6, _p(o16), sp, mode, H, 2, _p(None)]
    _refused(m, "pt_op_cvit_ln", ln(1, 3), [o16], "must be even")
    _refused(m, "pt_op_cvit_ln", ln(1, 1), [o16], "must be even")
    _refused(m, "pt_op_cvit_ln", ln(3, 2), [o16], "mode = 3")
    _refused(m, "pt_op_cvit_ln", ln(0, 1, x=None), [o16], "null argument")
    _refused(m, "pt_op_cvit_ln", ln(0, 1, beta=None), [o16], "gamma and beta go together")
