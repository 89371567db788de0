"""CPU half of the op-level tests of the ConvNextViT recogniser's kernels: every float64 reference of tests/cvit_ops_ref.py is tied to something
independent of it, the generators produce the edges they are named after, the fused-MLP weight packer writes the layout cvit_mlp_kernel reads, and
the committed GELU polynomial meets the contract the GPU probe asserts (tests/test_gpu_cvit_ops.py)."""
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvit_ops_ref as R  # noqa: E402
from oracle import convnext_vit as ocv  # noqa: E402
from pdf_table_amd import weights as Wt  # noqa: E402


def _vals(bits, fmt):
    return torch.from_numpy(bits.view(np.int16).copy()).view(R.DT[fmt]).double()


# ---- the packer --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("C", [96, 192, 256])
def test_pack_cvit_mlp_layout(C, fmt):
    """W2p is [chunk][C][32] and slot (s2, half, j) of chunk hc holds hidden unit 32 hc + (j & 3) + 8 (2 s2 + (j >> 2)) + 4 half"""
    # W2[o, k] = a value that names (o, k) and survives the rounding: o in the high bits, k % 32 and the chunk in separate small integers
    o, k = torch.meshgrid(torch.arange(C), torch.arange(4 * C), indexing="ij")
    w2 = (k % 32 + 1).double() * torch.pow(2.0, -(o % 7).double())                 # 5 significant bits: exact in both formats
    w1 = torch.randn(4 * C, C, generator=torch.Generator().manual_seed(C)).double()
    w1b, w2pb = Wt.pack_cvit_mlp(w1.float(), w2.float(), fmt)
    assert w1b.shape == (4 * C, C) and w1b.dtype == np.uint16 and w2pb.shape == (4 * C // 32, C, 32) and w2pb.dtype == np.uint16
    assert torch.equal(_vals(w1b, fmt), R.rnd(w1.float(), fmt)), "W1 is stored as it is, rounded to the storage format"
    units = Wt.cvit_mlp_slot_units()
    assert units.shape == (2, 2, 8) and sorted(units.reshape(-1).tolist()) == list(range(32)), "the column permutation is a bijection"
    got = _vals(w2pb, fmt)
    for s2 in range(2):
        for half in range(2):
            for j in range(8):
                unit = (j & 3) + 8 * (2 * s2 + (j >> 2)) + 4 * half
                assert units[s2, half, j] == unit
                slot = s2 * 16 + half * 8 + j
                for hc in (0, 1, 4 * C // 32 - 1):
                    assert torch.equal(got[hc, :, slot], w2[:, 32 * hc + unit]), (s2, half, j, hc)
    # a second matrix that tells the chunks apart
    w2c = (k // 32 + 1).double() / 64.0
    _, p2 = Wt.pack_cvit_mlp(w1.float(), w2c.float(), fmt)
    assert torch.equal(_vals(p2, fmt), ((torch.arange(4 * C // 32) + 1).double() / 64.0)[:, None, None].expand(-1, C, 32))


def test_the_model_packer_uses_pack_cvit_mlp():
    from pdf_table_amd.synth_weights import convnext_vit_state_dict
    sd = convnext_vit_state_dict(seed=29)
    blob = Wt.pack_convnext_vit(sd, x3=False)
    n = struct.unpack("<I", blob[4:8])[0]
    ten = {}
    for i in range(n):
        rec = struct.unpack("<96sII6IQQ", blob[8 + i * 144: 8 + (i + 1) * 144])
        ten[rec[0].split(b"\0")[0].decode()] = (rec[9], rec[10])
    w1 = sd["vitstr.vit.encoder.layer.3.intermediate.dense.weight"].float()
    w2 = sd["vitstr.vit.encoder.layer.3.output.dense.weight"].float()
    w1b, w2pb = Wt.pack_cvit_mlp(w1, w2, "bf16")
    for name, want in (("vit.l3.mlp.w1", w1b), ("vit.l3.mlp.w2p", w2pb)):
        off, nb = ten[name]
        assert np.array_equal(np.frombuffer(blob, np.uint16, nb // 2, off), want.reshape(-1)), name
    assert "s3.l0.mlp.w1" not in ten and "s2.l7.mlp.w2p" in ten          # C = 512 keeps the two GEMMs


# ---- references against independent implementations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C", [(8, 11, 96), (1, 5, 40), (2, 8, 64)])
def test_dwconv_ln_ref_is_conv2d_plus_layer_norm(H, W, C):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, C, generator=g, dtype=torch.float64)
    w49 = torch.randn(49, C, generator=g, dtype=torch.float64) * 0.2
    bias, ga, be = (torch.randn(C, generator=g, dtype=torch.float64) for _ in range(3))
    y, tol, q = R.dwconv_ln_ref(x, w49, bias, ga, be, 2.0 ** -8)
    conv = F.conv2d(x.permute(0, 3, 1, 2), w49.t().reshape(C, 1, 7, 7), bias, padding=3, groups=C).permute(0, 2, 3, 1)
    want = F.layer_norm(conv, (C,), ga, be, 1e-6)
    assert (y - want).abs().max() <= 1e-12
    assert torch.allclose(q[..., 0], conv.var(-1, unbiased=False), rtol=1e-10, atol=1e-14) and bool((tol > 0).all())


def test_ln_ref_is_layer_norm():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(9, 192, generator=g, dtype=torch.float64) * 3 + 256
    ga, be = torch.randn(192, generator=g, dtype=torch.float64), torch.randn(192, generator=g, dtype=torch.float64)
    for eps in (1e-6, 1e-12):
        y, _, _ = R.ln_ref(x, ga, be, eps, 2.0 ** -8)
        assert (y - F.layer_norm(x, (192,), ga, be, eps)).abs().max() <= 1e-9


def test_stitch_map_is_the_oracles_stitching():
    n = 2
    seq = torch.arange(3 * n * R.CV_T, dtype=torch.float64).reshape(3 * n, R.CV_T, 1).expand(-1, -1, 2).contiguous()     # a token holds its own row number
    want = ocv.stitch_chunks(seq).reshape(n * R.LINE_T, 2)[:, 0].long().numpy()
    src = R.stitch_source_rows(n)
    assert np.array_equal(src, want)
    # the borders by name: 68 | 69 is chunk 0 token 68 | chunk 1 token 6, 131 | 132 is chunk 1 token 68 | chunk 2 token 6, 200 is chunk 2 token 74
    assert [int(src[R.LINE_T + p]) - 3 * R.CV_T for p in (0, 68, 69, 131, 132, 200)] == [0, 68, 75 + 6, 75 + 68, 150 + 6, 150 + 74]
    cmap = np.array([4, 1, 1, 0, 1, 1], np.int32)                                   # line-chunks sharing one compact chunk
    shared = R.stitch_source_rows(n, cmap)
    full = seq.reshape(-1, 2)[:, 0].reshape(3 * n, R.CV_T)
    compact = torch.stack([full[3], full[1], full[2], full[2], full[0]])            # any five chunks; cmap picks among them
    line_chunks = compact[torch.from_numpy(cmap).long()]                            # what the lines see: [6, 75]
    want2 = ocv.stitch_chunks(line_chunks.reshape(3 * n, R.CV_T, 1).contiguous()).reshape(-1)
    assert torch.equal(compact.reshape(-1)[torch.from_numpy(shared)], want2)


@pytest.mark.parametrize("H", [8, 4, 2])
def test_pair_rows_is_the_k_layout_of_the_2x1_conv(H):
    B, W, C, N = 2, 5, 12, 7
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(N, C, 2, 1, generator=g, dtype=torch.float64)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, stride=(2, 1)).permute(0, 2, 3, 1).reshape(-1, N)      # cnn_forward_fp32's down-sampler
    wk = w[:, :, :, 0].permute(0, 2, 1).reshape(N, 2 * C)                                              # weights.py: K = row * Cin + c
    got = R.pair_rows(x.reshape(-1, C), B, H, W) @ wk.t()
    assert (got - want).abs().max() <= 1e-12


def test_attention_ref_is_softmax_qk_v_per_head():
    qkv = R.attention_case(3, "normal", 5)
    out, pav, s = R.attention_ref(qkv)
    for c in range(3):
        rows = qkv[c * 75:(c + 1) * 75]
        for h in range(3):
            q, k, v = (rows[:, p * 192 + h * 64: p * 192 + (h + 1) * 64] for p in range(3))
            want = torch.softmax(q @ k.t(), -1) @ v
            assert (out[c * 75:(c + 1) * 75, h * 64:(h + 1) * 64] - want).abs().max() <= 1e-12
    assert bool((pav >= out.abs() - 1e-12).all())


def test_mlp_ref_is_linear_gelu_linear():
    xb, w1, b1, w2, b2, x = R.mlp_case(96, 9, 1.3, "bf16", 1)
    ref, tol, pre = R.mlp_ref(xb, w1, b1, w2, b2, x, "bf16")
    want = x + F.linear(F.gelu(F.linear(xb, w1, b1)), w2, b2)
    assert (ref - want).abs().max() <= 1e-12 and bool((tol > 0).all())


# ---- the generators produce their edges ---------------------------------------------------------------------------------------------------------------
def test_mlp_gains_reach_the_clamp():
    for fmt in ("bf16", "f16"):
        pre = R.mlp_ref(*R.mlp_case(192, 200, 1.3, fmt, 2), fmt)[2]
        assert 4.0 < pre.abs().max() < 7.0
        pre = R.mlp_ref(*R.mlp_case(192, 200, 4.1, fmt, 3), fmt)[2]
        assert 15.0 < pre.abs().max() < 24.0 and 0.25 < float((pre.abs() > 4).double().mean()) < 0.4
        assert float((pre < -4).double().mean()) > 0.1


def test_attention_families():
    mid = slice(75, 150)
    for fmt in ("bf16", "f16"):
        for fam in R.ATT_FAMILIES:
            qkv = R.rnd(R.attention_case(3, fam, 11), fmt)
            out, pav, s = R.attention_ref(qkv)
            p = torch.softmax(s[1], -1)                                             # the chunk under test: [head, query, key]
            assert s.abs().max() <= 20.0, (fam, float(s.abs().max()))
            if fam == "normal":
                assert 0.5 < float(s[1].std()) < 2.0
            elif fam == "peaked":
                assert 12.0 < float(s[1].abs().max()) <= 20.0 and float(p.max(-1).values.median()) > 0.9 and float(p.max()) > 0.99
            elif fam == "planted":
                i = torch.arange(75)
                top = p.argmax(-1)
                assert bool((top[:, i % 3 == 0] == 74).all()) and bool((top[:, i % 3 == 1] == 0).all()) and bool((top[:, i % 3 == 2] >= 64).all())
                up = s[1][:, i % 3 != 1]
                jump = up[..., 64:].max(-1).values - up[..., :64].max(-1).values    # what the running maximum rises by at the last tile
                assert float(jump.min()) > 12.0
                assert float(p[:, i % 3 == 0][..., 74].min()) > 0.5
            else:
                assert float(s[1].abs().max()) == 0.0
                v = qkv[mid, 384:].double()
                assert (out[mid] - v.mean(0, keepdim=True)).abs().max() <= 1e-12
            # another chunk's keys would take over: the middle chunk's queries against chunk 0's keys
            if fam != "equal":
                q1 = qkv[mid, :192].reshape(75, 3, 64)
                k0 = qkv[:75, 192:384].reshape(75, 3, 64)
                leak = torch.einsum("ihd,jhd->hij", q1, k0)
                assert float((leak.max(-1).values - s[1].max(-1).values).median()) > 3.0


# ---- the GELU contract, on the CPU ---------------------------------------------------------------------------------------------------------------
def test_committed_gelu_polynomial_meets_the_contract_but_not_the_old_comment():
    x = torch.cat([torch.linspace(-12, 12, 240001, dtype=torch.float64), torch.linspace(-4.01, -3.99, 2001, dtype=torch.float64),
                   torch.linspace(3.99, 4.01, 2001, dtype=torch.float64)])
    ref = R.gelu_erf(x)
    for dtype in (torch.float64, torch.float32):
        xs = x.to(dtype).double()
        err = (R.gelu_poly(xs, dtype) - R.gelu_erf(xs)).abs()
        assert bool((err <= R.gelu_delta(xs)).all()), float((err / R.gelu_delta(xs)).max())
    err = (R.gelu_poly(x) - ref).abs()
    inside = x.abs() <= 4
    # what the comment above gelu_pair used to promise (absolute error < 3e-6 on [-4, 4]) does not hold for these coefficients
    assert float(err[inside].max()) > 3e-6
    assert float(err[inside].max()) < 2.0 ** -15


def test_mlp_bound_has_room_for_a_correct_kernel_and_none_for_a_dropped_chunk():
    """a float32 emulation of the kernel's arithmetic (bf16 hidden values, the committed polynomial) against the bound the GPU test asserts"""
    for C, gain in ((96, 1.3), (96, 4.1), (256, 4.1)):
        xb, w1, b1, w2, b2, x = R.mlp_case(C, 37, gain, "bf16", 7)
        ref, tol, _ = R.mlp_ref(xb, w1, b1, w2, b2, x, "bf16")
        pre = (xb.float() @ w1.float().t() + b1.float())
        h = R.rnd(R.gelu_poly(pre.double(), torch.float32), "bf16")
        got = (x.float() + (h.float() @ w2.float().t() + b2.float())).double()
        assert float(((got - ref).abs() / tol).max()) <= 0.6
        h[:, 64:96] = 0                                                            # chunk 2 dropped
        bad = (x.float() + (h.float() @ w2.float().t() + b2.float())).double()
        assert float(((bad - ref).abs() / tol).max()) > 2.0
