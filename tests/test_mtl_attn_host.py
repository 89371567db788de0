"""tests/mtl_attn_ref.py tied to things it does not share code with: the oracle's own attention (oracle/mtl_tabnet.py::_mha, pinned to the reference
module by tests/test_oracle_mtl_tabnet.py), torch.softmax in float64, the e4m3 grid written out by hand; and pick_split()'s contract, read through the
library's host entry point.  No GPU."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mtl_attn_ref as R  # noqa: E402
from oracle import mtl_tabnet as omt  # noqa: E402


def _identity_mha(p, g, d=R.D):
    """state dict of a MultiHeadAttention with random q / k / v projections and an identity output projection, float64"""
    sd = {}
    for i in range(3):
        sd[f"{p}.linears.{i}.weight"] = torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d)
        sd[f"{p}.linears.{i}.bias"] = 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
    sd[f"{p}.linears.3.weight"] = torch.eye(d, dtype=torch.float64)
    sd[f"{p}.linears.3.bias"] = torch.zeros(d, dtype=torch.float64)
    return sd


def _lin(sd, p, i, t):
    return t @ sd[f"{p}.linears.{i}.weight"].t() + sd[f"{p}.linears.{i}.bias"]


@pytest.mark.parametrize("shared_kv", [False, True])
def test_source_attention_is_the_oracles(shared_kv):
    """MultiHeadAttention (one table per row batch) and MultiHeadAttentionCell (all rows share one table's keys): _mha on random float64 inputs ==
    softmax_attention per head on q and k / 8"""
    g = torch.Generator().manual_seed(5 + shared_kv)
    sd = _identity_mha("a", g)
    nb, nq, hw = (4, 1, 37) if shared_kv else (2, 3, 37)
    x = torch.randn(nb, nq, R.D, generator=g, dtype=torch.float64) * 2
    feat = torch.randn(1 if shared_kv else nb, hw, R.D, generator=g, dtype=torch.float64) * 2
    with torch.no_grad():
        want = omt._mha(sd, "a", x, feat, None, shared_kv=shared_kv)
    for b in range(nb):
        fb = feat[0 if shared_kv else b]
        q = _lin(sd, "a", 0, x[b]).reshape(nq, R.HEADS, R.DK)
        k = (_lin(sd, "a", 1, fb) / 8.0).reshape(hw, R.HEADS, R.DK)
        v = _lin(sd, "a", 2, fb).reshape(hw, R.HEADS, R.DK)
        got = torch.stack([R.softmax_attention(q[:, h], k[:, h], v[:, h])["out"] for h in range(R.HEADS)], 1).reshape(nq, R.D)
        assert float((got - want[b]).abs().max()) <= 1e-12 * float(want.abs().max())


def test_self_attention_and_the_pad_query_rule_are_the_oracles():
    """_mha under make_mask (_tgt_mask): causal rows, and the row of a <PAD> token attending uniformly to ALL positions, later ones included"""
    g = torch.Generator().manual_seed(9)
    sd = _identity_mha("s", g)
    L, pad = 9, 3
    tokens = torch.tensor([[5, 7, 1, pad, 2, 9, 9, 4, 6], [pad, 1, 2, 8, 5, 5, 6, 7, pad]])
    h = torch.randn(2, L, R.D, generator=g, dtype=torch.float64) * 2
    with torch.no_grad():
        want = omt._mha(sd, "s", h, h, omt._tgt_mask(tokens, pad))
    for b in range(2):
        q = _lin(sd, "s", 0, h[b]).reshape(L, R.HEADS, R.DK)
        k = (_lin(sd, "s", 1, h[b]) / 8.0).reshape(L, R.HEADS, R.DK)
        v = _lin(sd, "s", 2, h[b]).reshape(L, R.HEADS, R.DK)
        for p in range(L):
            is_pad = int(tokens[b, p]) == pad
            got = torch.cat([R.self_attention_row(q[p, hh], k[:, hh], v[:, hh], p, is_pad)["out"] for hh in range(R.HEADS)])
            assert float((got - want[b, p]).abs().max()) <= 1e-12 * float(want.abs().max()), (b, p)
            if is_pad:
                assert torch.allclose(got, v.mean(0).reshape(-1), rtol=0, atol=1e-12)


def test_softmax_attention_is_torch_softmax_and_its_side_sums():
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(n, R.DK, generator=g, dtype=torch.float64) for n in (5, 70, 70))
    r = R.softmax_attention(q, k, v)
    s = torch.einsum("qd,kd->qk", q, k)
    assert torch.allclose(r["s"], s, rtol=0, atol=1e-13)
    assert torch.allclose(r["out"], torch.softmax(s, -1) @ v, rtol=0, atol=1e-13)
    assert torch.allclose(r["p"].sum(-1), torch.ones(5, dtype=torch.float64), rtol=0, atol=1e-13)
    assert bool((r["pav"] >= r["out"].abs() - 1e-15).all()) and bool((r["sabs"] >= r["s"].abs() - 1e-13).all())


def test_e4m3_round_trip_against_the_grid_written_out():
    """every one of the 254 finite e4m3 patterns decodes to (1 + m / 8) 2^(e - 7) (subnormals m 2^-9), encodes back to itself, and a value between
    two neighbours goes to the nearer one, to the even pattern on a tie; beyond +-448 / 8 it saturates"""
    pats = torch.tensor([b for b in range(256) if (b & 127) != 127], dtype=torch.uint8)
    vals = R.e4m3_decode(pats)
    for b, x in zip(pats.tolist(), vals.tolist()):
        e, m = (b >> 3) & 15, b & 7
        mag = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        assert x == (-mag if b & 128 else mag), b
    assert torch.equal(R.e4m3_bytes(vals / 8.0), pats)
    pos = vals[:127]                                                     # patterns 0 .. 126 ascending
    mid = (pos[:-1] + pos[1:]) / 2
    even = torch.where(torch.arange(126) % 2 == 0, pats[:126], pats[1:127])
    assert torch.equal(R.e4m3_bytes(mid / 8.0), even)
    assert torch.equal(R.e4m3_bytes((mid * (1 + 2.0 ** -10)) / 8.0), pats[1:127]) and torch.equal(R.e4m3_bytes((mid * (1 - 2.0 ** -10)) / 8.0), pats[:126])
    assert R.e4m3_bytes(torch.tensor([100.0, -100.0, 56.0, 60.0])).tolist() == [126, 254, 126, 126]
    assert torch.equal(R._e4m3_by_hand(torch.cat([vals, mid, -mid]).float()), R.e4m3_bytes(torch.cat([vals, mid, -mid]) / 8.0))


def test_generators_keep_their_promises():
    """planted keys lead by >= 20 at each of the four seams, the equal head is flat, the spread head spans more than 100 -- in every storage mode, and
    over the e4m3 copy of the keys too"""
    for mode in ("bf16", "f16", "bf16x3"):
        hw, kps, ns = 200, 96, 3
        marks = R.seam_marks(hw, 64, kps, ns)
        assert marks == (0, 63, 192, 199)
        kv, us = R.cross_case(2, hw, (0, 4), marks, mode, 11)
        assert torch.equal(kv, R.rnd(kv, mode))
        g = torch.Generator().manual_seed(3)
        for sl in (0, 4):
            for b in range(2):
                q = R.rnd(R.make_queries(4, us[sl][b], g).reshape(4, R.D), mode)
                R.check_patterns(R.cross_reference(q, kv, hw, b, sl), marks)
                if mode == "bf16":
                    kv8 = R.e4m3_decode(R.e4m3_bytes(kv)) / 8.0
                    R.check_patterns(R.cross_reference(q, kv8, hw, b, sl), marks)
    assert R.seam_marks(1, 64, 32, 1) == (0, 0, 0, 0) and R.seam_marks(496, 64, 32, 16) == (0, 63, 480, 495)


def test_tolerance_terms():
    """the bound is the sum of its stated terms: at least the store's half-ulp, growing with the slice length, larger for the MFMA kernel by P's rounding"""
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(n, R.DK, generator=g, dtype=torch.float64) for n in (3, 130, 130))
    r = R.softmax_attention(q, k, v)
    for mode in ("bf16", "f16", "bf16x3"):
        t1 = R.attention_tol(r, v, "stream", mode, 130, 1)
        t2 = R.attention_tol(r, v, "stream", mode, 4096, 1)
        tm = R.attention_tol(r, v, "mfma", mode, 130, 1, x3_products=mode == "bf16x3")
        assert bool((t1 >= R.U_OUT[mode] * r["out"].abs()).all()) and bool((t2 > t1).all()) and bool((tm > t1).all())
        assert bool((t1 <= R.U_OUT[mode] * r["out"].abs() + 1e-4 * (r["pav"] + r["out"].abs()) + 1e-7).all())      # the fp32 terms stay small
    assert R.shape_counts("stream", 64, 1) == (11, 2, 8 + 2 + 3 + 1) and R.shape_counts("stream8", 300, 2) == (18, 3 + 1 + 1, 19 + 5 + 4 + 4 + 1)
    assert R.shape_counts("mfma", 33, 1) == (64, 2, 33 + 2 + 1 + 1)


# ---- pick_split through the library's host entry point -----------------------------------------------------------------------------------------
def test_pick_split_contract():
    """for every (tiles, hw) the loops can ask for: slices of a multiple of 32 keys, at most 16 of them, covering hw with a last slice that holds a key"""
    from pdf_table_amd.build import build
    from pdf_table_amd.engine import mtl_pick_split
    from pdf_table_amd import lib as L
    build(verbose=False)
    for hw in (1, 31, 32, 33, 600, 3600, 4096):
        for tiles in range(1, 601):
            ns, kps = mtl_pick_split(tiles, hw)
            assert kps % 32 == 0 and 1 <= ns <= 16 and (ns - 1) * kps < hw <= ns * kps, (tiles, hw, ns, kps)
    assert mtl_pick_split(3, 24) == (1, 32) and mtl_pick_split(2, 48) == (2, 32)         # what the decoder tests' 3x8 and 6x8 maps run
    assert mtl_pick_split(87, 3600)[0] > 1
    with pytest.raises(L.PtError, match="hw = 4097"):
        mtl_pick_split(1, 4097)
    with pytest.raises(L.PtError, match="ntiles = 0"):
        mtl_pick_split(0, 10)
