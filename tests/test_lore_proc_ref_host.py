"""tests/lore_proc_ref.py tied to the oracle (oracle/lore_processor.py, pinned to the reference module by tests/golden/lore_processor.npz), and the
discriminating power of its bounds shown without running a broken kernel anywhere: deliberately wrong variants of the references are compared with
the right ones at cases of tests/test_gpu_lore_proc_ops.py's own lists (R.ATTN_CASES, R.norm_case, R.tok_case), in float64 plus the store of the
mode, and each must leave the bound the GPU test asserts.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lore_proc_ref as R  # noqa: E402
from oracle import lore_processor as olp  # noqa: E402


# ---- tie to the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_norm_is_the_oracles():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, R.D, generator=g, dtype=torch.float64) * 3 + 1
    sd = {"n.alpha": torch.randn(R.D, generator=g, dtype=torch.float64), "n.bias": torch.randn(R.D, generator=g, dtype=torch.float64)}
    want = olp.norm(sd, "n", x)
    got = R.norm_reference(x, sd["n.alpha"], sd["n.bias"])
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_attention_is_the_oracles_mha():
    """mha() with random q / k / v projections and an identity output projection == softmax_attention per head on the projected rows"""
    g = torch.Generator().manual_seed(2)
    sd = {}
    for nm in ("q_linear", "k_linear", "v_linear"):
        sd[f"a.{nm}.weight"] = torch.randn(R.D, R.D, generator=g, dtype=torch.float64) / 16
        sd[f"a.{nm}.bias"] = 0.1 * torch.randn(R.D, generator=g, dtype=torch.float64)
    sd["a.out.weight"], sd["a.out.bias"] = torch.eye(R.D, dtype=torch.float64), torch.zeros(R.D, dtype=torch.float64)
    x = torch.randn(2, 37, R.D, generator=g, dtype=torch.float64) * 2
    want = olp.mha(sd, "a", x)
    for b in range(2):
        rows = torch.cat([x[b] @ sd[f"a.{nm}.weight"].t() + sd[f"a.{nm}.bias"] for nm in ("q_linear", "k_linear", "v_linear")], 1)
        got, _ = R.reference_out_tol(R.attention_reference(rows), "bf16x3")
        assert float((got - want[b]).abs().max()) <= 1e-12 * float(want.abs().max())
    r = R.softmax_attention(x[0, :5, :32], x[0, :, 32:64], x[0, :, 64:96])
    assert torch.allclose(r["p"].sum(-1), torch.ones(5, dtype=torch.float64), rtol=0, atol=1e-13)
    assert bool((r["pav"] >= r["out"].abs() - 1e-15).all()) and bool((r["sabs"] >= r["s"].abs() - 1e-13).all())


def test_token_preparation_is_the_oracles_embedding_add():
    """processor_forward with no encoder layers, identity projections and a decoder bias that keeps both ReLUs open returns its embedded input: equal to
    tok_reference on the indices the stage hands the reference model (int32 cast, round, clamp)"""
    logi, dets, x_pe, y_pe = R.tok_case(5)
    eye, zero = torch.eye(R.D, dtype=torch.float64), torch.zeros(R.D, dtype=torch.float64)
    big = torch.full((R.D,), 1e4, dtype=torch.float64)
    sd = {"x_position_embeddings.weight": x_pe.double(), "y_position_embeddings.weight": y_pe.double(),
          "tsfm_axis.linear.weight": eye, "tsfm_axis.linear.bias": zero, "tsfm_axis.decoder.linear.0.weight": eye, "tsfm_axis.decoder.linear.0.bias": big,
          "tsfm_axis.decoder.linear.2.weight": eye, "tsfm_axis.decoder.linear.2.bias": zero,
          "stacker.logi_encoder.0.weight": torch.zeros(8, R.D, dtype=torch.float64), "stacker.logi_encoder.2.weight": torch.zeros(R.D, 8, dtype=torch.float64),
          "stacker.tsfm.linear.weight": torch.zeros(R.D, 2 * R.D, dtype=torch.float64), "stacker.tsfm.decoder.linear.0.weight": eye,
          "stacker.tsfm.decoder.linear.2.weight": eye}
    for use_pe in (False, True):
        got, mag = R.tok_reference(logi, dets, R.TOK_COUNTS, x_pe, y_pe, use_pe)
        n = 0
        for t, c in enumerate(R.TOK_COUNTS):
            if c:
                ps = torch.zeros(1, c, 8, dtype=torch.int64)
                ps[0, :, [0, 1, 2, 5]] = dets[t, :c][:, [0, 1, 2, 5]].to(torch.int32).to(torch.float32).round().to(torch.int64).clamp(0, 255)
                want = olp.processor_forward(sd, logi[t:t + 1, :c].double(), ps if use_pe else None, 0, 0)[0][0] - 1e4
                assert float((got[n:n + c] - want).abs().max()) <= 1e-11 * 1e4, (t, use_pe)
            n += c
        assert got.shape == (sum(R.TOK_COUNTS), R.D) and bool(torch.isfinite(got).all()) and bool((mag > 0).all())


def test_generators_keep_their_promises():
    """on the storage grid of every mode: the random head's scores have the model's spread, planted keys lead by >= 20 at each seam (clamped into small
    tables), the equal head is flat, the spread head spans more than 100"""
    assert R.seam_marks(1) == (0, 0, 0, 0) and R.seam_marks(33) == (0, 31, 32, 32) and R.seam_marks(700) == (0, 31, 32, 699)
    for mode in R.MODES:
        for counts in ([1], [2], [33], [64], [33, 0, 1, 64, 31, 200]):
            qkv = R.attention_case(counts, mode)
            assert torch.equal(qkv, R.rnd(qkv, mode)) and qkv.shape == (sum(counts), 3 * R.D)
            for t0, c in R.table_rows(counts):
                if c:
                    R.check_patterns(R.attention_reference(qkv[t0:t0 + c]), c)


def test_tolerance_terms():
    """the bound is the sum of its stated terms: at least the store's half-ulp, growing with the key count, and the fp32 terms stay small"""
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(n, R.DK, generator=g, dtype=torch.float64) for n in (3, 130, 130))
    r = R.softmax_attention(q, k, v)
    for mode in R.MODES:
        t1 = R.attention_tol(r, v, mode)
        assert bool((t1 >= R.U_OUT[mode] * r["out"].abs()).all())
        assert bool((t1 <= (R.U_OUT[mode] + 2.0 ** -15) * (r["out"].abs() + r["pav"]) + 3e-4 * (r["pav"] + r["out"].abs()) + 1e-6).all())   # 2 (2^-16 + 98 E32) sabs, sabs < 5
    assert R.attention_counts(33, "bf16") == (34, 2, 64 + 2 + 2) and R.attention_counts(3000, "bf16x3") == (98, 94, 96 * 94 + 94 + 2)
    assert R.npad_of(0) == 128 and R.npad_of(128) == 128 and R.npad_of(129) == 256 and R.npad_of(sum(R.TOK_COUNTS)) == 256


# ---- what the bounds separate ----------------------------------------------------------------------------------------------------------------------
def _online(q, k, v, rescale=True):
    """the kernel's loop over 32-key tiles in float64: running maximum m, row sum l, accumulator acc; rescale=False leaves acc without its factor
    e^(m - mn) (the row sum keeps it)"""
    s = q @ k.t() / R.SCALE
    m = torch.full((q.shape[0], 1), -float("inf"), dtype=torch.float64)
    l = torch.zeros(q.shape[0], 1, dtype=torch.float64)
    acc = torch.zeros(q.shape[0], R.DK, dtype=torch.float64)
    for k0 in range(0, k.shape[0], 32):
        st = s[:, k0:k0 + 32]
        mn = torch.maximum(m, st.max(-1, keepdim=True).values)
        scale = torch.exp(m - mn)
        p = torch.exp(st - mn)
        l = l * scale + p.sum(-1, keepdim=True)
        acc = (acc * scale if rescale else acc) + p @ v[k0:k0 + 32]
        m = mn
    return acc / l


def _attn_variant(kind, qkv, counts):
    """[N, 256] float64 of a wrong attention over the whole batch"""
    out = torch.zeros(qkv.shape[0], R.D, dtype=torch.float64)
    spans = [sp for sp in R.table_rows(counts) if sp[1]]
    for i, (t0, c) in enumerate(spans):
        q, k, v = (qkv[t0:t0 + c, j * R.D:(j + 1) * R.D].reshape(c, R.HEADS, R.DK) for j in range(3))
        if kind == "last key dropped" and c > 1:
            k, v = k[:-1], v[:-1]
        elif kind == "partial last tile dropped" and c > 32 and c % 32:
            k, v = k[:c // 32 * 32], v[:c // 32 * 32]
        elif kind == "neighbour's keys":
            n0 = spans[(i + 1) % len(spans)][0]                                  # the next table's first token in place of its own
            rows = (n0 + torch.arange(c)).clamp(max=qkv.shape[0] - 1)
            k, v = (qkv[rows, j * R.D:(j + 1) * R.D].reshape(c, R.HEADS, R.DK) for j in (1, 2))
        for h in range(R.HEADS):
            out[t0:t0 + c, h * R.DK:(h + 1) * R.DK] = _online(q[:, h], k[:, h], v[:, h], rescale=kind != "no rescale")
    return out


# variant -> the cases of R.ATTN_CASES at which it must leave the bound, in every mode
ATTN_VARIANTS = {
    "right": [],
    "last key dropped": [[2], [33], [64], [700], [R.MAX_CELLS], [33, 0, 1, 64, 31, 200]],
    "partial last tile dropped": [[33], [65], [97], [33, 0, 1, 64, 31, 200]],
    "no rescale": [[33], [64], [700]],
    "neighbour's keys": [[33, 0, 1, 64, 31, 200]],
}


@pytest.mark.parametrize("mode", R.MODES)
def test_attention_bound_separates_the_wrong_variants(mode):
    """the online loop itself (variant "right") stays at fp64 noise of the reference on every case; each wrong variant, stored in the mode, exceeds the
    asserted bound at its cases.  The 3000-key case is checked once, for the dropped last key."""
    for counts in R.ATTN_CASES:
        assert all(c in R.ATTN_CASES for cs in ATTN_VARIANTS.values() for c in cs)
        kinds = [kd for kd, cs in ATTN_VARIANTS.items() if counts in cs or (kd == "right" and sum(counts) <= 700)]
        if not kinds:
            continue
        qkv = R.attention_case(counts, mode)
        refs = [(t0, c, R.reference_out_tol(R.attention_reference(qkv[t0:t0 + c]), mode)) for t0, c in R.table_rows(counts) if c]
        for kd in kinds:
            got = R.rnd(_attn_variant(kd, qkv, counts), mode)
            ratio = max(float(((got[t0:t0 + c] - out).abs() / tol).max()) for t0, c, (out, tol) in refs)
            print(f"attention [{mode}] {counts}: {kd}: err/tol {ratio:.3g}")
            if kd == "right":
                assert ratio <= 1.0, (counts, ratio)
            else:
                assert ratio > 1.0, (kd, counts, ratio)


def _norm_variant(kind, x, alpha, bias):
    xd, a, b = x.double(), alpha.double(), bias.double()
    d = xd - xd.mean(-1, keepdim=True)
    q = (d * d).sum(-1, keepdim=True)
    if kind == "biased std":
        return a * d / ((q / R.D).sqrt() + R.EPS) + b
    if kind == "eps in the variance":
        return a * d / (q / (R.D - 1) + R.EPS).sqrt() + b
    assert kind == "one-pass variance"
    mean = x.mean(-1, keepdim=True)                                             # fp32 throughout, as a kernel would
    var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp(min=0.0) * (R.D / (R.D - 1.0))
    return (alpha * (x - mean) / (var.sqrt() + R.EPS) + bias).double()


@pytest.mark.parametrize("mode", R.MODES)
def test_norm_bound_separates_the_wrong_variants(mode):
    """sqrt(256 / 255) - 1 = 0.196 % is about one bf16 half-ulp (2^-9 = 0.195 %, the store's bound is 2^-8), so the biased std is expected to be
    separable in BF16X3 and f16 only: it is asserted there, and only printed for bf16, where no case is stretched to separate it (what the bf16 line
    shows comes from the few elements at which alpha d / den and bias cancel, so that the store of the small sum is fine enough to see 0.2 % of the
    large term; nothing is built on that).  eps in the variance shows on the row whose std is 1e-7,
    the one-pass variance on the row of mean 1000 (x^2 ~ 1e6 leaves 2^-24 1e6 = 0.06 of a variance of 1)."""
    x, alpha, bias, kinds = R.norm_case(129, 129)
    ref, tol = R.norm_reference(x, alpha, bias), R.norm_tol(x, alpha, bias, mode)
    assert float(((R.rnd(ref, mode) - ref).abs() / tol).max()) <= 1.0
    rows = {kd: [i for i, k2 in enumerate(kinds) if k2 == kd] for kd in R.NORM_KINDS}
    for kd, where in (("biased std", "random"), ("eps in the variance", "tiny"), ("one-pass variance", "mean1000")):
        got = R.rnd(_norm_variant(kd, x, alpha, bias), mode)
        ratio = float(((got - ref).abs() / tol)[rows[where]].max())
        print(f"norm [{mode}] rows of kind {where}: {kd}: err/tol {ratio:.3g}")
        if kd == "biased std" and mode == "bf16":
            continue
        assert ratio > 1.0, (kd, mode, ratio)


def test_token_preparation_bound_separates_rounding_and_clamp_order_is_no_variant():
    """an index that rounds where it should truncate takes another table row at 11.5 and 254.999 (10.5 ties to even: 10 either way) and leaves the
    bound in every mode.  Clamping BEFORE the truncation is not a mistake the outputs can show: trunc is monotone and fixes 0 and 255, so
    clamp(trunc(x), 0, 255) == trunc(clamp(x, 0, 255)) for every x an int32 holds -- asserted here over the planted coordinates and a sweep."""
    logi, dets, x_pe, y_pe = R.tok_case(5)
    ref, t32 = R.tok_reference(logi, dets, R.TOK_COUNTS, x_pe, y_pe, True)
    rounded = lambda d: d.round().to(torch.int64).clamp(0, 255)
    early = lambda d: d.clamp(0.0, 255.0).to(torch.int32).to(torch.int64)
    sweep = torch.cat([torch.tensor(R.PLANTED), torch.linspace(-300.0, 600.0, 90001), torch.tensor([-2.0 ** 31, 2.0 ** 31 - 128, -1e-30, 1e-30])])
    assert torch.equal(early(sweep), R.tok_index(sweep))
    assert R.tok_index(torch.tensor(R.PLANTED)).tolist() == [0, 0, 0, 10, 11, 254, 255, 255, 255, 255, 255]
    assert rounded(torch.tensor(R.PLANTED)).tolist() == [0, 0, 0, 10, 12, 255, 255, 255, 255, 255, 255]
    for col in (0, 1, 2, 5):                                                   # every planted value is met in every column the operation reads
        seen = set(torch.cat([dets[t, :c, col] for t, c in enumerate(R.TOK_COUNTS)]).tolist())
        assert {float(torch.tensor(p, dtype=torch.float32)) for p in R.PLANTED} <= seen
    for mode in R.MODES:
        tol = t32 + R.store_tol(ref, mode)
        assert float(((R.rnd(ref, mode) - ref).abs() / tol).max()) <= 1.0
        got = R.rnd(R.tok_reference(logi, dets, R.TOK_COUNTS, x_pe, y_pe, True, index=rounded)[0], mode)
        ratio = float(((got - ref).abs() / tol).max())
        print(f"token preparation [{mode}]: rounded index: err/tol {ratio:.3g}")
        assert ratio > 1.0
        same = R.tok_reference(logi, dets, R.TOK_COUNTS, x_pe, y_pe, True, index=early)[0]
        assert torch.equal(same, ref)
