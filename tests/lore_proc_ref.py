"""Plain float64 references of the Lore processor's five kernels (csrc/lore_processor.hip), with the error bounds the GPU tests assert, the operand
generators and the case lists both suites share.  No GPU, no engine: tests/test_lore_proc_ref_host.py ties every function here to the oracle
(oracle/lore_processor.py) and shows which mistakes the bounds separate; tests/test_gpu_lore_proc_ops.py compares the kernels with them.

The operations, as the reference model defines them (lore_processor.py:117-163, 465-514; restated in oracle/lore_processor.py):
  attention        out[q, head] = softmax_k(q_head . k_head[k] / sqrt(32)) v_head[k] over the cells of the query's own table, 256 = 8 heads of 32.
  norm             alpha (x - mean) / (std + 1e-6) + bias over 256 channels, std unbiased (/ 255), eps added to the std.
  token preparation  x = logi + x_pe[p0] + y_pe[p1] + x_pe[p2] + y_pe[p5], p_i = clamp(trunc(dets_i), 0, 255): the float quad is cast to int32
                   (truncation towards zero), then rounded (a no-op on integers) and clamped.
  cvt_logic, scatter4   copies: 4 of 8 fp32 columns to a zero-padded 16-bit row of 32 / to row r of table b.

Storage formats: "bf16" / "f16" single pass, "bf16x3" = (hi | lo) bf16 pairs.  Every constant below is derived from the arithmetic a kernel is specified to
do; none is fitted to a kernel:
  U_OUT    the largest relative error of one round-to-nearest store (the format's unit round-off): 2^-8 for bf16 (8 significant bits), 2^-11 for f16
           (11 bits).  Its mean magnitude is half that (2^-9 / 2^-12); the bounds use the largest.  A (hi | lo) pair stores hi = bf16(x) and
           lo = bf16(x - hi) with |x - hi| <= 2^-8 |x|, so |x - hi - lo| <= 2^-16 |x|.  f16 only: below 2^-14 the spacing is 2^-24, so a store is off by
           up to 2^-25 absolute whatever the value.
  E32      fp32 unit round-off 2^-24: n dependent fp32 operations on a sum are off by at most n 2^-24 of the sum of magnitudes (first order).
  EXP_ULP  expf, the division and sqrtf of the HIP device library: at most 1 ulp = 2^-23 relative.
  F32_MIN  2^-126: a weight below fp32's normal range may be flushed to 0.
"""
import math

import torch

from mtl_attn_ref import DT, E32, EXP_ULP, U_OUT, fmt_of, rnd, split_pair  # noqa: F401  (the formats are the same; re-exported for the tests)

HEADS, DK, D = 8, 32, 256
SCALE = math.sqrt(DK)
MAX_CELLS = 3000                       # lib.PT_TSR_MAX_CELLS
EPS = 1e-6
F32_MIN = 2.0 ** -126
MODES = ("bf16", "f16", "bf16x3")


def npad_of(n):
    return max(128, (n + 127) // 128 * 128)


# ---- attention ---------------------------------------------------------------------------------------------------------------------------------
def softmax_attention(q, k, v):
    """q [nq, 32], k / v [nk, 32] float64 -> dict: out [nq, 32], s scores [nq, nk], p normalised weights, pav = sum_k p |v|,
    sabs[q, k] = sum_j |q_j k_j| / sqrt(32) (what a rounding of the dot product is relative to)"""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.t() / SCALE
    p = torch.softmax(s, -1)
    return dict(out=p @ v, s=s, p=p, pav=p @ v.abs(), sabs=q.abs() @ k.abs().t() / SCALE)


def attention_counts(nk, mode):
    """(n_dot, n_steps, n_acc): dependent fp32 operations of attention_kernel<SPLIT>, from its loop structure.
    n_dot: additions behind one score: 32 products per pass accumulated by the matrix pipe in an order we do not assume, three passes into the same
      accumulator in the pair mode (hi hi + hi lo + lo hi), + 2 for the division by sqrtf(32) and that constant's own rounding.
    n_steps: factors e^x a weight passes through: its own expf, then one rescale per later 32-key tile = at most the number of tiles; each costs an
      expf (EXP_ULP), a subtraction and a product (E32 each).
    n_acc: additions behind one output sum: every key slot of every tile enters an MFMA sum (32 per tile and pass), + one rescale per tile, + the
      exchange of the row sum with lane ^ 32, + the division."""
    tiles = -(-nk // 32)
    passes = 3 if mode == "bf16x3" else 1
    return 32 * passes + 2, tiles, 32 * passes * tiles + tiles + 2


def attention_tol(r, v, mode):
    """Tolerance [nq, 32] of an attention output against `r` (a dict of softmax_attention) and v [nk, 32].
    Every weight p_k reaches the output as p_k (1 + eps_k) with
      eps_k <= n_dot E32 sabs_k             the score's own rounding, through e^x (d e^x = e^x dx)
             + 2^-16 sabs_k                  pair mode: q_lo k_lo, the product of the four that is not formed (|lo| <= 2^-8 |hi| each)
             + E32 (s_max - s_k)             the subtractions s - m along the chain of running maxima telescope to s_max - s_k
             + n_steps (EXP_ULP + E32)       an expf and a product per factor
    normalised weights move by at most e^(2 eps) - 1 (numerator and denominator): |d out| <= sum_k p_k (e^(2 eps_k) - 1) (|v_k| + |out|).
    P is rounded to the storage format before the second MFMA while the row sum uses the unrounded P, so that rounding enters once: U_OUT sum_k p_k
    |v_k| in the single-pass modes; a pair: 2^-16 for its rounding + 2^-16 for p_lo v_lo, the product that is not formed.  A weight below the normal
    range of its format is flushed or rounded absolutely: F32_MIN sum_k |v_k| for expf's underflow, in f16 2^-25 sum_k |v_k| for P's rounding
    (the row sum is >= 1: the largest weight is exactly 1).  Then n_acc E32 (pav + |out|) for the two fp32 sums and the division, U_OUT |out| for
    the store; f16: + 2^-25 for a subnormal store."""
    ndot, n_steps, n_acc = attention_counts(v.shape[0], mode)
    s, p, sabs, out, pav = r["s"], r["p"], r["sabs"], r["out"], r["pav"]
    eps = ndot * E32 * sabs + E32 * (s.max(-1, keepdim=True).values - s).clamp(max=200.0) + n_steps * (EXP_ULP + E32)
    if mode == "bf16x3":
        eps = eps + 2.0 ** -16 * sabs
    grow = torch.expm1(2 * eps)
    va = v.double().abs()
    tol = (p * grow) @ va + (p * grow).sum(-1, keepdim=True) * out.abs()
    tol = tol + (2.0 ** -15 if mode == "bf16x3" else U_OUT[mode]) * pav + F32_MIN * va.sum(0, keepdim=True)
    if mode == "f16":
        tol = tol + 2.0 ** -25 * va.sum(0, keepdim=True) + 2.0 ** -25
    return tol + n_acc * E32 * (pav + out.abs()) + U_OUT[mode] * out.abs()


# One score pattern per head, so every launch carries all of them:
HEAD_PATTERNS = ("random", "dominant0", "dominant31", "dominant32", "dominant_last", "equal", "spread", "wide")
DOMINANCE = 20.0
SCORE_STD = 1.3                       # of the random head: what the model's eight attention layers show


def seam_marks(n):
    """where the four dominant keys sit: key 0, the end of the first tile, the start of the second, the last key -- clamped to the table"""
    return (0, min(31, n - 1), min(32, n - 1), n - 1)


def _unit(g, *shape):
    u = torch.randn(*shape, DK, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def make_table(n, g, shift):
    """q, k, v [n, 8, 32] float64 (before rounding) of one table of n cells.  random: q ~ N(0, 1), k ~ N(0, 1.3), scores of std 1.3.  Heads
    dominant*: key seam_marks(n)[i] is 4 u, every other key has its u component removed, the queries look along u with a score of 32 .. 38 on
    the planted key.  equal: q = 0.  spread: k = (a sqrt(32) / 8) u + noise with a uniform in +-80 and one key at exactly 80, q = 8 u.  wide: three
    times random.  v ~ N(shift, 1)."""
    marks = seam_marks(n)
    u = _unit(g, HEADS)
    q = torch.randn(n, HEADS, DK, generator=g, dtype=torch.float64)
    k = SCORE_STD * torch.randn(n, HEADS, DK, generator=g, dtype=torch.float64)
    v = torch.randn(n, HEADS, DK, generator=g, dtype=torch.float64) + shift
    for h in range(1, 5):
        k[:, h] -= (k[:, h] @ u[h])[:, None] * u[h]
        k[marks[h - 1], h] = 4.0 * u[h]
        top = 32 + 6 * torch.rand(n, generator=g, dtype=torch.float64)
        q[:, h] = 0.3 * q[:, h] + (top * SCALE / 4.0)[:, None] * u[h]
    q[:, 5] = 0
    a = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * 80.0
    if n > 1:
        a[int(torch.randint(0, n, (1,), generator=g))] = 80.0
    k[:, 6] = 0.05 * k[:, 6] + (a * SCALE / 8.0)[:, None] * u[6]
    q[:, 6] = 0.02 * q[:, 6] + 8.0 * u[6]
    q[:, 7] *= 3.0
    return q, k, v


# the GPU test's attention cases: single tables around the 32-key tile, a long one, the largest a table can be, and a batch with a zero count in
# the middle, unaligned first tokens and neighbours on both sides
ATTN_CASES = [[1], [2], [31], [32], [33], [63], [64], [65], [97], [700], [MAX_CELLS], [33, 0, 1, 64, 31, 200]]


def attn_seed(counts):
    return 1000 + sum(counts) + 7 * len(counts)


def attention_case(counts, mode, seed=None):
    """qkv [N, 768] float64 as stored in `mode` (token rows [q 256 | k 256 | v 256], head h at 32 h) of tables with different data"""
    g = torch.Generator().manual_seed(attn_seed(counts) if seed is None else seed)
    rows = []
    for t, c in enumerate(counts):
        if c:
            q, k, v = make_table(c, g, 0.5 * (t - 1))
            rows.append(torch.cat([q.reshape(c, D), k.reshape(c, D), v.reshape(c, D)], 1))
    return rnd(torch.cat(rows, 0), mode)


def table_rows(counts):
    """[(first token, cells)] per table"""
    out, n = [], 0
    for c in counts:
        out.append((n, c))
        n += c
    return out


def attention_reference(rows):
    """token rows [c, 768] of ONE table -> per head (dict of softmax_attention, v_h)"""
    c = rows.shape[0]
    q, k, v = (rows[:, i * D:(i + 1) * D].reshape(c, HEADS, DK) for i in range(3))
    return [(softmax_attention(q[:, h], k[:, h], v[:, h]), v[:, h]) for h in range(HEADS)]


def reference_out_tol(ref, mode):
    """-> (out [c, 256], tol [c, 256]) of attention_reference's result"""
    c = ref[0][0]["out"].shape[0]
    return (torch.stack([r["out"] for r, _ in ref], 1).reshape(c, D), torch.stack([attention_tol(r, v, mode) for r, v in ref], 1).reshape(c, D))


def check_patterns(ref, n):
    """the generator's promises, read off the reference's own scores: the random head's scores have a std near 1.3, a planted key leads by >= DOMINANCE,
    `equal` is flat, `spread` spans > 100 and reaches fp32's underflow (e^-104 < 2^-126 needs a span > 87.4)"""
    marks = seam_marks(n)
    if n >= 64:
        assert 1.0 <= float(ref[0][0]["s"].std()) <= 1.6, float(ref[0][0]["s"].std())
    for h in range(1, 5):
        s = ref[h][0]["s"]
        if n > 1:
            rest = s.clone()
            rest[:, marks[h - 1]] = -math.inf
            lead = float((s[:, marks[h - 1]] - rest.max(-1).values).min())
            assert lead >= DOMINANCE, (h, lead)
    assert float(ref[5][0]["s"].abs().max()) == 0.0
    if n >= 16:
        span = ref[6][0]["s"].max(-1).values - ref[6][0]["s"].min(-1).values
        assert float(span.min()) > 100.0, float(span.min())


# ---- norm ----------------------------------------------------------------------------------------------------------------------------------------
NORM_ROWS = (1, 3, 4, 5, 129)                   # four tokens per workgroup
NORM_KINDS = ("random", "mean1000", "constant", "tiny", "outlier")
CONSTANT = 2.5                                   # every partial sum of 256 copies is exact in fp32, so mean == x and the row normalises to exactly bias


def norm_case(rows, seed):
    """x fp32 [rows, 256] with the row kinds in turn, alpha / bias fp32 [256] away from 1 and 0.  random: N(0.3, 2); mean1000: N(1000, 1);
    constant: 2.5; tiny: N(0, 1e-7), where eps = 1e-6 decides the result; outlier: N(0, 1) with one element of 1e4."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g, dtype=torch.float64)
    kinds = [NORM_KINDS[i % len(NORM_KINDS)] for i in range(rows)]
    for i, kd in enumerate(kinds):
        if kd == "random":
            x[i] = 2 * x[i] + 0.3
        elif kd == "mean1000":
            x[i] += 1000.0
        elif kd == "constant":
            x[i] = CONSTANT
        elif kd == "tiny":
            x[i] *= 1e-7
        else:
            x[i, (37 * i) % D] = 1e4
    alpha = (1.0 + 0.5 * torch.randn(D, generator=g, dtype=torch.float64)).float()
    bias = (0.7 * torch.randn(D, generator=g, dtype=torch.float64)).float()
    return x.float(), alpha, bias, kinds


def norm_reference(x, alpha, bias):
    x, alpha, bias = x.double(), alpha.double(), bias.double()
    d = x - x.mean(-1, keepdim=True)
    std = ((d * d).sum(-1, keepdim=True) / (D - 1)).sqrt()
    return alpha * d / (std + EPS) + bias


def norm_tol(x, alpha, bias, mode):
    """Bound on norm_kernel's output against norm_reference, following the kernel's order of operations:
      mean   4 values in the lane + 6 butterfly steps + 1 division = 10 roundings of a sum whose magnitudes total sum|x|: dm = 10 E32 mean|x|
      d      one subtraction from that mean: dd = E32 |d| + dm
      q      sum of d^2: each term moves by dd (2 |d| + dd); products and the 9 additions of positive terms: 10 E32 more
      std    sqrt(q / 255): through the square root (lower side, the larger one), + a division and a sqrtf (EXP_ULP each)
      den    std + eps: one addition
      t      alpha d / den: d / den moves by dd / den + |d| dden / den^2 (den taken at its low end), then a product (E32) and a division (EXP_ULP)
      out    t + bias: one addition, then the store (U_OUT; f16: + 2^-25)."""
    x, alpha, bias = x.double(), alpha.double(), bias.double()
    d = x - x.mean(-1, keepdim=True)
    q = (d * d).sum(-1, keepdim=True)
    std = (q / (D - 1)).sqrt()
    den = std + EPS
    dm = 10 * E32 * x.abs().mean(-1, keepdim=True)
    dd = E32 * d.abs() + dm
    dq = (dd * (2 * d.abs() + dd)).sum(-1, keepdim=True)
    dq = dq + 10 * E32 * (q + dq)
    dstd = std - ((q - dq).clamp(min=0.0) / (D - 1)).sqrt() + 2 * EXP_ULP * std
    dden = dstd + E32 * den
    den_lo = den - dden
    assert bool((den_lo > 0).all())
    t = alpha * d / den
    dt = alpha.abs() * (dd / den_lo + d.abs() * dden / (den * den_lo)) + (E32 + EXP_ULP) * t.abs()
    out = t + bias
    return dt + E32 * out.abs() + U_OUT[mode] * out.abs() + (2.0 ** -25 if mode == "f16" else 0.0)


# ---- token preparation ---------------------------------------------------------------------------------------------------------------------------
TOK_COUNTS = [5, 0, 130]                        # N = 135, Npad = 256
# around every decision point of clamp(trunc(x), 0, 255): the sign change, a tie that rounds down and one that rounds up, the upper clamp, far outside
PLANTED = (-1.0, -0.5, 0.0, 10.5, 11.5, 254.999, 255.0, 255.9, 256.0, 300.0, 1e6)


def tok_index(d):
    """the reference's index of a coordinate: int32 cast (truncation), then clamp to [0, 255]"""
    return d.to(torch.int32).to(torch.int64).clamp(0, 255)


def tok_case(seed):
    """logi fp32 [3, 3000, 256], dets fp32 [3, 3000, 9], x_pe / y_pe fp32 [256, 256].  Rows at and beyond a table's count are NaN in logi and dets, the
    columns of dets that the operation does not read (3, 4, 6, 7, 8) are NaN everywhere; the planted coordinates appear in each of the columns read."""
    g = torch.Generator().manual_seed(seed)
    nt = len(TOK_COUNTS)
    logi = torch.full((nt, MAX_CELLS, D), float("nan"))
    dets = torch.full((nt, MAX_CELLS, 9), float("nan"))
    planted = torch.tensor(PLANTED, dtype=torch.float32)
    for t, c in enumerate(TOK_COUNTS):
        logi[t, :c] = torch.randn(c, D, generator=g)
        for j, col in enumerate((0, 1, 2, 5)):
            vals = torch.rand(c, generator=g) * 300 - 20
            idx = (torch.arange(c) + 3 * j) % (len(PLANTED) + 2)
            vals = torch.where(idx < len(PLANTED), planted[idx.clamp(max=len(PLANTED) - 1)], vals)
            dets[t, :c, col] = vals
    x_pe = torch.randn(256, D, generator=g)
    y_pe = torch.randn(256, D, generator=g)
    return logi, dets, x_pe, y_pe


def tok_reference(logi, dets, counts, x_pe, y_pe, use_pe, index=tok_index):
    """-> (x [N, 256] float64, tol without the store: four fp32 additions of a sum whose magnitudes total `mag`)"""
    xs, mags = [], []
    for t, c in enumerate(counts):
        x = logi[t, :c].double()
        mag = x.abs()
        if use_pe:
            for tab, col in ((x_pe, 0), (y_pe, 1), (x_pe, 2), (y_pe, 5)):
                e = tab.double()[index(dets[t, :c, col])]
                x = x + e
                mag = mag + e.abs()
        xs.append(x)
        mags.append(mag)
    return torch.cat(xs, 0), 4 * E32 * torch.cat(mags, 0)


def store_tol(x, mode):
    return U_OUT[mode] * x.abs() + (2.0 ** -25 if mode == "f16" else 0.0)
