"""Plain float64 references of the MtlTabNet decoders' attention kernels (csrc/mtl_decoder.hip), with the error bounds the GPU tests assert and the
operand generators both suites share.  No GPU, no engine: tests/test_mtl_attn_host.py ties every function here to something independent (the oracle's
own attention, torch.softmax in float64), tests/test_gpu_mtl_attn.py compares the kernels with them.

The operations, as the reference model defines them (master_decoder.py:57-96, 117-144, 264-278; restated in oracle/mtl_tabnet.py::_mha):
  source attention  out[q, head] = softmax_k(q_head . k_head[k]) v_head[k] over the hw keys of the query's table, d = 512 = 8 heads of 64.  The keys are
                    stored already divided by sqrt(64) = 8 (the reference scales the KEYS, :65), so no scale appears here.
  self attention    the same over positions 0 .. p of the query's own sequence; a query whose own token is <PAD> has every score replaced by -6.55e4
                    (make_mask masks the query ROW), i.e. attends with equal weights to all Lcur positions of the prefix, later ones included.
  e4m3 copy         byte = e4m3(clamp(8 x, -448, 448)), round to nearest even (OCP e4m3fn: 4 exponent bits, 3 mantissa bits, largest value 448).

Storage formats: "bf16" / "f16" single pass, "bf16x3" = (hi | lo) bf16 pairs.  Error bounds (every constant derived here, none fitted to a kernel):
  U_OUT   one round-to-nearest store, relative to the value: 2^-8 for bf16 (8 significant bits), 2^-11 for f16 (11 bits); a (hi | lo) pair stores
          hi = bf16(x) and lo = bf16(x - hi) with |x - hi| <= 2^-8 |x|, so |x - hi - lo| <= 2^-8 2^-8 |x| = 2^-16 |x|.  f16 only: below 2^-14 the format
          is subnormal with spacing 2^-24, so a store is off by up to 2^-25 absolute whatever the value.
  E32     fp32 unit round-off 2^-24: n dependent fp32 operations on a sum are off by at most n 2^-24 of the sum of magnitudes (first order).
  EXP_ULP expf of the HIP device library is documented at 1 ulp = 2^-23 relative.
"""
import math

import torch

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
U_OUT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "bf16x3": 2.0 ** -16}
E32 = 2.0 ** -24
EXP_ULP = 2.0 ** -23
HEADS, DK, D, NL = 8, 64, 512, 5
KVC = NL * 2 * D
KV8_SCALE = 8.0
PAD_SCORE = -6.55e4
STREAM, STREAM8, MFMA = 0, 1, 2          # lib.PT_MTL_ATTN_*


def fmt_of(mode):
    return "f16" if mode == "f16" else "bf16"


def rnd(x, mode):
    """float64 values -> the float64 values one store in `mode` holds (a pair holds hi + lo)"""
    if mode != "bf16x3":
        return x.to(DT[mode]).double()
    hi = x.to(torch.bfloat16)
    return hi.double() + (x.double() - hi.double()).to(torch.bfloat16).double()


def split_pair(x):
    hi = x.to(torch.bfloat16)
    return hi, (x.double() - hi.double()).to(torch.bfloat16)


# ---- the operations ------------------------------------------------------------------------------------------------------------------------------
def softmax_attention(q, k, v):
    """q [nq, 64], k / v [nk, 64] float64 (k pre-scaled) -> dict: out [nq, 64], s scores [nq, nk], p normalised weights, pav = sum_k p |v|,
    sabs[q, k] = sum_j |q_j k_j| (what a rounding of the dot product is relative to)"""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.t()
    p = torch.softmax(s, -1)
    return dict(out=p @ v, s=s, p=p, pav=p @ v.abs(), sabs=q.abs() @ k.abs().t())


def self_attention_row(q, k, v, p, is_pad):
    """one query at position p of a sequence whose cache holds Lcur = len(k) positions: scores of keys > p are replaced by PAD_SCORE as the
    causal mask does, ALL scores when the query's token is <PAD> (make_mask); soft-max over all Lcur positions like the reference"""
    s = (k.double() @ q.double())
    keep = torch.arange(len(k)) <= p
    if is_pad:
        keep = torch.zeros_like(keep)
    sm = torch.where(keep, s, torch.full_like(s, PAD_SCORE))
    w = torch.softmax(sm, -1)
    return dict(out=w @ v.double(), s=sm, p=w, pav=w @ v.double().abs(), sabs=(k.double().abs() @ q.double().abs()))


def e4m3_bytes(x):
    """float values -> uint8 e4m3 patterns of 8 x, saturating at +-448, round to nearest even"""
    y = (x.float() * KV8_SCALE).clamp(-448.0, 448.0)
    if hasattr(torch, "float8_e4m3fn"):
        return y.to(torch.float8_e4m3fn).view(torch.uint8)
    return _e4m3_by_hand(y)


def _e4m3_by_hand(y):
    """e4m3fn of values already within +-448: exponent bias 7, subnormal spacing 2^-9, ties to even"""
    y = y.double()
    a = y.abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -20))).clamp(-6, 8)            # binade of a normal value; everything below 2^-6 shares spacing 2^-9
    step = 2.0 ** (e - 3)
    r = torch.round(a / step) * step                                                # torch.round: half to even
    e2 = torch.floor(torch.log2(r.clamp_min(2.0 ** -20))).clamp(-6, 8)
    man = torch.where(r < 2.0 ** -6, r / 2.0 ** -9, (r / 2.0 ** e2 - 1.0) * 8)
    byte = torch.where(r < 2.0 ** -6, man, (e2 + 7) * 8 + man).to(torch.uint8)
    sign = (torch.signbit(y)).to(torch.uint8) * 128
    return byte | sign


def e4m3_decode(b):
    """uint8 e4m3 patterns -> float64 values of the scaled copy (8 x)"""
    if hasattr(torch, "float8_e4m3fn"):
        return b.view(torch.float8_e4m3fn).double()
    b = b.to(torch.int64)
    e, m = (b >> 3) & 15, (b & 7).double()
    val = torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e.double() - 7))
    return torch.where((b & 128) != 0, -val, val)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------
def shape_counts(kind, keys_in_slice, nsplit):
    """(n_dot, n_steps, n_acc): dependent fp32 operations of a kernel, from its loop structure.
    n_dot: additions behind one score.  stream: 8 fused multiply-adds in the lane + 3 butterfly steps = 11; stream8: 16 + 2 = 18; mfma: 64 products
      accumulated by the matrix pipe in an order we do not assume = 64; self: as stream.
    n_steps: factors e^(m_old - m_new) a weight passes through: at most one per chunk of its slice (64 keys; 128 stream8; 32 mfma), one at the stream
      merge (none in mfma), one at the slice merge; each costs an expf (EXP_ULP), a subtraction and a product (E32 each).
    n_acc: additions behind one output sum: the keys one accumulator walks (a slice's keys over 8 streams; 16 in stream8; every key in mfma, whose
      MFMA adds 16 products per step in an unknown order), + n_steps rescalings, + 3 (4) butterfly additions, + 2 nsplit for the slice merge's
      multiply-adds, + 1 division."""
    chunk, streams, ndot, merge = {"stream": (64, 8, 11, 3), "self": (64, 8, 11, 3), "stream8": (128, 16, 18, 4), "mfma": (32, 1, 64, 1)}[kind]
    chunks = -(-keys_in_slice // chunk)
    n_steps = chunks + (0 if kind == "mfma" else 1) + (1 if nsplit > 1 else 0)
    n_acc = -(-keys_in_slice // streams) + n_steps + merge + (2 * nsplit if nsplit > 1 else 0) + 1
    return ndot, n_steps, n_acc


def attention_tol(r, v, kind, mode, keys_in_slice, nsplit, x3_products=False):
    """Tolerance [nq, 64] of an attention output against `r` (a dict of softmax_attention / self_attention_row stacked to [nq, nk]) and v [nk, 64].
    Every weight p_k reaches the output as p_k (1 + eps_k) with
      eps_k <= n_dot E32 sabs_k                     the score's own rounding, through e^x (d e^x = e^x dx)
             + 2^-16 sabs_k                          mfma in the pair mode only: q_lo k_lo is the product of the three that is not formed
             + E32 (s_max - s_k)                     the subtractions s - m along the chain of running maxima telescope to s_max - s_k
             + n_steps (EXP_ULP + E32)               an expf and a product per factor
             + u_p                                   mfma only: P is rounded to the storage format before the second MFMA.  Set to 2^-9 for bf16 (the
                                                     mean magnitude of a bf16 rounding; its largest is 2^-8), 2^-12 for f16 likewise; a pair: 2^-16 for its
                                                     rounding + 2^-16 for p_lo v_lo, the product of the three that is not formed = 2^-15.
    normalised weights move by at most e^(2 eps) - 1 (numerator and denominator), so |d out| <= sum_k p_k (e^(2 eps_k) - 1) (|v_k| + |out|) ...
    the P rounding excepted: the row sum l uses the unrounded P, so u_p enters once: u_p sum_k p_k |v_k|.
    Then n_acc E32 (pav + |out|) for the two fp32 sums and the division, U_OUT |out| for the store; f16: + 2^-25 for a subnormal store and, in
    mfma, 2^-25 sum_k |v_k| for weights below f16's normal range (l >= 1: the largest weight is exactly 1)."""
    ndot, n_steps, n_acc = shape_counts(kind, keys_in_slice, nsplit)
    s, p, sabs, out, pav = r["s"], r["p"], r["sabs"], r["out"], r["pav"]
    eps = ndot * E32 * sabs + E32 * (s.max(-1, keepdim=True).values - s).clamp(max=200.0) + n_steps * (EXP_ULP + E32)
    if kind == "mfma" and x3_products:
        eps = eps + 2.0 ** -16 * sabs
    grow = torch.expm1(2 * eps)
    va = v.double().abs()
    tol = (p * grow) @ va + (p * grow).sum(-1, keepdim=True) * out.abs()
    if kind == "mfma":
        tol = tol + {"bf16": 2.0 ** -9, "f16": 2.0 ** -12, "bf16x3": 2.0 ** -15}[mode] * pav
        if mode == "f16":
            tol = tol + 2.0 ** -25 * va.sum(0, keepdim=True)
    tol = tol + n_acc * E32 * (pav + out.abs()) + U_OUT[mode] * out.abs()
    if mode == "f16":
        tol = tol + 2.0 ** -25
    return tol


def split_agreement_tol(r, v, kind, keys_a, keys_b, nsplit_b):
    """bound on |out(nsplit = 1) - out(nsplit > 1)| BEFORE the store: both are within their fp32 terms of the exact value"""
    def fp32_terms(keys, ns):
        ndot, n_steps, n_acc = shape_counts(kind, keys, ns)
        s, p, sabs, out, pav = r["s"], r["p"], r["sabs"], r["out"], r["pav"]
        eps = ndot * E32 * sabs + E32 * (s.max(-1, keepdim=True).values - s).clamp(max=200.0) + n_steps * (EXP_ULP + E32)
        grow = torch.expm1(2 * eps)
        return (p * grow) @ v.double().abs() + (p * grow).sum(-1, keepdim=True) * out.abs() + n_acc * E32 * (pav + out.abs())
    return fp32_terms(keys_a, 1) + fp32_terms(keys_b, nsplit_b)


# ---- operand generators ---------------------------------------------------------------------------------------------------------------------
# One score pattern per head, so every launch carries all of them:
HEAD_PATTERNS = ("random", "dominant0", "dominant1", "dominant2", "dominant3", "equal", "spread", "wide")
DOMINANCE = 20.0


def _unit(g, *shape):
    u = torch.randn(*shape, DK, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def make_keys_values(nk, marks, g, shift):
    """k, v [nk, 8, 64] float64 (before rounding) + the planted directions u [8, 64].  Heads dominant0..3: key marks[i] is 4 u, every other key
    has its u component removed; `spread`: k = (a / 8) u + noise with a uniform in +-80; the others: N(0, 0.35).  v ~ N(shift, 1)."""
    u = _unit(g, HEADS)
    k = 0.35 * torch.randn(nk, HEADS, DK, generator=g, dtype=torch.float64)
    v = torch.randn(nk, HEADS, DK, generator=g, dtype=torch.float64) + shift
    for h in range(1, 5):
        k[:, h] -= (k[:, h] @ u[h])[:, None] * u[h]
        k[marks[h - 1], h] = 4.0 * u[h]
    a = (torch.rand(nk, generator=g, dtype=torch.float64) * 2 - 1) * 80.0
    if nk > 1:
        a[int(torch.randint(0, nk, (1,), generator=g))] = 80.0
    k[:, 6] = 0.05 * k[:, 6] + (a / 8.0)[:, None] * u[6]
    return k, v, u


def make_queries(nq, u, g):
    """q [nq, 8, 64] for keys of make_keys_values: dominant heads look along u with a score of 32 .. 38 on the planted key, `equal` is 0 (every
    score equal), `spread` is 8 u, `wide` three times `random`"""
    q = torch.randn(nq, HEADS, DK, generator=g, dtype=torch.float64)
    for h in range(1, 5):
        top = 32 + 6 * torch.rand(nq, generator=g, dtype=torch.float64)
        q[:, h] = 0.3 * q[:, h] + (top / 4.0)[:, None] * u[h]
    q[:, 5] = 0
    q[:, 6] = 0.02 * q[:, 6] + 8.0 * u[6]
    q[:, 7] *= 3.0
    return q


def seam_marks(hw, chunk, keys_per_split, nsplit):
    """the four places a dominant key is planted: key 0, the last key of the first chunk, the first key of the last slice, key hw - 1"""
    return (0, min(chunk, hw) - 1, (nsplit - 1) * keys_per_split, hw - 1)


def cross_case(n_tables, hw, slots, marks, mode, seed):
    """kv [n_tables * hw, 5120] float64 as stored in `mode` (k of slot l at channel 1024 l, v at 1024 l + 512; planted slots `slots`, every other
    channel N(0, 1)) and u[slot][table] for make_queries"""
    g = torch.Generator().manual_seed(seed)
    kv = torch.randn(n_tables, hw, KVC, generator=g, dtype=torch.float64)
    us = {}
    for sl in slots:
        us[sl] = []
        for b in range(n_tables):
            k, v, u = make_keys_values(hw, marks, g, float(b - 1) + 0.25 * sl)
            kv[b, :, sl * 2 * D:sl * 2 * D + D] = k.reshape(hw, D)
            kv[b, :, sl * 2 * D + D:(sl + 1) * 2 * D] = v.reshape(hw, D)
            us[sl].append(u)
    return rnd(kv.reshape(n_tables * hw, KVC), mode), us


def cross_reference(q_rows, kv, hw, table, slot):
    """q_rows [nq, 512] and the kv tensor as stored -> per head h the dict of softmax_attention over the keys of `table` at `slot`, and v_h"""
    kb = kv[table * hw:(table + 1) * hw, slot * 2 * D:slot * 2 * D + D].reshape(hw, HEADS, DK)
    vb = kv[table * hw:(table + 1) * hw, slot * 2 * D + D:(slot + 1) * 2 * D].reshape(hw, HEADS, DK)
    qh = q_rows.reshape(-1, HEADS, DK)
    return [(softmax_attention(qh[:, h], kb[:, h], vb[:, h]), vb[:, h]) for h in range(HEADS)]


def check_patterns(refs, marks):
    """the generator's promises, read off the reference's own scores: the planted key leads by >= DOMINANCE, `equal` is flat, `spread` spans > 100"""
    for h in range(1, 5):
        s = refs[h][0]["s"]
        top = s[:, marks[h - 1]]
        rest = s.clone()
        rest[:, marks[h - 1]] = -math.inf
        if s.shape[1] > 1:
            assert float((top - rest.max(-1).values).min()) >= DOMINANCE, (h, float((top - rest.max(-1).values).min()))
    assert float(refs[5][0]["s"].abs().max()) == 0.0
    if refs[6][0]["s"].shape[1] >= 16:
        assert float((refs[6][0]["s"].max(-1).values - refs[6][0]["s"].min(-1).values).min()) > 100.0


def self_case(L, M, Mp, mode, seed, pad):
    """cache [L, Mp, 1536] float64 as stored (q | k | v of position p, sequence s; k pre-scaled), tok int64 [L, Mp].  Sequence 1 holds <PAD> at the
    interior position L // 2, sequence 2 at the last position.  Head patterns as in the source attention with the planted keys at positions 0,
    min(63, L - 1), L // 2 and L - 1."""
    g = torch.Generator().manual_seed(seed)
    cache = torch.randn(L, Mp, 3 * D, generator=g, dtype=torch.float64)
    marks = (0, min(64, L) - 1, L // 2, L - 1)
    for s in range(M):
        k, v, u = make_keys_values(L, marks, g, float(s - 1))
        q = make_queries(L, u, g)
        cache[:, s, :D] = q.reshape(L, D)
        cache[:, s, D:2 * D] = k.reshape(L, D)
        cache[:, s, 2 * D:] = v.reshape(L, D)
    tok = torch.randint(0, 40, (L, Mp), generator=g)
    tok[tok == pad] = pad + 1
    if M > 1 and L > 2:
        tok[L // 2, 1] = pad
    if M > 2 and L > 1:
        tok[L - 1, 2] = pad
    return rnd(cache, mode), tok


def self_reference(cache, tok, pad, p, s):
    """position p of sequence s -> per head (dict of self_attention_row with [1, L] shapes, v_h)"""
    L = cache.shape[0]
    q = cache[p, s, :D].reshape(HEADS, DK)
    k = cache[:, s, D:2 * D].reshape(L, HEADS, DK)
    v = cache[:, s, 2 * D:].reshape(L, HEADS, DK)
    out = []
    for h in range(HEADS):
        r = self_attention_row(q[h], k[:, h], v[:, h], p, int(tok[p, s]) == pad)
        out.append(({key: val[None] for key, val in r.items()}, v[:, h]))
    return out
