"""The Lore processor's kernels (csrc/lore_processor.hip) one at a time, through pt_op_lore_tok_prepare / norm / cvt_logic / attention / scatter4 -- the
launch helpers and the token / tile map builder of pt_tsr_process -- against the float64 references of tests/lore_proc_ref.py (tied to the oracle, and
shown to separate wrong variants, by tests/test_lore_proc_ref_host.py).  One engine per mode with no model loaded.  Then whole calls of pt_tsr_process
at the seams of the 32-key tile and of the cell limit, column by column against the oracle.

Every operand is generated already on the storage grid of the mode, so the reference reads what the kernel reads; outputs start as a sentinel that is
exact in every format; the bounds are stated with the references; every test prints its worst error / tolerance ratio.

Worst error / tolerance measured on an MI355X when the tests were written (bf16, f16, BF16X3; in the single-pass modes the store's half-ulp is most of
the bound of the element-wise kernels, so a correct kernel sits just under 1 there): attention 0.715 / 0.663 / 0.103 (at 3000 keys 0.588 / 0.356 /
0.026: the accumulation term grows with the key count, the errors do not); norm 0.982 / 0.994 / 0.483; token preparation 0.995 / 0.997 / 0.490;
cvt_logic, scatter4 and the parameter-free norm are bit-exact.  Whole calls in BF16X3: worst column 7.3e-05 of the 1e-3 allowed.  No kernel
needed a change.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lore_proc_ref as R  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MODES = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "bf16x3": L.PT_PRECISION_BF16X3}
ALL = list(MODES)
SENTINEL = 7.5                       # exact in bf16 and f16
TOL_REL = 1e-3                       # whole calls in BF16X3: as tests/test_gpu_tsr.py


class Mode:
    def __init__(self, name, eng):
        self.name, self.eng = name, eng
        self.split = name == "bf16x3"
        self.dt = R.DT[R.fmt_of(name)]
        self.m = 2 if self.split else 1

    def put(self, v):
        """float64 values [.., C] already on the mode's grid -> the tensor that holds them ([hi C | lo C] when split), on the host"""
        if not self.split:
            t = v.to(self.dt)
            assert torch.equal(t.double(), v)
            return t.contiguous()
        hi, lo = R.split_pair(v)
        assert torch.equal(hi.double() + lo.double(), v)
        return torch.cat([hi, lo], -1).contiguous()

    def encode(self, v32):
        """fp32 values [.., C] -> what a store of exactly these values leaves: round to nearest even, lo = the rounded rest"""
        hi = v32.to(self.dt)
        return torch.cat([hi, (v32 - hi.float()).to(self.dt)], -1) if self.split else hi

    def blank(self, *shape):
        return torch.full(shape[:-1] + (shape[-1] * self.m,), SENTINEL, dtype=self.dt, device=DEV)

    def halves(self, raw):
        c = raw.shape[-1] // self.m
        return [raw[..., i * c:(i + 1) * c] for i in range(self.m)]

    def get(self, raw):
        """host tensor as stored -> float64 values; every stored value must be finite"""
        assert bool(torch.isfinite(raw.float()).all()), "Inf / NaN stored"
        return sum(h.double() for h in self.halves(raw))

    def is_sentinel(self, raw):
        return bool((raw.float() == SENTINEL).all())


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
        pytest.exit(f"device error after a Lore processor op test, not continuing: {e}", returncode=3)


def _ratio(what, got, ref, tol):
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    i = int(r.flatten().argmax())
    worst = float(r.flatten()[i])
    assert worst <= 1.0, (f"{what}: {int((r > 1).sum())} of {r.numel()} values out of tolerance, worst err/tol {worst:.3f} "
                          f"(err {float(err.flatten()[i]):.3e} at ref {float(ref.flatten()[i]):.5g}, row {i // ref.shape[-1]}, column {i % ref.shape[-1]})")
    return worst


# ---- attention -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("case", range(len(R.ATTN_CASES)), ids=["-".join(map(str, c)) for c in R.ATTN_CASES])
def test_attention_against_fp64(engines, case, name):
    """attention_kernel<SPLIT> over the production tile list: every table against its own float64 reference, all eight score patterns per launch.
    Rows [N, Npad) of qkv are NaN: the kernel never reads them (every stored value is finite) and leaves their output rows alone."""
    m = engines(name)
    counts = R.ATTN_CASES[case]
    N = sum(counts)
    Npad = R.npad_of(N)
    vals = R.attention_case(counts, name)
    qkv = torch.full((Npad, 3 * R.D * m.m), float("nan"), dtype=m.dt)
    qkv[:N] = m.put(vals)
    out = m.blank(Npad, R.D)
    tiles = m.eng.op_lore_attention(qkv.to(DEV), counts, out, split=m.split)
    torch.cuda.synchronize()
    want_tiles = [(t0, q0, c) for t0, c in R.table_rows(counts) for q0 in range(0, c, 32)]
    assert tiles.cpu().tolist() == [list(t) for t in want_tiles]
    raw = out.cpu()
    assert m.is_sentinel(raw[N:]), "rows past the last token were written"
    got = m.get(raw[:N])
    worst = 0.0
    for t, (t0, c) in enumerate(R.table_rows(counts)):
        if c:
            ref = R.attention_reference(vals[t0:t0 + c])
            R.check_patterns(ref, c)
            want, tol = R.reference_out_tol(ref, name)
            worst = max(worst, _ratio(f"attention {counts} table {t} [{name}]", got[t0:t0 + c], want, tol))
    print(f"lore attention {counts} [{name}]: worst err/tol {worst:.3f}")


# ---- norm ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("rows", R.NORM_ROWS)
def test_norm_against_fp64(engines, rows, name):
    """norm_kernel, four tokens per workgroup: random rows, mean 1000 with std 1, a constant row (exactly bias), std 1e-7 (eps decides), one outlier;
    alpha and bias away from 1 and 0.  Rows past `rows` keep the sentinel."""
    m = engines(name)
    x, alpha, bias, kinds = R.norm_case(rows, rows)
    out = m.blank(rows + 3, R.D)
    m.eng.op_lore_norm(x.to(DEV), alpha.to(DEV), bias.to(DEV), out, split=m.split)
    torch.cuda.synchronize()
    raw = out.cpu()
    assert m.is_sentinel(raw[rows:]), "rows past the last were written"
    worst = _ratio(f"norm rows={rows} [{name}]", m.get(raw[:rows]), R.norm_reference(x, alpha, bias), R.norm_tol(x, alpha, bias, name))
    for i, kd in enumerate(kinds):
        if kd == "constant":
            assert torch.equal(raw[i], m.encode(bias)), f"constant row {i}: not exactly bias"
    print(f"lore norm rows={rows} [{name}]: worst err/tol {worst:.3f}")


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("rows", (5, 129))
def test_norm_without_parameters_is_the_conversion(engines, rows, name):
    """alpha == null: the fp32 value rounded to the format, bit for bit -- hi and lo halves in BF16X3"""
    m = engines(name)
    x = R.norm_case(rows, 50 + rows)[0]
    out = m.blank(rows + 3, R.D)
    m.eng.op_lore_norm(x.to(DEV), None, None, out, split=m.split)
    torch.cuda.synchronize()
    raw = out.cpu()
    assert m.is_sentinel(raw[rows:]) and torch.equal(raw[:rows], m.encode(x))


# ---- token preparation -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _tok_case():
    return R.tok_case(5)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("use_pe", [False, True])
def test_token_preparation_against_fp64(engines, use_pe, name):
    """tok_prepare_kernel over counts [5, 0, 130] (Npad 256): coordinates planted around every decision point of the index, NaN in the columns of dets
    that are not read and in every row at and beyond a table's count.  Rows below N: the float64 sum within four fp32 roundings plus the store (no
    position embeddings: the conversion of logi, bit for bit, lo halves included); rows [N, Npad) exactly 0 in x0 and in cat[:, 256:512]; cat[:, 0:256]
    untouched; in BF16X3 the sum hi + lo is held to the pair's 2^-16 and no lo exceeds half an ulp of its hi."""
    m = engines(name)
    logi, dets, x_pe, y_pe = _tok_case()
    counts = R.TOK_COUNTS
    N, Npad = sum(counts), R.npad_of(sum(counts))
    x0, cat = m.blank(Npad, R.D), m.blank(Npad, 2 * R.D)
    tok = m.eng.op_lore_tok_prepare(logi.to(DEV), dets.to(DEV) if use_pe else None, counts, x_pe.to(DEV) if use_pe else None,
                                    y_pe.to(DEV) if use_pe else None, x0, cat, use_pe, split=m.split)
    torch.cuda.synchronize()
    assert tok.cpu().tolist() == [[t, r] for t, c in enumerate(counts) for r in range(c)]
    rx, rc = x0.cpu(), cat.cpu()
    for h_x, h_c in zip(m.halves(rx), m.halves(rc)):
        assert m.is_sentinel(h_c[:, :R.D]), "cat[:, 0:256] was written"
        assert torch.equal(h_c[:, R.D:], h_x), "cat[:, 256:512] differs from x0"
        assert bool((h_x[N:].float() == 0).all()), "rows [N, Npad) are not zero"
    ref, t32 = R.tok_reference(logi, dets, counts, x_pe, y_pe, use_pe)
    worst = _ratio(f"token preparation use_pe={use_pe} [{name}]", m.get(rx[:N]), ref, t32 + R.store_tol(ref, name))
    if not use_pe:
        assert torch.equal(rx[:N], m.encode(torch.cat([logi[t, :c] for t, c in enumerate(counts)])))
    if m.split:
        hi, lo = m.halves(rx[:N])
        assert bool((lo.double().abs() <= 2.0 ** -8 * hi.double().abs()).all()), "a lo half is larger than half an ulp of its hi"
    print(f"lore token preparation use_pe={use_pe} [{name}]: worst err/tol {worst:.3f}")


# ---- the two copies --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_cvt_logic_and_scatter4_are_exact(engines, name):
    """cvt_logic_kernel: columns 0 .. 3 rounded to the format, channels 4 .. 31 zero, input columns 4 .. 7 (NaN) ignored, rows past Npad untouched.
    scatter4_kernel with the token map pt_op_lore_tok_prepare leaves: row r of table b = token row, rows at and beyond a table's count untouched."""
    m = engines(name)
    counts = R.TOK_COUNTS
    N, Npad = sum(counts), R.npad_of(sum(counts))
    g = torch.Generator().manual_seed(77)
    x = 3 * torch.randn(Npad, 8, generator=g)
    x[:, 4:] = float("nan")
    out = m.blank(Npad + 2, 32)
    m.eng.op_lore_cvt_logic(x.to(DEV), out, split=m.split)
    torch.cuda.synchronize()
    raw = out.cpu()
    assert m.is_sentinel(raw[Npad:]), "rows past Npad were written"
    want = torch.zeros(Npad, 32)
    want[:, :4] = x[:, :4]
    assert torch.equal(raw[:Npad], m.encode(want))

    logi = _tok_case()[0]
    tok = m.eng.op_lore_tok_prepare(logi.to(DEV), None, counts, None, None, m.blank(Npad, R.D), m.blank(Npad, 2 * R.D), False, split=m.split)
    res = torch.full((len(counts), L.PT_TSR_MAX_CELLS, 4), SENTINEL, dtype=torch.float32, device=DEV)
    m.eng.op_lore_scatter4(x.to(DEV), tok, res)
    torch.cuda.synchronize()
    res = res.cpu()
    for t, (t0, c) in enumerate(R.table_rows(counts)):
        assert torch.equal(res[t, :c], x[t0:t0 + c, :4]) and bool((res[t, c:] == SENTINEL).all()), t


# ---- refused calls ---------------------------------------------------------------------------------------------------------------------------------
def _p(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def _refused(m, fn, args, outs, match):
    keep = [o.cpu().clone() for o in outs]
    rc = getattr(m.eng.lib, fn)(m.eng._h, *args, m.eng._stream())
    torch.cuda.synchronize()
    with pytest.raises(L.PtError, match=match):
        L.check(rc, fn)
    for o, k in zip(outs, keep):
        assert torch.equal(o.cpu(), k), f"{fn} wrote its output although it refused the call"


@pytest.mark.parametrize("name", ALL)
def test_rejected_arguments(engines, name):
    """PT_ERR_INVALID with a message, and nothing is launched: the outputs keep their sentinel"""
    m = engines(name)
    sp = int(m.split)
    a16 = torch.full((256, 1536), 0.5, dtype=m.dt, device=DEV)
    f = torch.full((2, L.PT_TSR_MAX_CELLS, 256), 0.5, dtype=torch.float32, device=DEV)
    o16 = torch.full((256, 1024), SENTINEL, dtype=m.dt, device=DEV)
    o16b = torch.full((256, 1024), SENTINEL, dtype=m.dt, device=DEV)
    o32 = torch.full((2, L.PT_TSR_MAX_CELLS, 4), SENTINEL, dtype=torch.float32, device=DEV)
    i32 = torch.full((8192,), -1, dtype=torch.int32, device=DEV)
    cnt = lambda *c: np.asarray(c, dtype=np.int32)
    ok, over, neg, many = cnt(100, 28), cnt(100, L.PT_TSR_MAX_CELLS + 1), cnt(-1, 5), cnt(200, 100)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    outs = [o16, o16b, o32, i32]

    att = lambda qkv=_p(a16), c=ok, npad=128, tiles=_p(i32), out=_p(o16): [qkv, hp(c) if c is not None else C.c_void_p(0), 2, npad, tiles, out, sp]
    _refused(m, "pt_op_lore_attention", att(qkv=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_attention", att(out=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_attention", att(tiles=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_attention", att(c=None), outs, "host counts")
    _refused(m, "pt_op_lore_attention", att(c=over, npad=3200), outs, "bad cell count 3001")
    _refused(m, "pt_op_lore_attention", att(c=neg), outs, "bad cell count -1")
    _refused(m, "pt_op_lore_attention", att(qkv=_p(a16, 2)), outs, "unaligned pointer")
    _refused(m, "pt_op_lore_attention", att(npad=200), outs, "Npad = 200")
    _refused(m, "pt_op_lore_attention", att(c=many, npad=256), outs, "Npad = 256 must be a multiple of 128 and hold the 300 tokens")

    tp = lambda logi=_p(f), dets=_p(f), c=ok, pe=1, xpe=_p(f), npad=128, tok=_p(i32), x0=_p(o16), cat=_p(o16b): \
        [logi, dets, hp(c) if c is not None else C.c_void_p(0), 2, pe, xpe, _p(f), npad, tok, x0, cat, sp]
    _refused(m, "pt_op_lore_tok_prepare", tp(logi=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_tok_prepare", tp(cat=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_tok_prepare", tp(tok=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_tok_prepare", tp(dets=_p(None)), outs, "need the cell quads and both tables")
    _refused(m, "pt_op_lore_tok_prepare", tp(xpe=_p(None)), outs, "need the cell quads and both tables")
    _refused(m, "pt_op_lore_tok_prepare", tp(c=None), outs, "host counts")
    _refused(m, "pt_op_lore_tok_prepare", tp(c=over, npad=3200), outs, "bad cell count 3001")
    _refused(m, "pt_op_lore_tok_prepare", tp(npad=0), outs, "Npad = 0")
    _refused(m, "pt_op_lore_tok_prepare", tp(c=many, npad=256), outs, "hold the 300 tokens")

    nm = lambda x=_p(f), rows=4, a=_p(f), b=_p(f), out=_p(o16): [x, rows, a, b, out, sp]
    _refused(m, "pt_op_lore_norm", nm(x=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_norm", nm(out=_p(None)), outs, "null argument")
    _refused(m, "pt_op_lore_norm", nm(b=_p(None)), outs, "alpha and bias go together")
    _refused(m, "pt_op_lore_norm", nm(a=_p(None)), outs, "alpha and bias go together")
    _refused(m, "pt_op_lore_norm", nm(rows=0), outs, "rows = 0")
    _refused(m, "pt_op_lore_norm", nm(x=_p(f, 4)), outs, "unaligned pointer")

    _refused(m, "pt_op_lore_cvt_logic", [_p(None), _p(o16), 128, sp], outs, "null argument")
    _refused(m, "pt_op_lore_cvt_logic", [_p(f), _p(None), 128, sp], outs, "null argument")
    _refused(m, "pt_op_lore_cvt_logic", [_p(f), _p(o16), 100, sp], outs, "Npad = 100")
    _refused(m, "pt_op_lore_cvt_logic", [_p(f), _p(o16), 0, sp], outs, "Npad = 0")

    _refused(m, "pt_op_lore_scatter4", [_p(None), _p(i32), 4, _p(o32)], outs, "null argument")
    _refused(m, "pt_op_lore_scatter4", [_p(f), _p(None), 4, _p(o32)], outs, "null argument")
    _refused(m, "pt_op_lore_scatter4", [_p(f), _p(i32), 4, _p(None)], outs, "null argument")
    _refused(m, "pt_op_lore_scatter4", [_p(f), _p(i32), -1, _p(o32)], outs, "N = -1")


# ---- whole calls at the seams ----------------------------------------------------------------------------------------------------------------------
# counts -> (seed, position embeddings).  The decoders end in ReLU and output column 0 is 0 for every cell, so a case is only worth its time if enough
# of what it compares is not 0: the seeds were chosen on the CPU, with the oracle alone, so that at least MIN_NONZERO of the reference values are
MIN_NONZERO = 0.25
WHOLE_CASES = [([32], 32, False), ([64], 64, False), ([1], 1, False), ([L.PT_TSR_MAX_CELLS], 3000, False), ([31, 33, 0, 64], 128, True)]       # 38, 52, 50, 39 and 32 %


@functools.lru_cache(maxsize=1)
def _proc_sd():
    from pdf_table_amd.synth_weights import lore_processor_state_dict
    return lore_processor_state_dict(seed=31)


def whole_case(counts, seed, use_pe):
    """inputs of pt_tsr_process as tests/test_gpu_tsr.py draws them, and the oracle's (logic, stacked) [c, 4] per table (None for an empty one)"""
    from oracle import lore_processor as op
    g = torch.Generator().manual_seed(seed)
    n = len(counts)
    logi = torch.zeros(n, L.PT_TSR_MAX_CELLS, 256)
    dets = torch.zeros(n, L.PT_TSR_MAX_CELLS, 9)
    refs = []
    for t, c in enumerate(counts):
        logi[t, :c] = torch.randn(c, 256, generator=g)
        dets[t, :c, :8] = torch.rand(c, 8, generator=g) * 300 - 20
        if c:
            ps = dets[t, :c, :8].to(torch.int32).to(torch.float32).round().to(torch.int64).clamp(0, 255)[None]
            with torch.no_grad():
                lg, sk = op.processor_forward(_proc_sd(), logi[t:t + 1, :c], ps if use_pe else None)
            refs.append((lg[0], sk[0]))
        else:
            refs.append(None)
    return logi, dets, refs


def nonzero_fraction(refs):
    vals = torch.cat([torch.cat(r, 1).flatten() for r in refs if r is not None])
    return float((vals != 0).float().mean())


def _new_proc_engine(precision):
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.weights import pack_lore_processor
    e = HipEngine(0)
    e.load_weights(L.PT_MODEL_LORE_PROCESSOR, pack_lore_processor(_proc_sd()))
    e.set_precision(precision)
    return e


@pytest.fixture(scope="module")
def proc_x3():
    e = _new_proc_engine(L.PT_PRECISION_BF16X3)
    yield e
    e.close()


@pytest.mark.parametrize("counts,seed,use_pe", WHOLE_CASES, ids=["-".join(map(str, c[0])) for c in WHOLE_CASES])
def test_whole_call_at_the_seams(proc_x3, counts, seed, use_pe):
    """pt_tsr_process in BF16X3 against the oracle, every output column on its own: max|err| / max(1, max|ref|) of the column <= TOL_REL; a full last key
    tile (32, 64), a single cell, the cell limit, and a batch with an empty table between unaligned neighbours"""
    logi, dets, refs = whole_case(counts, seed, use_pe)
    frac = nonzero_fraction(refs)
    assert frac >= MIN_NONZERO, f"only {frac:.0%} of the reference values are not 0"
    logic, stacked = proc_x3.tsr_process(logi.to(DEV), dets.to(DEV), counts, use_2dpe=use_pe)
    torch.cuda.synchronize()
    got = torch.cat([torch.cat([logic[t, :c], stacked[t, :c]], 1).cpu() for t, c in enumerate(counts) if c])
    ref = torch.cat([torch.cat(r, 1) for r in refs if r is not None])
    for t, c in enumerate(counts):
        assert bool((logic[t, c:] == 0).all()) and bool((stacked[t, c:] == 0).all()), "rows at and beyond the count were written"
    col = (got - ref).abs().max(0).values / ref.abs().max(0).values.clamp(min=1.0)
    print(f"lore whole call {counts} use_pe={use_pe}: {frac:.0%} non-zero, worst column err {float(col.max()):.2e} (columns {[f'{float(v):.1e}' for v in col]})")
    assert float(col.max()) <= TOL_REL, col


@pytest.mark.parametrize("name", ["bf16", "bf16x3"])
def test_a_small_call_after_a_large_one_is_a_fresh_engines(name):
    """[700] then [1] on one engine: the result of [1] is bit-identical to [1] on a fresh engine -- nothing the larger call left in the arena reaches it"""
    small = whole_case([1], WHOLE_CASES[2][1], False)
    large = whole_case([700], 700, False)
    res = []
    for warm in (True, False):
        e = _new_proc_engine(MODES[name])
        try:
            if warm:
                e.tsr_process(large[0].to(DEV), large[1].to(DEV), [700])
            res.append([t.cpu() for t in e.tsr_process(small[0].to(DEV), small[1].to(DEV), [1])])
            torch.cuda.synchronize()
        finally:
            e.close()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())
