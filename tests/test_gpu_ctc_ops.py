"""pt_op_ctc_greedy (csrc/ctc_ops.hip) alone, through HipEngine.op_ctc_greedy, in the three storage modes (bf16, f16, the (hi | lo) pair mode): per
token row the lowest index of the largest logit and that class's soft-max probability, in one pass over the logits.

Reference: float64 NumPy on exactly the values the kernel reads (the 16-bit inputs; hi + lo of a pair), np.argmax (lowest index among equal values)
and 1 / sum exp(l - max).  ids must be equal on every row.  conf has no tolerance chosen in advance: in the same test the layered route
(op_softmax(f32=True).max(-1), what the crop door runs) is measured on the same input against the same reference, and the new kernel's largest relative
error must be within 4 x that figure -- and is never asked to be below 2^-23, one fp32 rounding of the reciprocal plus one of the sum.  Both figures
are printed.

Shapes (rows, C, Cp): a single channel; C < 64 with rows that do not fill a workgroup; Cp % 8 != 0 (2-byte loads, unaligned rows); padded channels;
many chunks per lane.  Ties need two channels (a tie 64 channels apart needs C > 64, one 512 apart -- the same lane under the 16-byte mapping --
C > 512): on shapes too narrow for a kind of tie the rows keep their seeded values."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MODES = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "split": L.PT_PRECISION_BF16X3}
SHAPES = [(1, 1, 8), (7, 38, 40), (10, 97, 97), (10, 97, 104), (5, 6625, 6656)]
CASES = ["normal", "max_first", "max_last", "ties", "all_equal", "large_negative", "hot_padding", "lo_decides"]
TOP = 40.0          # above every seeded logit (6 sigma-scaled normals stay below 36), exact in bf16 and f16


@pytest.fixture(scope="module")
def engines():
    from pdf_table_amd.engine import HipEngine
    made = {}

    def get(mode):
        if mode not in made:
            e = HipEngine(0)
            e.set_precision(MODES[mode])
            made[mode] = e
        return made[mode]
    yield get
    for e in made.values():
        e.close()


def _inputs(case, mode, rows, C, Cp, seed):
    """-> (hi, lo) float64 arrays [rows, Cp] of values that are exact in the storage format (lo is zeros outside the pair mode)"""
    dt = torch.float16 if mode == "f16" else torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, Cp, generator=g, dtype=torch.float64) * 6.0
    if case == "all_equal":
        x[:] = 1.5
    if case == "large_negative":
        x = x + (-6.0e4 if mode == "f16" else -3.0e4)
    hi = x.to(dt).double()
    lo = (x - hi).to(dt).double() if mode == "split" else torch.zeros_like(hi)
    hi[:, C:], lo[:, C:] = 0.0, 0.0
    if case == "max_first":
        hi[:, 0], lo[:, 0] = TOP, 0.0
    elif case == "max_last":
        hi[:, C - 1], lo[:, C - 1] = TOP, 0.0
    elif case == "ties" and C >= 2:
        for i in range(rows):
            a = (3 * i) % (C - 1)
            kind = i % 3
            if kind == 1 and a + 64 < C:
                b = a + 64                      # the same lane when lane = channel % 64
            elif kind == 2 and a + 512 < C:
                b = a + 512                     # the same lane when lane = (channel / 8) % 64
            else:
                b = a + 1 + (5 * i) % (C - 1 - a)
            hi[i, a] = hi[i, b] = TOP
            lo[i, a] = lo[i, b] = 0.0
    elif case == "hot_padding":
        hi[:, C:] = float(torch.tensor(1.0e4).to(dt))      # +1e4 as the format stores it: above every real logit
    elif case == "lo_decides" and mode == "split" and C >= 2:
        for i in range(rows):
            a = (3 * i) % (C - 1)
            b = a + 1 + (5 * i) % (C - 1 - a)
            hi[i, a] = hi[i, b] = TOP
            lo[i, a], lo[i, b] = (0.0, 2.0 ** -4) if i % 2 == 0 else (2.0 ** -4, 0.0)      # |lo| <= ulp(40) / 2 = 2^-3: a normalised pair
    return hi.numpy(), lo.numpy()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", list(MODES))
def test_ctc_greedy(engines, mode, case):
    eng = engines(mode)
    split = mode == "split"
    dt = torch.float16 if mode == "f16" else torch.bfloat16
    for si, (rows, C, Cp) in enumerate(SHAPES):
        hi, lo = _inputs(case, mode, rows, C, Cp, 100 * CASES.index(case) + si)
        th = torch.from_numpy(hi).to(dt)
        assert np.array_equal(th.double().numpy(), hi)                      # the inputs are exact in the storage format
        x = torch.cat([th, torch.from_numpy(lo).to(dt)], -1) if split else th
        x = x.contiguous().to(DEV)
        v = (hi + lo)[:, :C]                                                # float64: what the kernel reads
        want_ids = np.argmax(v, -1)
        want_conf = 1.0 / np.exp(v - v.max(-1, keepdims=True)).sum(-1)
        ids, conf = eng.op_ctc_greedy(x, C, split=split)
        layered = eng.op_softmax(x, C, f32=True, split=split).max(-1).values
        torch.cuda.synchronize()
        eng.check()
        assert ids.dtype == torch.int32 and conf.dtype == torch.float32 and tuple(ids.shape) == tuple(conf.shape) == (rows,)
        got_ids, got_conf = ids.cpu().numpy(), conf.cpu().numpy().astype(np.float64)
        assert np.array_equal(got_ids, want_ids), (case, mode, (rows, C, Cp), got_ids, want_ids)
        err = float((np.abs(got_conf - want_conf) / want_conf).max())
        err_layered = float((np.abs(layered.cpu().numpy().astype(np.float64) - want_conf) / want_conf).max())
        print(f"ctc_greedy {mode} {case} rows={rows} C={C} Cp={Cp}: conf rel err {err:.3e}, layered route {err_layered:.3e}")
        assert np.isfinite(got_conf).all()
        assert err <= max(4.0 * err_layered, 2.0 ** -23), (case, mode, (rows, C, Cp), err, err_layered)
        if case == "all_equal":
            assert (got_ids == 0).all() and np.abs(got_conf - 1.0 / C).max() <= 2.0 ** -23 / C
