"""pt_op_pico_candidates (csrc/layout_ops.hip) alone, through HipEngine.op_pico_candidates, in the three storage modes (bf16, f16, the (hi | lo) pair
mode) on activations built here -- no network runs.

Reference: NumPy on the fp32 values ``HipGraphExecutor.values()`` would compute from the same bits (float(hi), or float(hi) + float(lo) as one fp32
add), the real channels only: an anchor is a candidate when the fp32 maximum of its class values is > thr_lo, its record is (int32 level, int32 anchor,
the class values, the 32 distribution values, zeros up to 48).  Every comparison is EXACT, on the raw 32-bit words: the kernel converts, adds once and
copies, so there is nothing to tolerate.  Arrival order inside a page is not defined: records are compared after sorting by (level, anchor).

Every input has its padding channels filled with +1e4 (scores and distributions): they must never make a candidate or leak into a record.  Page 0
holds candidates at anchor 0 and A_l - 1 of every level, rows whose maximum EQUALS thr_lo (not kept) and, in the pair mode, rows that only hi + lo
decides; page 1 holds no candidate (count 0, slab untouched); the last page is all candidates (count = sum A_l, and again both edges of every level).
The output buffer is pre-filled with a sentinel word, so whatever the kernel did not have to write must still hold it."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.onnx_exec import _pad64        # the executor's rule for the padded width of an output's channel slice

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MODES = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "split": L.PT_PRECISION_BF16X3}
B = 3
THR = 0.5                 # exact in bf16 and f16, so a score can EQUAL it
SENTINEL = 0x7FC0BEEF     # a NaN pattern no conversion of a 16-bit value produces
RF = L.PT_LAYOUT_CAND_FLOATS
# (anchors per level, classes, wider rows than the executor's rule): the two anchor sets, every class count, L = 1 and L = 3 once each, and one set
# whose 403 anchors per page need a second workgroup along x
CASES = [((77, 21, 5, 1), 1, False), ((77, 21, 5, 1), 5, False), ((77, 21, 5, 1), 10, True), ((96, 24, 6, 2), 1, False), ((96, 24, 6, 2), 5, True),
         ((96, 24, 6, 2), 10, False), ((77,), 5, False), ((77, 21, 5), 10, False), ((300, 77, 21, 5), 10, False)]


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


def _dt(mode):
    return torch.float16 if mode == "f16" else torch.bfloat16


def _pair(x: torch.Tensor, mode):
    """fp64 values -> (hi, lo) as the storage format holds them (lo zeros outside the pair mode)"""
    dt = _dt(mode)
    hi = x.to(dt)
    lo = (x - hi.double()).to(dt) if mode == "split" else torch.zeros_like(hi)
    return hi, lo


def make_inputs(mode, anchors, ncls, wide, seed, full_last=True, stride=7):
    """-> per level (score hi, score lo, dist hi, dist lo), 16-bit tensors [B, A_l, Cp] on the host"""
    cps, cpd = (_pad64(ncls) + 64, _pad64(32) + 64) if wide else (_pad64(ncls), _pad64(32))
    dt = _dt(mode)
    g = torch.Generator().manual_seed(seed)
    hot = torch.tensor(1.0e4).to(dt)                       # +1e4 as the format stores it
    levels = []
    for A in anchors:
        s_hi, s_lo = _pair(torch.rand(B, A, cps, generator=g, dtype=torch.float64) * 0.45, mode)          # below thr_lo, hi + lo too
        c_hi, c_lo = _pair(0.55 + 0.45 * torch.rand(B, A, cps, generator=g, dtype=torch.float64), mode)   # candidate values
        d_hi, d_lo = _pair(torch.randn(B, A, cpd, generator=g, dtype=torch.float64) * 3.0, mode)
        for a in range(A):
            ch = a % ncls
            edge = a in (0, A - 1)
            if edge or a % stride == 0:                     # page 0: both edges of the level and every stride-th anchor
                s_hi[0, a, ch], s_lo[0, a, ch] = c_hi[0, a, ch], c_lo[0, a, ch]
            elif a % stride == 3:                           # the maximum EQUALS thr_lo: not kept
                s_hi[0, a, ch], s_lo[0, a, ch] = THR, 0.0
            elif a % stride == 4 and mode == "split":       # hi alone <= thr_lo, hi + lo > thr_lo: kept
                s_hi[0, a, ch], s_lo[0, a, ch] = THR, 2.0 ** -12
            elif a % stride == 5 and mode == "split":       # hi alone > thr_lo, hi + lo == thr_lo: not kept
                s_hi[0, a, ch], s_lo[0, a, ch] = THR + 2.0 ** -8, -(2.0 ** -8)
            if full_last:                                   # the last page: every anchor
                s_hi[B - 1, a, ch], s_lo[B - 1, a, ch] = c_hi[B - 1, a, ch], c_lo[B - 1, a, ch]
        s_hi[..., ncls:], s_lo[..., ncls:], d_hi[..., 32:], d_lo[..., 32:] = hot, hot, hot, hot
        levels.append((s_hi, s_lo, d_hi, d_lo))
    return levels


def device_tensors(levels, mode):
    """the activations as the executor holds them: [B, 1, A_l, Cp] ([hi | lo] of twice the width in the pair mode)"""
    sc, bd = [], []
    for s_hi, s_lo, d_hi, d_lo in levels:
        s = torch.cat([s_hi, s_lo], -1) if mode == "split" else s_hi
        d = torch.cat([d_hi, d_lo], -1) if mode == "split" else d_hi
        sc.append(s[:, None].contiguous().to(DEV))
        bd.append(d[:, None].contiguous().to(DEV))
    return sc, bd


def reference(levels, mode, ncls, thr=THR):
    """-> per page the expected records [k, 48] as uint32 words in (level, anchor) order"""
    pages = [[] for _ in range(B)]
    for l, (s_hi, s_lo, d_hi, d_lo) in enumerate(levels):
        sv, dv = s_hi[..., :ncls].float().numpy(), d_hi[..., :32].float().numpy()
        if mode == "split":
            sv, dv = sv + s_lo[..., :ncls].float().numpy(), dv + d_lo[..., :32].float().numpy()          # one fp32 add, as values() does
        assert sv.dtype == dv.dtype == np.float32
        for b in range(B):
            keep = np.nonzero(sv[b].max(1) > np.float32(thr))[0]
            r = np.zeros((len(keep), RF), np.float32)
            r[:, 0] = np.full(len(keep), l, np.int32).view(np.float32)
            r[:, 1] = keep.astype(np.int32).view(np.float32)
            r[:, 2:2 + ncls], r[:, 2 + ncls:2 + ncls + 32] = sv[b][keep], dv[b][keep]
            pages[b].append(r)
    return [np.concatenate(p, 0).view(np.uint32) for p in pages]


def fresh_out(max_cands, canary=0):
    """(counts, cands, backing buffer): cands pre-filled with the sentinel, `canary` more sentinel words behind it"""
    buf = torch.full((B * max_cands * RF + canary,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    counts = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    return counts, buf[:B * max_cands * RF].view(B, max_cands, RF), buf


def sorted_words(rec_u32):
    return rec_u32[np.lexsort((rec_u32[:, 1].view(np.int32), rec_u32[:, 0].view(np.int32)))]


def check_pages(counts, cands, want, max_cands):
    got_counts = counts.cpu().numpy()
    words = cands.cpu().numpy().view(np.uint32)
    assert got_counts.tolist() == [len(w) for w in want]
    for b in range(B):
        k = len(want[b])
        assert k <= max_cands
        assert np.array_equal(sorted_words(words[b, :k]), want[b]), f"page {b}: records differ"
        assert (words[b, k:] == SENTINEL).all(), f"page {b}: words behind the {k} records were written"


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"A{'-'.join(map(str, a))}_c{n}{'_wide' if w else ''}" for a, n, w in CASES])
@pytest.mark.parametrize("mode", list(MODES))
def test_pico_candidates(engines, mode, case):
    anchors, ncls, wide = CASES[case]
    eng = engines(mode)
    levels = make_inputs(mode, anchors, ncls, wide, seed=10 * case + 1)
    want = reference(levels, mode, ncls)
    total = sum(anchors)
    # the planted cases are really in the input: edges on the first and the last page, an empty page, a full page, rows equal to thr_lo
    assert len(want[1]) == 0 and len(want[B - 1]) == total and 0 < len(want[0]) < total
    for b in (0, B - 1):
        got_la = {(int(r[0]), int(r[1])) for r in want[b]}
        assert all((l, 0) in got_la and (l, A - 1) in got_la for l, A in enumerate(anchors))
    s0_hi, s0_lo = levels[0][0], levels[0][1]
    if anchors[0] > 10:
        kept0 = {int(r[1]) for r in want[0] if int(r[0]) == 0}
        assert float(s0_hi[0, 3, :ncls].float().max()) == THR and 3 not in kept0
        if mode == "split":
            assert float(s0_hi[0, 4, :ncls].float().max()) <= THR and 4 in kept0             # hi alone would drop it
            assert float(s0_hi[0, 5, :ncls].float().max()) > THR and 5 not in kept0          # hi alone would keep it
            assert float(s0_lo[0, 4, 4 % ncls]) > 0 > float(s0_lo[0, 5, 5 % ncls])
    sc, bd = device_tensors(levels, mode)
    max_cands = total + 3
    counts, cands, _ = fresh_out(max_cands)
    eng.op_pico_candidates(sc, bd, ncls, THR, max_cands=max_cands, split=mode == "split", out=(counts, cands))
    torch.cuda.synchronize()
    eng.check()
    check_pages(counts, cands, want, max_cands)
    # new tensors when no buffers are given
    c2, r2 = eng.op_pico_candidates(sc, bd, ncls, THR, max_cands=max_cands, split=mode == "split")
    torch.cuda.synchronize()
    assert c2.dtype == torch.int32 and r2.dtype == torch.float32 and tuple(r2.shape) == (B, max_cands, RF)
    assert c2.cpu().numpy().tolist() == [len(w) for w in want]
    for b in range(B):
        assert np.array_equal(sorted_words(r2[b, :len(want[b])].cpu().numpy().view(np.uint32)), want[b])


@pytest.mark.parametrize("mode", list(MODES))
def test_pico_candidates_overflow(engines, mode):
    """max_cands below a page's count: counts report the true number, the stored records are distinct members of the expected set, the next page's
    slab and a canary behind the buffer are intact"""
    anchors, ncls = (77, 21, 5, 1), 5
    eng = engines(mode)
    levels = make_inputs(mode, anchors, ncls, False, seed=77)
    want = reference(levels, mode, ncls)
    max_cands = 8
    assert len(want[0]) > max_cands and len(want[B - 1]) > max_cands and len(want[1]) == 0
    sc, bd = device_tensors(levels, mode)
    counts, cands, buf = fresh_out(max_cands, canary=4 * RF)
    eng.op_pico_candidates(sc, bd, ncls, THR, max_cands=max_cands, split=mode == "split", out=(counts, cands))
    torch.cuda.synchronize()
    eng.check()
    assert counts.cpu().numpy().tolist() == [len(w) for w in want]
    words = cands.cpu().numpy().view(np.uint32)
    for b in (0, B - 1):
        expect = {w.tobytes() for w in want[b]}
        stored = [w.tobytes() for w in words[b]]
        assert all(s_ in expect for s_ in stored) and len(set(stored)) == max_cands
    assert (words[1] == SENTINEL).all()                                               # the slab after an overflowing page
    assert (buf.view(torch.int32)[B * max_cands * RF:].cpu().numpy().view(np.uint32) == SENTINEL).all()      # the canary behind the last page


@pytest.mark.parametrize("mode", list(MODES))
def test_pico_candidates_second_call(engines, mode):
    """two calls on the same output buffers with different inputs: the counters start from zero again, the second result holds nothing of the first"""
    anchors, ncls = (96, 24, 6, 2), 10
    eng = engines(mode)
    first = make_inputs(mode, anchors, ncls, False, seed=5)
    second = make_inputs(mode, anchors, ncls, False, seed=6, full_last=False, stride=11)
    want1, want2 = reference(first, mode, ncls), reference(second, mode, ncls)
    assert 0 < len(want2[0]) < len(want1[0]) and len(want2[B - 1]) == 0 < len(want1[B - 1])
    max_cands = sum(anchors)
    counts, cands, _ = fresh_out(max_cands)
    for levels, want in ((first, want1), (second, want2)):
        sc, bd = device_tensors(levels, mode)
        eng.op_pico_candidates(sc, bd, ncls, THR, max_cands=max_cands, split=mode == "split", out=(counts, cands))
        torch.cuda.synchronize()
        eng.check()
        got_counts = counts.cpu().numpy()
        words = cands.cpu().numpy().view(np.uint32)
        assert got_counts.tolist() == [len(w) for w in want]
        for b in range(B):
            assert np.array_equal(sorted_words(words[b, :len(want[b])]), want[b])


def test_pico_candidates_refuses_15_classes(engines):
    """ncls + 32 must fit the record behind (level, anchor): 15 classes are an invalid argument, and nothing is launched or zeroed"""
    eng = engines("bf16")
    levels = make_inputs("bf16", (21, 5), 5, False, seed=3)
    sc, bd = device_tensors(levels, "bf16")
    counts, cands, _ = fresh_out(16)
    with pytest.raises(L.PtError, match="pt_op_pico_candidates"):
        eng.op_pico_candidates(sc, bd, 15, THR, max_cands=16, out=(counts, cands))
    torch.cuda.synchronize()
    eng.check()
    assert counts.cpu().numpy().tolist() == [7] * B and (cands.cpu().numpy().view(np.uint32) == SENTINEL).all()
    with pytest.raises(L.PtError, match="pt_op_pico_candidates"):          # five levels: more than a launch takes
        eng.op_pico_candidates(sc * 3, bd * 3, 5, THR, max_cands=16, out=(counts, cands))
