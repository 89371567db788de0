"""pt_op_sla_decode (csrc/sla_head.hip) alone, through HipEngine.op_sla_decode, in the three storage modes (bf16, f16, the (hi | lo) pair mode): the whole
greedy walk of SLANet's attention-GRU head in one launch, against the float64 restatement of tests/slanet_ref.py on exactly the values the kernel
reads (weights and fea as the storage mode holds them; hi + lo in the pair mode).

Forced walk (every mode): the ids fed back are the float64 walk's, so all three routes walk the same sequence and every step's probs and loc compare.
No bound is chosen in advance: the yardstick is the same recurrence by plain torch on the CPU in fp32 on the same inputs against float64; the kernel's
largest absolute error over probs and loc must be within 4 x that figure (never asked to be below 2^-23: the outputs lie in [0, 1] and are stored as
fp32 after one rounding of the quotient and one of the sum under it).  Both figures are printed.

Greedy walk (pair mode): ids and steps equal the float64 walk's on every table, zeros after the stop row, all T rows with eos_id = -1.  The test first
asserts ON THE REFERENCE ALONE that every walked step's top-two logit margin exceeds 4 x the measured fp32 logit error; no step is left out.

Shapes: N 1 (one token) / 20 (not a multiple of the wave count or of 16) / 256 (the model's); (V, L) (30, 4) / (50, 8); (H, C) (256, 96) / (64, 40) --
the narrow one with rows padded to 48 channels and the padding filled with 1e4, which must never be read as data; T 1 / 12; B 1 / 3 / 17."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slanet_ref as R  # noqa: E402
from pdf_table_amd import lib as L
from pdf_table_amd import weights as W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MODES = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "split": L.PT_PRECISION_BF16X3}
# (N, H, C, c_pad, V, L, T, B): every listed value of every dimension, and each (H, C) with each (V, L), N and more than one B
SHAPES = [(256, 256, 96, 96, 50, 8, 12, 17), (20, 64, 40, 48, 30, 4, 12, 3), (1, 256, 96, 96, 30, 4, 1, 1), (20, 256, 96, 96, 50, 8, 12, 1),
          (256, 64, 40, 48, 30, 4, 12, 3), (1, 64, 40, 48, 50, 8, 12, 17), (256, 256, 96, 96, 30, 4, 1, 3)]
FLOOR = 2.0 ** -23


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


@functools.lru_cache(maxsize=None)
def case(shape, mode, tie=False):
    """the head and the tokens as `mode` stores them, the float64 free walk (eos_id = -1), the forced float64 and fp32 walks.  Computed once, shared."""
    N, H, C, Cp, V, Lo, T, B = shape
    seed = 1000 + SHAPES.index(shape)
    p = R.make_head(seed, H, C, V, Lo)
    if tie:                     # two generator rows made equal and pushed to the top: the logits of classes 3 and 7 are equal and the largest
        p["s2_w"][7] = p["s2_w"][3]
        p["s2_b"][3] = p["s2_b"][7] = 40.0
    ps = R.storable_head(p, mode)
    fea, (fhi, flo) = R.storable(R.make_fea(seed + 500, B, N, C), mode)
    free = R.sla_walk(ps, fea, T)
    forced64 = R.sla_walk(ps, fea, T, force_ids=free["ids"])
    forced32 = R.sla_walk(ps, fea, T, dtype=torch.float32, force_ids=free["ids"])
    return dict(p=p, ps=ps, fea=fea, fhi=fhi, flo=flo, free=free, f64=forced64, f32=forced32)


def device_operands(eng, c, shape, mode):
    N, H, C, Cp, V, Lo, T, B = shape
    split = mode == "split"
    fmt = "f16" if mode == "f16" else "bf16"
    dt = torch.float16 if mode == "f16" else torch.bfloat16
    w16, vec = W.pack_sla_head(c["p"], fmt=fmt, split=split)
    halves = []
    for part in ((c["fhi"], c["flo"]) if split else (c["fhi"],)):
        rows = np.full((B, N, Cp), 1.0e4)                   # hot padding: channels C .. Cp - 1 are not data
        rows[:, :, :C] = part
        halves.append(torch.from_numpy(rows).to(dt))
    fea = torch.cat(halves, -1).contiguous().to(DEV)
    return fea, torch.from_numpy(w16.view(np.int16)).to(DEV), torch.from_numpy(vec).to(DEV)


def run(eng, c, shape, mode, eos_id=-1, force=None):
    N, H, C, Cp, V, Lo, T, B = shape
    fea, w16, vec = device_operands(eng, c, shape, mode)
    f = None if force is None else torch.from_numpy(force.astype(np.int32)).to(DEV)
    probs, loc, ids, steps = eng.op_sla_decode(fea, C, w16, vec, H, V, Lo, T, eos_id=eos_id, force_ids=f, split=mode == "split")
    torch.cuda.synchronize()
    eng.check()
    assert probs.dtype == torch.float32 and tuple(probs.shape) == (B, T, V) and tuple(loc.shape) == (B, T, Lo)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, T) and steps.dtype == torch.int32 and tuple(steps.shape) == (B,)
    return probs.cpu().numpy().astype(np.float64), loc.cpu().numpy().astype(np.float64), ids.cpu().numpy(), steps.cpu().numpy()


def walk_err(a_probs, a_loc, ref):
    return max(float(np.abs(a_probs - ref["probs"]).max()), float(np.abs(a_loc - ref["loc"]).max()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_H%d_C%d_V%d_L%d_T%d_B%d" % (s[0], s[1], s[2], s[4], s[5], s[6], s[7]))
@pytest.mark.parametrize("mode", list(MODES))
def test_forced_walk(engines, mode, shape):
    c = case(shape, mode)
    probs, loc, ids, steps = run(engines(mode), c, shape, mode, force=c["free"]["ids"])
    yard = walk_err(c["f32"]["probs"], c["f32"]["loc"], c["f64"])
    err = walk_err(probs, loc, c["f64"])
    print(f"sla forced {mode} {shape}: kernel max abs err {err:.3e}, torch fp32 on the CPU {yard:.3e}")
    assert np.isfinite(probs).all() and np.isfinite(loc).all()
    assert (steps == shape[6]).all()
    assert err <= max(4.0 * yard, FLOOR), (mode, shape, err, yard)


def pick_eos(free, V, T):
    """the class whose use as `eos` stops the number of tables closest to half of them before the last step -- read off the float64 walk alone"""
    ids = free["ids"]
    best, best_d = 0, None
    for k in range(V):
        stops = sum(1 for b in range(ids.shape[0]) if (ids[b, 1:T - 1] == k).any()) if T > 2 else 0
        d = abs(stops - ids.shape[0] / 2.0)
        if best_d is None or d < best_d:
            best, best_d = k, d
    return best


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_H%d_C%d_V%d_L%d_T%d_B%d" % (s[0], s[1], s[2], s[4], s[5], s[6], s[7]))
def test_greedy_walk_pairs(engines, shape):
    mode = "split"
    N, H, C, Cp, V, Lo, T, B = shape
    c = case(shape, mode)
    free = c["free"]
    # pre-condition, on the reference alone: no walked step is closer to a tie than 4 x the fp32 logit error
    logit_err = float(np.abs(c["f32"]["logits"] - c["f64"]["logits"]).max())
    margin = float(R.top2_margin(free["logits"]).min())
    print(f"sla greedy {shape}: smallest top-two margin {margin:.3e}, fp32 logit error {logit_err:.3e}")
    assert margin > 4.0 * logit_err, (shape, margin, logit_err)
    eng = engines(mode)
    # eos_id = -1: all T rows
    probs, loc, ids, steps = run(eng, c, shape, mode)
    assert (steps == T).all() and np.array_equal(ids, free["ids"])
    yard = walk_err(c["f32"]["probs"], c["f32"]["loc"], c["f64"])
    assert walk_err(probs, loc, free) <= max(4.0 * yard, FLOOR)
    # with an eos class: stop rows, counts, zeros after them
    eos = pick_eos(free, V, T)
    want = R.sla_walk(c["ps"], c["fea"], T, eos_id=eos)
    if B >= 3 and T > 2:
        assert (want["steps"] < T).any() and (want["steps"] == T).any(), want["steps"]      # the case does exercise both ends
    probs, loc, ids, steps = run(eng, c, shape, mode, eos_id=eos)
    assert np.array_equal(steps, want["steps"]), (steps, want["steps"])
    assert np.array_equal(ids, want["ids"])
    for b in range(B):
        n = int(steps[b])
        assert not probs[b, n:].any() and not loc[b, n:].any() and not ids[b, n:].any()
        assert np.abs(probs[b, :n].sum(-1) - 1.0).max() < 1e-5
    assert walk_err(probs, loc, want) <= max(4.0 * yard, FLOOR)


def test_eos_at_step_zero_does_not_stop(engines):
    """the reference's rule (t > 0): a table whose FIRST id is the eos class walks on"""
    shape, mode = SHAPES[1], "split"
    c = case(shape, mode)
    eos = int(c["free"]["ids"][0, 0])
    want = R.sla_walk(c["ps"], c["fea"], shape[6], eos_id=eos)
    assert want["steps"][0] > 1
    probs, loc, ids, steps = run(engines(mode), c, shape, mode, eos_id=eos)
    assert np.array_equal(steps, want["steps"]) and np.array_equal(ids, want["ids"])


@pytest.mark.parametrize("mode", list(MODES))
def test_ties_take_the_lower_index(engines, mode):
    shape = SHAPES[1]
    c = case(shape, mode, tie=True)
    assert (c["free"]["ids"] == 3).all() and np.array_equal(c["free"]["logits"][..., 3], c["free"]["logits"][..., 7])
    probs, loc, ids, steps = run(engines(mode), c, shape, mode)
    assert (ids == 3).all()
    assert np.array_equal(probs[..., 3], probs[..., 7])


@pytest.mark.parametrize("what", ["N=257", "V=65", "H=48"])
def test_refusals(engines, what):
    eng = engines("bf16")
    N, H, C, V, Lo, T, B = 20, 64, 40, 30, 4, 2, 1
    if what == "N=257":
        N = 257
    elif what == "V=65":
        V = 65
    else:
        H = 48
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)      # every pointer valid and aligned: the refusal must come from the sizes
    p = buf.data_ptr()
    rc = eng.lib.pt_op_sla_decode(eng._h, p, B, N, 40, C, H, V, Lo, T, p, p, p, 1 << 18, -1, None, p, p, p, p, 0, None)
    assert rc == 1, rc                                               # PT_ERR_INVALID
    msg = eng.lib.pt_last_error().decode()
    assert "pt_op_sla_decode" in msg and what.split("=")[1] in msg, msg
    torch.cuda.synchronize()
    assert not buf.any()                                             # and nothing was launched
