"""The generic ONNX executor's LSTM layer on the GPU (pdf_table_amd/onnx_exec.py::_lstm -> pt_op_conv2d for the input projection, pt_op_lstm of
csrc/lstm_op.hip for the recurrence), operator level: ``LstmOnly`` graphs from PyTorch's exporter and hand-built one-node graphs
(tools/onnx_export_rnn.py) through ``HipGraphExecutor``, against the fp64 evaluation of the operator definition (tests/onnx_lstm_ref.py).

Shapes -- the smallest at which the kernel can still go wrong:

    H 48, I 40, T 5, B 3, bidirectional     padding of H (48 -> K 64) and I (40 -> 64); an odd T, so a reverse walk that is off by one shows;
                                            a partial tile of 16 sequences
    H 48, I 40, T 5, B 17                   a second sequence tile with one live sequence
    H 128, I 64, T 4, B 2                   the LDS limit (128 KiB of recurrent weights; two unit blocks per wave; R_lo streamed in bf16x3)
    H 24, I 24, T 7, B 1                    direction="reverse" alone (hand-built node), and forward alone
    H 48, I 40, T 6, B 3, 2 layers + Linear the Y view feeding the next LSTM and the GEMM without a copy
    H 48, T 1                               a single step

Tolerances.  ``bf16x3``: max |error| <= 1e-3 against the fp32 module, the project's bound for that mode (tests/test_gpu_onnx_seq.py).  ``bf16``
and ``f16``: the bound of a case is TWICE the error of the CPU emulation (onnx_lstm_ref.stack_emulated: operands, pre-gates and h rounded to
the storage format, c in fp32) against fp64 on that case -- computed here on the CPU, never from the engine; the factor 2 is for the MFMA's
summation order and the fast sigmoid / tanh.  Measured on an MI355X (profiles/r08/onnx_lstm.txt), max |engine - fp64| / max |emulation - fp64|:

    case        bf16 engine   bf16 emul.  ratio   f16 engine    f16 emul.  ratio  bf16x3 vs fp32
    bi48-b3       7.686e-03    7.686e-03   1.00    9.666e-04    9.666e-04   1.00       1.284e-05
    bi48-b17      6.851e-03    6.851e-03   1.00    8.257e-04    8.257e-04   1.00       1.159e-05
    bi128         4.442e-03    4.442e-03   1.00    6.257e-04    6.257e-04   1.00       7.927e-06
    rev24         3.320e-03    3.320e-03   1.00    2.472e-04    2.472e-04   1.00       6.370e-06
    fwd24         2.430e-03    2.430e-03   1.00    3.811e-04    3.811e-04   1.00       7.845e-06
    stack48       6.011e-03    6.011e-03   1.00    5.139e-04    5.476e-04   0.94       8.881e-06
    bi48-t1       3.443e-03    3.443e-03   1.00    6.340e-04    6.340e-04   1.00       6.318e-06

The engine's error equals the emulation's to the printed digits on the single-layer cases: the same roundings in the same places.
"""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# name: (H, I, T, B, kind)   kind: bi / fwd (torch export), rev (hand-built node), stack (two bidirectional layers + Linear(30))
CASES = {"bi48-b3": (48, 40, 5, 3, "bi"), "bi48-b17": (48, 40, 5, 17, "bi"), "bi128": (128, 64, 4, 2, "bi"), "rev24": (24, 24, 7, 1, "rev"),
         "fwd24": (24, 24, 7, 1, "fwd"), "stack48": (48, 40, 6, 3, "stack"), "bi48-t1": (48, 40, 1, 3, "bi")}
_CACHE = {}


def _case(name):
    """-> (onnx bytes, x [B, I, 1, T] fp32, fp64 reference [T, B, C], fp32 module output, {fmt: emulation}) -- computed once, shared, read-only"""
    if name in _CACHE:
        return _CACHE[name]
    import onnx_export as X
    import onnx_export_rnn as XR
    import onnx_lstm_ref as LR
    H, I, T, B, kind = CASES[name]
    seed = sorted(CASES).index(name) + 40
    x = torch.randn(B, I, 1, T, generator=torch.Generator().manual_seed(seed))
    xs = x.squeeze(2).permute(2, 0, 1).numpy()                                     # [T, B, I]
    m = XR.seeded_rnn(XR.LstmOnly(I, H, bidirectional=kind in ("bi", "stack"), layers=2 if kind == "stack" else 1, out=30 if kind == "stack" else 0), seed)
    layers = [XR.onnx_lstm_params(r) for r in m.rnns]
    head = None if m.head is None else (m.head.weight.detach().numpy(), m.head.bias.detach().numpy())
    if kind == "rev":
        W, R, Bv, _ = layers[0]
        layers = [(W, R, Bv, "reverse")]
        data = XR.write_lstm_node(W, R, Bv, "reverse", B, T)
        want32 = LR.stack_fp64(xs, layers).astype(np.float32)                       # no torch module walks one direction backwards
    else:
        data = X.torch_export(m, x)
        with torch.no_grad():
            want32 = m(x).numpy()
    ref = LR.stack_fp64(xs, layers, head)
    assert np.abs(ref - want32).max() <= 1e-4                                      # the fp64 helper and the fp32 module describe the same layer
    emu = {fmt: LR.stack_emulated(xs, layers, head, fmt) for fmt in ("bf16", "f16")}
    for v in (xs, ref, want32, *emu.values()):
        v.setflags(write=False)
    _CACHE[name] = (data, x.numpy(), ref, want32, emu)
    return _CACHE[name]


@pytest.fixture(scope="module")
def engines():
    from pdf_table_amd import lib as L
    from pdf_table_amd.engine import HipEngine
    e16, ef = HipEngine(0), HipEngine(0)
    ef.set_precision(L.PT_PRECISION_F16)
    yield {"bf16": e16, "bf16x3": e16, "f16": ef}
    e16.close()
    ef.close()


@pytest.mark.parametrize("precision", ["bf16", "f16", "bf16x3"])
@pytest.mark.parametrize("name", list(CASES))
def test_lstm_layer_against_fp64(engines, name, precision):
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    data, x, ref, want32, emu = _case(name)
    ex = HipGraphExecutor(data, engine=engines[precision], precision=precision)
    assert [l.op for l in ex.layers].count("lstm") == (2 if CASES[name][4] == "stack" else 1)
    got = ex.run(x)[0]
    assert got.shape == ref.shape
    err = float(np.abs(got - ref).max())
    if precision == "bf16x3":
        err32 = float(np.abs(got - want32).max())
        print(f"LSTM {name} bf16x3: max|engine - fp32 module| = {err32:.3e} (vs fp64 {err:.3e})")
        assert err32 <= 1e-3
    else:
        e_emu = float(np.abs(emu[precision] - ref).max())
        print(f"LSTM {name} {precision}: max|engine - fp64| = {err:.3e}, max|emulation - fp64| = {e_emu:.3e}, ratio {err / e_emu:.2f}")
        assert e_emu > 0 and err <= 2 * e_emu
    assert np.array_equal(got, ex.run(x)[0])                                       # operands are cached after the first run


def test_padding_channels_of_y_are_zero(engines):
    """the token rows the kernel writes are [B, 1, T, pad64(D H)]: the channels past D H are read by the next GEMM's zero weight columns and must hold
    zeros, not stale memory"""
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    data, x, ref, _, _ = _case("bi48-b3")
    ex = HipGraphExecutor(data, engine=engines["bf16"])
    nhwc = torch.from_numpy(x).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
    (a,) = ex.run_device(nhwc, x.shape[1])
    assert a.seq and a.tm and a.c == 96 and tuple(a.t.shape) == (3, 1, 5, 128)
    assert not a.t[..., 96:].float().abs().max().item()


def test_graph_replay_equals_the_eager_walk(engines):
    """run_device_graphed: eager, capture, replay -- the LSTM launch is capturable (no allocation, no host synchronisation in pt_op_lstm) and
    gives the same bits"""
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    data, x, _, _, _ = _case("stack48")
    ex = HipGraphExecutor(data, engine=engines["bf16"])
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(3, 1, 6, 40, generator=g).to(torch.bfloat16).cuda() for _ in range(4)]
    want = [ex.values(ex.run_device(v, 40)[0]).clone() for v in xs]
    got = [ex.values(ex.run_device_graphed(v, 40)[0]).clone() for v in xs]
    assert len(ex._graphs) == 1 and not ex._bad
    for w, o in zip(want, got):
        assert torch.equal(w, o)


def test_refusals_name_the_layer_and_the_reason(engines):
    import onnx_export_rnn as XR
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    from pdf_table_amd.onnx_import import UnsupportedOnnxGraph
    g = np.random.default_rng(1)
    W, R, Bv = g.uniform(-.3, .3, (1, 96, 24)).astype(np.float32), g.uniform(-.3, .3, (1, 96, 24)).astype(np.float32), np.zeros((1, 192), np.float32)
    x = g.standard_normal((1, 24, 1, 7)).astype(np.float32)
    for kw, why in (({"initial_h": np.full((1, 1, 24), 0.25, np.float32)}, "non-zero initial_h"), ({"sequence_lens": np.array([7])}, "sequence_lens")):
        ex = HipGraphExecutor(XR.write_lstm_node(W, R, Bv, "forward", 1, 7, **kw), engine=engines["bf16"])
        with pytest.raises(UnsupportedOnnxGraph, match="LSTM_3.*" + why):
            ex.run(x)
    W, R = g.uniform(-.1, .1, (1, 4 * 136, 24)).astype(np.float32), g.uniform(-.1, .1, (1, 4 * 136, 136)).astype(np.float32)
    for precision in ("bf16", "bf16x3"):
        ex = HipGraphExecutor(XR.write_lstm_node(W, R, None, "forward", 1, 7), engine=engines[precision], precision=precision)
        with pytest.raises(UnsupportedOnnxGraph, match="136 hidden units.*" + precision):
            ex.run(x)
