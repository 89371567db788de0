"""Host half of the generic executor's LSTM layer (pdf_table_amd/onnx_exec.py, csrc/lstm_op.hip): the references the GPU tests rely on
(tests/onnx_lstm_ref.py) against the CPU oracle, the packing of the recurrent weights into MFMA operand order, the zero padding of the hidden
units, and what the importer hands the executor for forward / reverse / bidirectional and dynamic-batch exports.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import onnx_lstm_ref as LR  # noqa: E402

# (H, I, T, B, directions): the shapes of tests/test_gpu_onnx_lstm.py
SHAPES = [(48, 40, 5, 3, "bidirectional"), (48, 40, 5, 17, "bidirectional"), (128, 64, 4, 2, "bidirectional"), (24, 24, 7, 1, "reverse"),
          (24, 24, 7, 1, "forward"), (48, 40, 1, 3, "bidirectional")]


def _case(H, I, T, B, direction, seed=0):
    g = np.random.default_rng(seed)
    D = 2 if direction == "bidirectional" else 1
    s = 2.5 / np.sqrt(H)
    return (g.standard_normal((T, B, I)).astype(np.float32), g.uniform(-s, s, (D, 4 * H, I)).astype(np.float32),
            g.uniform(-s, s, (D, 4 * H, H)).astype(np.float32), g.uniform(-0.5, 0.5, (D, 8 * H)).astype(np.float32))


@pytest.mark.parametrize("H,I,T,B,direction", SHAPES)
def test_references_agree_with_the_oracle(H, I, T, B, direction):
    """the emulation with every rounding switched off, and the fp64 evaluation, against oracle/onnx_ref._lstm (fp32 torch): fp32 round-off.
    Bound: a gate pre-activation is a sum of I + H <= 192 products, each term within 2^-24 relative of |g| <= ~10 in fp32 -> <= 1.2e-4 worst
    case per step before the (contracting) sigmoid / tanh; 1e-4 on |h| <= 1."""
    from oracle.onnx_ref import _lstm
    X, W, R, Bv = _case(H, I, T, B, direction)
    want = _lstm([torch.from_numpy(v) for v in (X, W, R, Bv)], {"hidden_size": H, "direction": direction})[0].numpy()
    got = LR.lstm_emulated(X, W, R, Bv, direction, fmt=None)
    ref = LR.lstm_fp64(X, W, R, Bv, direction)
    assert got.shape == want.shape == ref.shape == (T, 2 if direction == "bidirectional" else 1, B, H)
    assert np.abs(got - want).max() <= 1e-4 and np.abs(ref - want).max() <= 1e-4
    assert np.abs(want).max() > 0.5                                   # the gates do leave their linear range


@pytest.mark.parametrize("fmt,eps", [("bf16", 2.0 ** -8), ("f16", 2.0 ** -11)])
def test_emulation_rounds_to_the_storage_format(fmt, eps):
    X, W, R, Bv = _case(48, 40, 5, 3, "bidirectional")
    y = LR.lstm_emulated(X, W, R, Bv, "bidirectional", fmt=fmt)
    assert np.array_equal(y, LR.round_to(y, fmt).numpy())              # h is stored in the format
    err = np.abs(y - LR.lstm_fp64(X, W, R, Bv, "bidirectional")).max()
    assert 0 < err <= 64 * eps                                         # a 16-bit effect, not a different recurrence


@pytest.mark.parametrize("H,D", [(24, 1), (48, 2), (50, 2), (128, 2), (7, 1)])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_r_packer_round_trips(H, D, fmt):
    from pdf_table_amd import lib as L
    from pdf_table_amd.build import build
    from pdf_table_amd.weights import lstm_padded_sizes, pack_lstm_r, unpack_lstm_r
    R = np.random.default_rng(H).uniform(-1, 1, (D, 4 * H, H)).astype(np.float32)
    Hp, KS = lstm_padded_sizes(H)
    p = pack_lstm_r(R, fmt)
    assert p.dtype == np.uint16 and p.shape == (D, 1, (Hp // 16) * 4 * KS, 64, 8)
    assert np.array_equal(unpack_lstm_r(p, H, fmt), LR.round_to(R, fmt).numpy())
    # the operand order csrc/lstm_op.hip reads: fragment (ub * 4 + gate) * KS + kk, lane l, element j
    bits = lambda v: LR.round_to(np.float32(v), fmt).to(LR._DT[fmt]).view(torch.int16).numpy().view(np.uint16)
    for d, ub, gate, kk, lane, j in [(0, 0, 0, 0, 0, 0), (D - 1, Hp // 16 - 1, 3, KS - 1, 63, 7), (0, 0, 2, 0, 37, 5), (D - 1, (Hp // 16) // 2, 1, KS // 2, 18, 3)]:
        unit, k = ub * 16 + (lane & 15), kk * 32 + 8 * (lane >> 4) + j
        want = bits(R[d, gate * H + unit, k]) if unit < H and k < H else np.uint16(0)
        assert p[d, 0, (ub * 4 + gate) * KS + kk, lane, j] == want
    build(verbose=False)
    lib = L.load()
    assert lib.pt_op_lstm_packed_elems(H, D, 0) == p.size
    if fmt == "bf16":                                                  # the tolerance mode's two halves: hi + lo carries 16 significant bits
        p2 = pack_lstm_r(R, fmt, split=True)
        assert p2.shape == (D, 2) + p.shape[2:] and np.array_equal(p2[:, 0], p[:, 0]) and lib.pt_op_lstm_packed_elems(H, D, 1) == p2.size
        assert np.abs(unpack_lstm_r(p2, H, fmt) - R).max() <= 2.0 ** -16
    assert lib.pt_op_lstm_packed_elems(136, 2, 0) == 0


@pytest.mark.parametrize("H,I", [(24, 24), (50, 40), (48, 40)])
def test_zero_padded_hidden_units_stay_zero(H, I):
    """the executor pads H to Hp = a multiple of 16 with zero rows of W, zero rows and columns of R and zero bias (onnx_exec.lstm_gemm_operands,
    weights.pack_lstm_r).  The LSTM of Hp units those operands describe, run through the emulation: padded units are exactly 0 in every step and
    the real units are bit for bit those of the unpadded layer."""
    from pdf_table_amd.onnx_exec import lstm_gemm_operands
    from pdf_table_amd.weights import lstm_padded_sizes, pack_lstm_r, unpack_lstm_r
    X, W, R, Bv = _case(H, I, 6, 3, "bidirectional", seed=3)
    Hp, KS = lstm_padded_sizes(H)
    wp, bp = lstm_gemm_operands(W, Bv, 64)
    assert tuple(wp.shape) == (2 * 4 * Hp, 64, 1, 1)
    Wp = wp[:, :I, 0, 0].numpy().reshape(2, 4 * Hp, I)
    Bp = np.concatenate([bp.numpy().reshape(2, 4 * Hp), np.zeros((2, 4 * Hp), np.float32)], 1)
    # R of the padded layer, read back from the packed image: fragment element (unit, k) for every unit, k < Hp
    p = pack_lstm_r(R, "bf16")[:, 0].reshape(2, Hp // 16, 4, KS, 64, 8)
    Rp = np.zeros((2, 4 * Hp, Hp), np.float32)
    vals = torch.from_numpy(p.view(np.int16).copy()).view(torch.bfloat16).float().numpy()
    for lane in range(64):
        for j in range(8):
            for kk in range(KS):
                k = kk * 32 + 8 * (lane >> 4) + j
                if k < Hp:
                    for g in range(4):
                        Rp[:, g * Hp + (lane & 15) + 16 * np.arange(Hp // 16), k] = vals[:, :, g, kk, lane, j]
    assert np.array_equal(Rp.reshape(2, 4, Hp, Hp)[:, :, :H, :H], unpack_lstm_r(pack_lstm_r(R, "bf16"), H).reshape(2, 4, H, H))
    yp = LR.lstm_emulated(X, Wp, Rp, Bp, "bidirectional", "bf16")
    y = LR.lstm_emulated(X, W, R, Bv, "bidirectional", "bf16")
    assert yp.shape[-1] == Hp and np.array_equal(yp[..., :H], y)
    assert not yp[..., H:].any()


def _lstm_layers(data):
    from pdf_table_amd.onnx_import import load_onnx
    g = load_onnx(data)
    return g, [l for l in g.layers() if l.op == "lstm"]


def test_importer_yields_lstm_layers_for_every_direction():
    import onnx_export as X
    import onnx_export_rnn as XR
    from pdf_table_amd.onnx_import import UnsupportedOnnxGraph, recognise
    for bid in (False, True):
        m = XR.seeded_rnn(XR.LstmOnly(24, 24, bidirectional=bid), 3)
        g, (lay,) = _lstm_layers(X.torch_export(m, torch.zeros(1, 24, 1, 7)))
        W, R, B, direction = XR.onnx_lstm_params(m.rnns[0])
        assert g.unsupported_ops() == [] and lay.attrs["hidden_size"] == 24 and lay.attrs["direction"] == direction
        assert np.array_equal(lay.extra["W"], W) and np.array_equal(lay.extra["R"], R) and np.array_equal(lay.extra["B"], B)
        assert lay.attrs["all_inputs"][0] == lay.inputs[0] and lay.attrs["all_outputs"][0] == lay.outputs[0] and "hidden_size" in lay.attrs["node_attrs"]
        with pytest.raises(UnsupportedOnnxGraph):
            recognise(g)                                              # not the 256-unit in-tree CRNN: the generic executor's graph
    Xc, W, R, Bv = _case(24, 24, 7, 1, "reverse")
    data = XR.write_lstm_node(W, R, Bv, "reverse", 1, 7)
    g, (lay,) = _lstm_layers(data)
    assert lay.attrs["direction"] == "reverse" and lay.attrs["all_inputs"][:4] == ["xt", "W", "R", "B"]
    # the hand-built graph means what the operator definition says (oracle: the CPU graph reference)
    from oracle import onnx_ref
    x_map = np.ascontiguousarray(Xc.transpose(1, 2, 0))[:, :, None, :]                 # [B, I, 1, T]
    got = onnx_ref.run(g.model, {"x": x_map})[0]
    assert np.abs(got - LR.merge_directions(LR.lstm_fp64(Xc, W, R, Bv, "reverse"))).max() <= 1e-4
    g, (lay,) = _lstm_layers(XR.write_lstm_node(W, R, Bv, "forward", 1, 7, initial_h=np.full((1, 1, 24), 0.25, np.float32), sequence_lens=np.array([7])))
    assert lay.attrs["all_inputs"][4:6] == ["sequence_lens", "initial_h"]


def _host_walk(data, x_shape):
    """the executor's host side only (no engine): shape plumbing folded over index arrays, every LSTM layer planned; device layers are
    stood in for by token rows of the right shape.  -> [(layer, plan)]"""
    from pdf_table_amd.onnx_exec import HipGraphExecutor, _Act, _View
    from pdf_table_amd.onnx_import import load_onnx
    ex = HipGraphExecutor.__new__(HipGraphExecutor)
    ex.graph = load_onnx(data)
    ex.layers = ex.graph.layers()
    ex.outputs = [o.name for o in ex.graph.model.outputs]
    ex.precision, ex.split, ex.m = "bf16", False, 1
    ex._read = {nm for l in ex.layers for nm in list(l.inputs) + list(l.attrs.get("all_inputs", ())) if nm} | set(ex.outputs)
    B, I, _, T = x_shape
    (inp,) = [i for i in ex.graph.model.inputs if i.name not in ex.graph.init]
    env = {inp.name: _Act(torch.zeros(B, 1, T, 64, dtype=torch.bfloat16), I)}
    plans = []
    for lay in ex.layers:
        if ex._host_layer(lay, env):
            continue
        assert lay.op == "lstm", lay.op
        H, Hp, D, reverse, y_name = ex._lstm_plan(lay, env)
        x = ex._time_major_rows(env[lay.attrs["all_inputs"][0]], lay.name)
        assert x is not None and x.shape() == (B, T, lay.extra["W"].shape[2])
        y = _Act(torch.zeros(B, 1, T, 128, dtype=torch.bfloat16), D * H, seq=True)
        idx = ((np.arange(B)[None, None, :, None] * T + np.arange(T)[:, None, None, None]) * (D * H) + np.arange(D)[None, :, None, None] * H
               + np.arange(H)[None, None, None, :])
        env[y_name] = _View(y, idx)
        plans.append((lay, (H, Hp, D, reverse)))
    assert ex._time_major_rows(env[ex.outputs[0]], "y") is not None            # the Transpose + Reshape after Y moved no data
    return plans


def test_dynamic_batch_export_folds_the_zero_initial_states():
    """with a symbolic batch axis torch writes h_0 / c_0 as Shape -> Gather -> ... -> ConstantOfShape / Expand: computed inputs of the node that
    the executor's host walk folds to zero constants per input shape"""
    import onnx_export as X
    import onnx_export_rnn as XR
    m = XR.seeded_rnn(XR.LstmOnly(40, 48, bidirectional=True, layers=2), 5)
    data = X.torch_export(m, torch.zeros(2, 40, 1, 6), dynamic_batch=True)
    g, lays = _lstm_layers(data)
    assert len(lays) == 2
    dyn = [l for l in lays if len(l.attrs["all_inputs"]) > 5 and l.attrs["all_inputs"][5] and l.attrs["all_inputs"][5] not in g.init]
    assert dyn, "the exporter no longer writes computed initial states: this test needs another producer"
    for B in (3, 17):
        plans = _host_walk(data, (B, 40, 1, 6))
        assert [p for _, p in plans] == [(48, 48, 2, False)] * 2


def test_host_plan_refusals():
    import onnx_export_rnn as XR
    from pdf_table_amd.onnx_import import UnsupportedOnnxGraph
    _, W, R, Bv = _case(24, 24, 7, 1, "forward")
    assert [p for _, p in _host_walk(XR.write_lstm_node(W, R, Bv, "reverse", 1, 7), (1, 24, 1, 7))] == [(24, 32, 1, True)]
    zero = np.zeros((1, 1, 24), np.float32)
    assert _host_walk(XR.write_lstm_node(W, R, Bv, "forward", 1, 7, initial_h=zero, initial_c=zero), (1, 24, 1, 7))[0][1] == (24, 32, 1, False)
    with pytest.raises(UnsupportedOnnxGraph, match="LSTM_3.*non-zero initial_h"):
        _host_walk(XR.write_lstm_node(W, R, Bv, "forward", 1, 7, initial_h=zero + 0.25), (1, 24, 1, 7))
    with pytest.raises(UnsupportedOnnxGraph, match="LSTM_3.*sequence_lens"):
        _host_walk(XR.write_lstm_node(W, R, Bv, "forward", 1, 7, sequence_lens=np.array([7])), (1, 24, 1, 7))
    _, W, R, Bv = _case(136, 24, 2, 1, "forward")
    with pytest.raises(UnsupportedOnnxGraph, match="136 hidden units"):
        _host_walk(XR.write_lstm_node(W, R, Bv, "forward", 1, 2), (1, 24, 1, 2))
