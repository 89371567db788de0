"""Recogniser-shaped graphs through the generic ONNX executor (pdf_table_amd/onnx_exec.py): convolutions whose stride differs per axis, 1x3 / 3x1
kernels and rectangular pools on pt_op_conv2d_rect / pt_op_dwconv_rect / pt_op_pool_rect (csrc/rect_ops.hip, ABI 18).  The graphs are the stand-ins of
tools/onnx_export_pprec.py from PyTorch's own exporter; the checker is the module itself in fp32 (and oracle/onnx_ref on the exported bytes within
1e-4 wherever that interpreter has the graph's operators: it has no ReduceMean, so the decomposed LayerNorm of the SVTR neck is checked against the
module only).  Tolerances of tests/test_gpu_onnx_exec.py: 4e-2 of the output scale in bf16 / f16, 1e-3 in bf16x3."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _check(model, x, eng, tol_rel, precision="bf16", dynamic_batch=False):
    """test_gpu_onnx_exec.py::_check with an engine per storage format and an oracle that may lack an operator"""
    from onnx_export import torch_export
    from oracle import onnx_ref
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    from pdf_table_amd.onnx_proto import parse_model
    blob = torch_export(model, x, dynamic_batch=dynamic_batch)
    ex = HipGraphExecutor(blob, engine=None if precision == "f16" else eng, precision=precision)
    try:
        (got,) = ex.run(x.numpy())
        (again,) = ex.run(x.numpy())                      # operands are cached after the first run
        with torch.no_grad():
            want = model(x).numpy()
        scale = float(np.abs(want).max())
        try:
            (ref,) = onnx_ref.run(parse_model(blob), {ex.inputs[0].name: x.numpy()})
            assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-4 * max(scale, 1.0)        # the exported graph is the module
        except NotImplementedError as e:
            assert "ReduceMean" in str(e)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(got, again)
        d = float(np.abs(got - want).max())
        print(f"{type(model).__name__} [{precision}]: max|d| = {d:.3e} on scale {scale:.2f} ({len(ex.layers)} layers)")
        assert d <= tol_rel * scale + 1e-3
    finally:
        if precision == "f16":
            ex.eng.close()
    return ex


def _geometry(ex):
    convs = [l for l in ex.layers if l.op == "conv"]
    return {"strides": {tuple(l.attrs["strides"]) for l in convs}, "kernels": {tuple(l.attrs["kernel"]) for l in convs},
            "avgpool": {tuple(l.attrs["kernel"]) for l in ex.layers if l.op == "avgpool"},
            "maxpool": {tuple(l.attrs["kernel"]) for l in ex.layers if l.op == "maxpool"}}


@pytest.mark.parametrize("precision,tol", [("bf16", 4e-2), ("bf16x3", 1e-3)])
def test_resvd_like_blocks(eng, precision, tol):
    """dense 3x3 of stride (2,1) twice, a [3,1] convolution that is not folded with its Add, an AvgPool((2,1), ceil_mode=True) shortcut on an even
    height, a shortcut written as a 1x1 convolution of stride (2,1), a residual folded into the square 3x3 that follows a rectangular one"""
    import onnx_export_pprec as P
    torch.manual_seed(0)
    m = P.seeded_pprec(P.ResVdRecLike(), 3)
    ex = _check(m, torch.randn(2, 3, 32, 48), eng, tol, precision)
    geo = _geometry(ex)
    assert (2, 1) in geo["strides"] and (3, 1) in geo["kernels"] and (2, 1) in geo["avgpool"]
    rect = [k for k, l in enumerate(ex.layers) if l.op == "conv" and ex._is_rect(l)]
    assert len(rect) == 4 and not any(k in ex._fuse for k in rect)          # pt_op_conv2d_rect has no residual operand: conv -> add -> ReLU


@pytest.mark.parametrize("precision,tol", [("bf16", 4e-2), ("f16", 4e-2), ("bf16x3", 1e-3)])
def test_svtr_lcnet_like_recogniser(eng, precision, tol):
    """depthwise strides (2,1) and (1,2), 5x5 (2,1), avg_pool2d (3, 2) on three rows, the [1,3] neck convolutions on the one-row map around two
    token-mixing blocks, Concat of 120 + 120 channels; dynamic batch"""
    import onnx_export_pprec as P
    torch.manual_seed(0)
    m = P.seeded_pprec(P.SvtrLcnetRecLike(), 3, head_scale=6.0)
    ex = _check(m, torch.randn(2, 3, 48, 64), eng, tol, precision, dynamic_batch=True)
    geo = _geometry(ex)
    assert {(2, 1), (1, 2)} <= geo["strides"] and (1, 3) in geo["kernels"] and (3, 2) in geo["avgpool"]


def test_mobilev3_like_recogniser(eng):
    """inverted-residual blocks with depthwise strides (2,1), MaxPool2d(2) on three rows (floor), two BiLSTMs"""
    import onnx_export_pprec as P
    torch.manual_seed(0)
    m = P.seeded_pprec(P.MobileV3RecLike(), 2)
    ex = _check(m, torch.randn(3, 3, 48, 64), eng, 4e-2, dynamic_batch=True)
    geo = _geometry(ex)
    assert (2, 1) in geo["strides"] and (2, 2) in geo["maxpool"] and [l.op for l in ex.layers].count("lstm") == 2


def test_mobilev3_like_logits_tolerance_mode(eng):
    """the LOGITS (the graph without its Softmax) in bf16x3 within 1e-3 of the fp32 module; the max pool does run on a map of three rows"""
    import onnx_export_pprec as P
    from onnx_export import torch_export
    from pdf_table_amd.onnx_exec import HipGraphExecutor

    class Logits(nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, x):
            return self.net.logits(x)
    torch.manual_seed(0)
    m = P.seeded_pprec(P.MobileV3RecLike(), 2)
    x = torch.randn(3, 3, 48, 64)
    ex = HipGraphExecutor(torch_export(Logits(m).eval(), x, dynamic_batch=True), engine=eng, precision="bf16x3")
    seen = {}
    real = eng.op_pool_rect

    def spy(t, kind, kh, kw, split=False):
        seen["pool"] = (tuple(t.shape[1:3]), kind, kh, kw)
        return real(t, kind, kh, kw, split=split)
    eng.op_pool_rect = spy
    try:
        (got,) = ex.run(x.numpy())
    finally:
        del eng.op_pool_rect
    with torch.no_grad():
        want = m.logits(x).numpy()
    d = float(np.abs(got - want).max())
    print(f"MobileV3RecLike logits [bf16x3]: max|d| = {d:.3e} on scale {float(np.abs(want).max()):.2f}")
    assert got.shape == want.shape == (3, 16, 97) and d <= 1e-3
    assert seen["pool"] == ((3, 32), 0, 2, 2)


def test_graph_replay_equals_the_eager_walk(eng):
    """run_device_graphed: the first call walks eagerly, the second captures, the third replays -- the new entry points allocate nothing and do not
    synchronise, so the capture succeeds and every call gives the bits of run()"""
    import onnx_export_pprec as P
    from onnx_export import torch_export
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    torch.manual_seed(0)
    m = P.seeded_pprec(P.SvtrLcnetRecLike(), 3, head_scale=6.0)
    x = torch.randn(2, 3, 48, 64)
    ex = HipGraphExecutor(torch_export(m, x, dynamic_batch=True), engine=eng)
    (want,) = ex.run(x.numpy())
    nhwc = x.permute(0, 2, 3, 1).contiguous().to(eng._tdev).to(ex.adt)
    outs = []
    for _ in range(3):
        (a,) = ex.run_device_graphed(nhwc, 3)
        outs.append(ex.values(a)[:, 0].cpu().numpy().copy())
    assert len(ex._graphs) == 1 and not ex._bad, "the capture failed: some layer allocates or synchronises"
    assert np.array_equal(outs[1], outs[2]) and np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], want)


def test_square_graphs_do_not_touch_the_new_entry_points(eng, monkeypatch):
    """no behaviour change: with the three new wrappers patched to raise, the square graphs of test_gpu_onnx_exec.py still run and pass their bounds"""
    import test_gpu_onnx_exec as T

    def boom(*a, **k):
        raise AssertionError("a square graph reached a rect entry point")
    for name in ("op_conv2d_rect", "op_dwconv_rect", "op_pool_rect"):
        monkeypatch.setattr(eng, name, boom)
    torch.manual_seed(0)
    T._check(T._randomise(T.LcNetLike(), 1), torch.randn(3, 3, 64, 96), eng, 4e-2)
    torch.manual_seed(0)
    T._check(T._randomise(T.FpnLike(), 2), torch.randn(2, 3, 64, 96), eng, 4e-2)
    torch.manual_seed(0)
    T._check(T._randomise(T.VdLike(), 4), torch.randn(2, 3, 32, 64), eng, 4e-2)


def test_still_refused(eng):
    """each with a message naming the layer"""
    from onnx_export import torch_export
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    from pdf_table_amd.onnx_import import UnsupportedOnnxGraph

    def refuse(mod, shape, match):
        ex = HipGraphExecutor(torch_export(mod.eval(), torch.randn(*shape)), engine=eng)
        with pytest.raises(UnsupportedOnnxGraph, match=match):
            ex.run(np.zeros(shape, np.float32))
    refuse(nn.Conv2d(3, 8, 3, 1, 2, dilation=2), (1, 3, 16, 16), r"Conv.*(dilation|padding)")
    refuse(nn.Conv2d(3, 8, 5, 1, 2), (1, 3, 16, 16), r"Conv.*dense 5x5")
    refuse(nn.Conv2d(3, 8, 3, (3, 1), 1), (1, 3, 16, 16), r"Conv.*stride")
    refuse(nn.Conv2d(3, 8, (1, 3), 1, 0), (1, 3, 16, 16), r"Conv.*padding")
    refuse(nn.Conv2d(8, 8, 3, (2, 1), 1, groups=2), (1, 8, 16, 16), r"Conv.*grouped")
    refuse(nn.AvgPool2d(2, 1), (1, 8, 16, 16), r"AveragePool.*stride = window")
    refuse(nn.MaxPool2d((2, 1), ceil_mode=True), (1, 8, 3, 16), r"MaxPool.*ceil_mode")
    refuse(nn.MaxPool2d((5, 1)), (1, 8, 10, 16), r"MaxPool.*1 \.\. 4")
