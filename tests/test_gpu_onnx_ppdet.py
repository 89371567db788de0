"""PP-OCRv4 mobile detector blocks through the generic ONNX executor (pdf_table_amd/onnx_exec.py, csrc/det_ops.hip): the ``LcnetV3DetLike`` stand-in of
tools/onnx_export_ppdet.py (PP-LCNetV3 with its LearnableAffineBlocks, RSE-FPN, DB head -- the layer geometry, not the shipped graph) against the fp32
PyTorch module, with the DB head's tail layer by layer and as one fused launch (``fuse_db_tail``); a three-block graph that isolates the importer's
constant-affine rules; and head patterns that must NOT fuse.

Bounds on the probability map: precision "bf16x3" (what the tasks call "fp32") holds the executor's contract, 1e-3; "bf16" and "f16" use the bound
tests/test_gpu_onnx_exec.py::test_fpn_like_detector uses for this class of graph -- ``d <= 4e-2 * scale + 1e-3`` with scale = max |module output| (at most
1 for a probability).  The fused result is compared with the layered one of the same precision under the same bound."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

BOUNDS = {"bf16x3": lambda scale: 1e-3, "bf16": lambda scale: 4e-2 * scale + 1e-3, "f16": lambda scale: 4e-2 * scale + 1e-3}


@pytest.fixture(scope="module")
def engs():
    """one engine per 16-bit storage format, made on first use"""
    from pdf_table_amd import lib as L
    from pdf_table_amd.engine import HipEngine
    made = {}

    def get(precision):
        key = "f16" if precision == "f16" else "bf16"
        if key not in made:
            made[key] = HipEngine(0)
            if key == "f16":
                made[key].set_precision(L.PT_PRECISION_F16)
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def det():
    """the exported stand-in, its input and the fp32 module's output -- computed once.  Seed 3, chosen on the CPU from the fp32 module alone: on this input
    its logits have the spread the stand-in is scaled for (mean -2.8, standard deviation 1.5, range -9 .. 3); seed 2 gives a standard deviation of 5 .. 7 on
    the same input, a map that is saturated almost everywhere, and a module that moves by 0.7 when only its PARAMETERS are rounded to bf16 (seed 3: 0.03)"""
    import onnx_export_ppdet as D
    m = D.seeded_ppdet(D.LcnetV3DetLike(), 3)
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        want = m(x).numpy()
    return D.torch_export(m, x), x, want


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "f16"])
def test_lcnetv3_det_like(engs, det, precision):
    """On the parent this raises UnsupportedOnnxGraph: '... Mul with a constant operand' at the first block.

    The error scales with the unit round-off of the storage format (bf16x3 : f16 : bf16), as the rounding of some 116 layers does; FpnLike, which the
    16-bit bound is quoted from, has 14.  Measured on the MI355X, max |dprob| layered / fused / fused against
    layered: bf16x3 3.2e-5 / 3.1e-5 / 1.8e-5, f16 2.1e-3 / 2.1e-3 / 7.7e-4, bf16 2.4e-2 / 2.4e-2 / 8.4e-3 (bound 3.9e-2).  With seed 2 (see the fixture)
    bf16 measured 1.4e-1 and missed the bound; bf16x3 and f16 met it."""
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    blob, x, want = det
    eng = engs(precision)
    scale = float(np.abs(want).max())
    bound = BOUNDS[precision](scale)
    got = {}
    for fuse in (False, True):
        ex = HipGraphExecutor(blob, engine=eng, precision=precision, fuse_db_tail=fuse)
        assert len(ex._tail) == int(fuse)
        assert sum(1 for l in ex.layers if l.op == "affine") == 14 and sum(1 for l in ex.layers if l.attrs.get("affine_folded")) == 28
        (y,) = ex.run(x.numpy())
        assert y.shape == want.shape and y.dtype == np.float32
        d = float(np.abs(y - want).max())
        print(f"LcnetV3DetLike [{precision}, fuse_db_tail={fuse}]: max|dprob| = {d:.3e} (bound {bound:.3e}; module output in [{want.min():.4f}, {want.max():.4f}])")
        got[fuse] = (y, d)
        # the captured graph replays the same kernels with the same arguments: the same bits
        nhwc = x.permute(0, 2, 3, 1).contiguous().to(eng._tdev)
        nhwc = nhwc if ex.split else nhwc.to(ex.adt)
        (a,) = ex.run_device(nhwc, 3)
        eager = a.t.clone()
        assert a.t.dtype == (torch.float32 if fuse else ex.adt)
        for _ in range(3):                              # eager, capture, replay
            (g,) = ex.run_device_graphed(nhwc, 3)
            torch.cuda.synchronize()
            assert torch.equal(g.t, eager)
        assert len(ex._graphs) == 1 and not ex._bad
    dfl = float(np.abs(got[True][0] - got[False][0]).max())
    print(f"LcnetV3DetLike [{precision}]: max|fused - layered| = {dfl:.3e}")
    assert got[False][1] <= bound and got[True][1] <= bound and dfl <= bound


def _run_rules(eng, precision, reversed_sub=False):
    import onnx_export_ppdet as D
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    m = D.seeded_ppdet(D.AffineRulesLike(reversed_sub=reversed_sub), 5)
    x = torch.randn(2, 3, 18, 26, generator=torch.Generator().manual_seed(3))
    ex = HipGraphExecutor(D.torch_export(m, x), engine=eng, precision=precision)
    with torch.no_grad():
        want = m(x).numpy()
    return ex, ex.run(x.numpy())[0], want


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_affine_rules(engs, precision):
    """conv -> LAB folds (and the hardswish behind it fuses into the epilogue); hardswish -> LAB and relu -> LAB run on pt_op_affine_act, the ReLU in the
    same launch; a chain of five nodes is one launch; the last affine sits in front of a ZERO-PADDED 3x3 convolution, where folding it forward would
    be wrong at the border -- the whole output, border included, is compared"""
    ex, got, want = _run_rules(engs(precision), precision)
    kinds = [(l.op, l.act, l.attrs.get("affine_folded"), l.attrs.get("act"), l.attrs.get("nodes")) for l in ex.layers]
    assert kinds == [("conv", "hardswish", 2, None, None), ("affine", None, None, None, 2), ("conv", None, None, None, None), ("add", None, None, None, None),
                     ("affine", None, None, "relu", 2), ("avgpool", None, None, None, None), ("affine", None, None, None, 5), ("conv", None, None, None, None)]
    scale = float(np.abs(want).max())
    d = float(np.abs(got - want).max())
    print(f"AffineRulesLike [{precision}]: max|d| = {d:.3e} on scale {scale:.2f}")
    assert got.shape == want.shape and d <= (1e-3 if precision == "bf16x3" else 4e-2) * scale + 1e-3


def test_reversed_sub_is_refused_by_name(engs):
    from pdf_table_amd.onnx_import import UnsupportedOnnxGraph
    with pytest.raises(UnsupportedOnnxGraph, match=r"Sub with the constant as its first operand \(c - x"):
        _run_rules(engs("bf16"), "bf16", reversed_sub=True)


class _Head(nn.Module):
    """Conv3x3 -> ConvT 2x2 / 2 (-> mid) + ReLU -> ConvT 2x2 / 2 (-> 1) -> Sigmoid; ``also``: the ReLU's output is a second graph output (a second
    reader of the intermediate); ``pool``: the Sigmoid is not the graph output"""

    def __init__(self, mid=16, also=False, pool=False):
        super().__init__()
        self.also, self.pool = also, pool
        self.conv = nn.Sequential(nn.Conv2d(3, 24, 3, 1, 1), nn.ReLU())
        self.up1, self.up2 = nn.ConvTranspose2d(24, mid, 2, 2), nn.ConvTranspose2d(mid, 1, 2, 2)

    def forward(self, x):
        h = torch.relu(self.up1(self.conv(x)))
        p = torch.sigmoid(self.up2(h))
        if self.pool:
            return nn.functional.max_pool2d(p, 2)
        return (p, h) if self.also else p


@pytest.mark.parametrize("case", ["fuses", "mid96", "second_reader", "not_the_output"])
def test_only_the_pattern_fuses(engs, case):
    """the flag replaces exactly the pattern: 65 or more channels between the transposed convolutions (a 96-channel head), a second reader of the
    intermediate, or a Sigmoid that is not the graph's output keep the layered route -- and then the flag changes no bit"""
    from onnx_export import torch_export
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    torch.manual_seed(11)
    m = _Head(mid=96 if case == "mid96" else 16, also=case == "second_reader", pool=case == "not_the_output").eval()
    x = torch.randn(2, 3, 10, 14)
    if case == "second_reader":
        import torch.onnx as tonnx
        from torch.onnx._internal.torchscript_exporter import utils as TU      # two outputs: torch_export names one
        from torch.onnx._internal.torchscript_exporter._globals import GLOBALS
        GLOBALS.export_onnx_opset_version = 13
        with torch.no_grad():
            graph, params, _ = TU._model_to_graph(m, (x,), False, ["x"], ["y", "h"], tonnx.OperatorExportTypes.ONNX, True, dynamic_axes={})
        blob = bytes(graph._export_onnx(params, 13, {}, False, tonnx.OperatorExportTypes.ONNX, True, True, {}, True, "", {})[0])
    else:
        blob = torch_export(m, x)
    eng = engs("bf16")
    off, on = HipGraphExecutor(blob, engine=eng), HipGraphExecutor(blob, engine=eng, fuse_db_tail=True)
    y_off, y_on = off.run(x.numpy()), on.run(x.numpy())
    with torch.no_grad():
        want = m(x)
    want = [w.numpy() for w in (want if isinstance(want, tuple) else (want,))]
    assert not off._tail and len(on._tail) == (1 if case == "fuses" else 0)
    for a, b, w in zip(y_off, y_on, want):
        assert a.shape == b.shape == w.shape
        assert np.abs(b - w).max() <= 4e-2 * float(np.abs(w).max()) + 1e-3
        if case != "fuses":
            assert np.array_equal(a, b)
