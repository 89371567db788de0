"""The PP-OCRv4 SERVER detector stand-in of tools/onnx_export_ppdet_server.py (``HgnetLkpanDetLike``: PP-HGNet-like backbone, LKPAN neck with 9x9
kernels and IntraCL blocks, PFHeadLocal) through ``HipGraphExecutor`` and through the product door ``OcrDetectionTask(model="db_pp", task_path=...,
server_model=True)``, on [2, 3, 96, 128]: the 1/32 level is 3 x 4, so the 9x9 layers run on a map smaller than their kernel.  The real ``*_infer`` file
is not available offline: this is a seeded module with the model's layer geometry.  Checker: the fp32 module on the oracle's pre-processing of the same
pixels.

Seed and box threshold were chosen on the CPU from the fp32 module and the oracle's own post-processing alone: with ``blob_map=True`` seeding, seed 7
puts 8.5 % of the first page above thresh = 0.3 and with box_thresh = 0.3 the oracle returns 7 boxes, the same 7 under four random perturbations of the
map by up to 1e-3 (the tolerance mode's bound), so the comparison corner for corner is not decided by a pixel on the threshold.

16-bit modes: no bound chosen in advance.  The layered torch module run in the same 16-bit dtype on the CPU is measured against the fp32 module on the
same input (on this input: bf16 7.3e-2 .. 1.0e-1 depending on the host's convolution kernels, fp16 8.4e-3 .. 8.7e-3; measured on the engine: bf16
6.1e-2, fp16 7.3e-3, tolerance mode 8.2e-5) and the executor must stay within 4 times that (the summation order differs, and the executor folds
BatchNorm where the module rounds once more)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

SEED, BOX_THRESH, BOXES_ORACLE = 7, 0.3, 7
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def server(tmp_path_factory):
    """a directory with model.onnx, two synthetic pages, the oracle's pre-processed pixels, the module's fp32 map on them and the distance of the
    module run in each 16-bit dtype on the CPU from that map -- computed once, shared by every test, never changed"""
    import onnx_export_ppdet_server as S
    from oracle import db_post, db_pre
    from pdf_table_amd.synth_pages import make_page
    pages = [make_page(2)[0][:96, :128].copy(), make_page(3)[0][200:296, 100:228].copy()]
    pre = [db_pre.preprocess_db_pp(p) for p in pages]
    pix = torch.from_numpy(np.stack([c for c, _ in pre]))
    assert tuple(pix.shape) == (2, 3, 96, 128)
    m = S.seeded_ppdet_server(S.HgnetLkpanDetLike(), SEED, example=pix, blob_map=True)
    d = tmp_path_factory.mktemp("ppocrv4_det_server")
    blob = S.torch_export(m, torch.zeros(1, 3, 64, 64))
    (d / "model.onnx").write_bytes(blob)
    with torch.no_grad():
        want = m(pix)[:, 0].numpy()
        d16 = {k: float(np.abs(copy.deepcopy(m).to(dt)(pix.to(dt))[:, 0].float().numpy() - want).max()) for k, dt in DTYPES.items()}
    ref_boxes = db_post.db_postprocess(want[0], pre[0][1], pages[0].shape, 0.3, BOX_THRESH)
    assert len(ref_boxes) == BOXES_ORACLE and BOXES_ORACLE >= 3
    return dict(dir=d, blob=blob, pages=pages, pix=pix, want=want, d16=d16, ref_boxes=ref_boxes, module=m)


def _rows(b):
    b = np.asarray(b, np.float64).reshape(-1, 8)
    return b[np.lexsort(b.T[::-1])]


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "f16"])
def test_executor(server, precision):
    """through HipGraphExecutor.run: the tolerance mode within the executor's 1e-3 of the fp32 module; the 16-bit modes within 4 times what the layered
    torch module in the same dtype on the CPU gives on the same input.  Every large dense layer went to pt_op_conv2d_large (counted)."""
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    ex = HipGraphExecutor(server["blob"], precision=precision)
    try:
        calls = []
        real = ex.eng.op_conv2d_large
        ex.eng.op_conv2d_large = lambda *a, **k: (calls.append((a[3], a[4])), real(*a, **k))[1]
        (got,) = ex.run(server["pix"].numpy())
        err = float(np.abs(got[:, 0] - server["want"]).max())
        if precision == "bf16x3":
            bound = 1e-3
        else:
            cpu = server["d16"]["bf16" if precision == "bf16" else "fp16"]
            bound = 4 * cpu
            print(f"layered torch module in {precision} on the CPU: max|d| = {cpu:.3e}")
        print(f"HgnetLkpanDetLike through HipGraphExecutor(precision={precision!r}): max|dprob| = {err:.3e} (bound {bound:.3e}); {len(calls)} large convolutions")
        want_large = sorted((l.attrs["kernel"][0], l.attrs["kernel"][1]) for l in ex.layers if l.op == "conv" and l.attrs["group"] == 1 and max(l.attrs["kernel"]) >= 5)
        assert sorted(calls) == want_large and {(9, 9), (7, 7), (5, 5), (7, 1), (1, 7), (5, 1), (1, 5)} == set(calls) and calls.count((9, 9)) == 8
        assert got.shape == (2, 1, 96, 128) and err <= bound
    finally:
        ex.eng.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_door(server, precision):
    """OcrDetectionTask(model="db_pp", task_path=..., server_model=True) in the three precisions: the map through the captured graph (three calls: eager,
    capture, replay) under the bounds of test_executor; precision="fp32": the boxes of the CPU oracle's post-processing on the fp32 module's map,
    corner for corner"""
    from pdf_table_amd import lib as L
    from pdf_table_amd.ocr_detection_task import OcrDetectionTask
    task = OcrDetectionTask(model="db_pp", task_path=str(server["dir"]), server_model=True, thresh=0.3, box_thresh=BOX_THRESH, precision=precision)
    try:
        assert task._engine.precision == {"fp32": L.PT_PRECISION_BF16X3, "bf16": L.PT_PRECISION_BF16, "fp16": L.PT_PRECISION_F16}[precision]
        bound = 1e-3 if precision == "fp32" else 4 * server["d16"][precision]
        pages = torch.from_numpy(np.stack(server["pages"])).cuda()
        for call in range(3):
            prob, _, _ = task._stage.forward(pages)
            got = prob.cpu().numpy()
            assert got.shape == server["want"].shape
            err = float(np.abs(got - server["want"]).max())
            print(f"HgnetLkpanDetLike through OcrDetectionTask(precision={precision!r}), call {call}: max|dprob| = {err:.3e} (bound {bound:.3e})")
            assert err <= bound
        out = task(server["pages"][0])
        assert len(out) == 1 and out[0].ndim == 2 and out[0].shape[1] == 8
        print(f"boxes [{precision}]: {len(out[0])} (the CPU oracle on the fp32 module's map: {BOXES_ORACLE})")
        if precision == "fp32":
            assert np.array_equal(_rows(out[0]), _rows(server["ref_boxes"]))
        else:
            assert len(out[0]) > 0
    finally:
        task._engine.close()


def test_pipeline_door(server, monkeypatch):
    """OcrTablePipeline(detect_model="db_pp", det_task_path=...) serves the graph: the detector of the pipeline is the generic executor on the stand-in
    and returns the door's boxes.  The pipeline's recogniser needs weights of its own and is not what this test is about: it is left out."""
    from pdf_table_amd import pipeline as P
    from pdf_table_amd.ocr_detection_task import OcrDetectionTask
    from pdf_table_amd.pipeline import OcrTablePipeline
    monkeypatch.setattr(P, "OcrRecognitionTask", lambda **k: None)
    pipe = OcrTablePipeline(detect_model="db_pp", det_task_path=str(server["dir"]), server_model=True, thresh=0.3, box_thresh=BOX_THRESH, precision="fp32")
    try:
        assert isinstance(pipe.text_detector, OcrDetectionTask)
        out = pipe.text_detector(server["pages"][0])
        assert np.array_equal(_rows(out[0]), _rows(server["ref_boxes"]))
    finally:
        pipe.engine.close()


def test_fuse_db_tail_runs_the_layered_route(server):
    """PFHeadLocal: the first transposed convolution's output feeds the local branch as well, and the second's Sigmoid is not the graph's output.  The
    pattern matcher of fuse_db_tail=True must not swallow that tail: the plan is empty and the map equals the layered route's bit for bit"""
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    a = HipGraphExecutor(server["blob"], precision="bf16")
    try:
        b = HipGraphExecutor(server["blob"], engine=a.eng, precision="bf16", fuse_db_tail=True)
        assert b._tail == {}
        (ya,), (yb,) = a.run(server["pix"].numpy()), b.run(server["pix"].numpy())
        assert np.array_equal(ya, yb)
    finally:
        a.eng.close()


class _ResLike(nn.Module):
    """relu(conv9x9(a) + a) behind a 3x3: the Add of an un-activated large convolution"""

    def __init__(self):
        super().__init__()
        self.c1, self.c9 = nn.Conv2d(3, 24, 3, 1, 1), nn.Conv2d(24, 24, 9, 1, 4)

    def forward(self, x):
        a = torch.relu(self.c1(x))
        return torch.relu(self.c9(a) + a)


def test_residual_add_of_a_large_convolution():
    """the route chosen for a residual Add behind a large convolution: convolution, pt_op_add, activation.  As a graph (tolerance mode, 1e-3 of the
    module) and through _conv(res=...) directly, which must equal the unfused sequence bit for bit -- it neither raises nor drops the operand"""
    from onnx_export import torch_export
    from pdf_table_amd.onnx_exec import HipGraphExecutor, _Act
    torch.manual_seed(3)
    mod = _ResLike().eval()
    x = torch.randn(2, 3, 12, 37)
    ex = HipGraphExecutor(torch_export(mod, x), precision="bf16x3")
    try:
        (got,) = ex.run(x.numpy())
        with torch.no_grad():
            want = mod(x).numpy()
        assert float(np.abs(got - want).max()) <= 1e-3 * max(1.0, float(np.abs(want).max()))
        k = next(i for i, l in enumerate(ex.layers) if l.op == "conv" and l.attrs["kernel"] == [9, 9])
        lay = ex.layers[k]
        g = torch.Generator().manual_seed(4)
        mk = lambda: _Act(torch.cat([torch.randn(2, 12, 37, 64, generator=g).bfloat16(), torch.zeros(2, 12, 37, 64).bfloat16()], -1).cuda(), 24)      # noqa: E731
        a, r = mk(), mk()
        a.t[..., 24:64] = 0
        fused = ex._conv(k, lay, a, res=r, res_act=1)
        plain = ex._conv(k, lay, a)
        seq = ex.eng.op_act(ex.eng.op_add(plain.t, r.t, split=True), 1, 0.0, 0.0, split=True)
        torch.cuda.synchronize()
        assert fused.c == 24 and torch.equal(fused.t.cpu().view(torch.int16), seq.cpu().view(torch.int16))
        assert not torch.equal(fused.t.cpu().view(torch.int16), plain.t.cpu().view(torch.int16))
    finally:
        ex.eng.close()


def test_a_lone_dense_5x5_on_a_feature_map_runs():
    """the counterpart of the refusals below: the same 5x5 / stride 1 on an 8-channel map goes to pt_op_conv2d_large (tolerance mode, 1e-3 of the module)"""
    from onnx_export import torch_export
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    torch.manual_seed(5)
    mod = nn.Conv2d(8, 8, 5, 1, 2).eval()
    x = torch.randn(2, 8, 16, 16)
    ex = HipGraphExecutor(torch_export(mod, x), precision="bf16x3")
    try:
        (got,) = ex.run(x.numpy())
        with torch.no_grad():
            want = mod(x).numpy()
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-3 * max(1.0, float(np.abs(want).max()))
    finally:
        ex.eng.close()


def test_still_refused():
    """a dense 5x5 of stride 2, an 11x11, an even side, a large kernel straight on the 3-channel image and a grouped 5x5 raise UnsupportedOnnxGraph
    naming the layer"""
    from onnx_export import torch_export
    from pdf_table_amd.onnx_exec import HipGraphExecutor
    from pdf_table_amd.onnx_import import UnsupportedOnnxGraph
    eng = None
    try:
        for mod, match in ((nn.Conv2d(3, 8, 5, 2, 2), r"Conv.*dense 5x5 convolution with strides \[2, 2\]"), (nn.Conv2d(3, 8, 11, 1, 5), r"Conv.*dense 11x11"),
                           (nn.Conv2d(3, 8, (5, 6), 1, (2, 3)), r"Conv.*(dense 5x6|padding)"), (nn.Conv2d(3, 8, 5, 1, 2), r"Conv.*dense 5x5 convolution on a 3-channel image"), (nn.Conv2d(8, 8, 5, 1, 2, groups=2), r"Conv.*grouped 5x5")):
            ex = HipGraphExecutor(torch_export(mod.eval(), torch.randn(1, mod.in_channels, 16, 16)), engine=eng)
            eng = ex.eng
            with pytest.raises(UnsupportedOnnxGraph, match=match):
                ex.run(np.zeros((1, mod.in_channels, 16, 16), np.float32))
    finally:
        if eng is not None:
            eng.close()
