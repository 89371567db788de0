"""Host side of the large dense kernels (csrc/large_conv.hip): the weight tiles of 9x9 and 7x1 kernels, the server-detector stand-in of
tools/onnx_export_ppdet_server.py through the exporter, the importer and the CPU interpreter, and the binding."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("kh,kw", [(9, 9), (7, 1)])
def test_tiles_are_the_explicit_permutation(kh, kw, fmt):
    """[N, Cin, kh, kw] -> [N/64][Cin/32][kh kw taps, row-major][64][32], element by element (the loop of tests/test_onnx_rect_host.py for the new sizes)"""
    from pdf_table_amd.weights import split_bf16, tile_conv_weight, tile_conv_weight_x3, to_bf16_bits
    n, cin = 128, 96
    w = torch.randn(n, cin, kh, kw, generator=torch.Generator().manual_seed(kh * 10 + kw))
    t = tile_conv_weight(w, fmt)
    assert t.shape == (n // 64, cin // 32, kh * kw, 64, 32) and t.dtype == np.uint16
    bits = to_bf16_bits(w, fmt)
    want = np.zeros_like(t)
    for nt in range(n // 64):
        for kc in range(cin // 32):
            for dy in range(kh):
                for dx in range(kw):
                    want[nt, kc, dy * kw + dx] = bits[nt * 64:(nt + 1) * 64, kc * 32:(kc + 1) * 32, dy, dx]
    assert np.array_equal(t, want)
    if fmt == "bf16":
        hi, lo = split_bf16(w)
        t3 = tile_conv_weight_x3(w)
        assert t3.shape == (n // 64, 3 * cin // 32, kh * kw, 64, 32)
        th, tl = tile_conv_weight(hi), tile_conv_weight(lo)
        k = cin // 32
        assert np.array_equal(t3[:, :k], th) and np.array_equal(t3[:, k:2 * k], th) and np.array_equal(t3[:, 2 * k:], tl)      # w_hi x_hi | w_hi x_lo | w_lo x_hi


def test_stand_in_exports_with_its_geometry():
    """the exporter writes the kernel sizes, OnnxGraph.layers() keeps them as lists and leaves no operator unsupported, and oracle/onnx_ref reproduces
    the fp32 module within 1e-4 (or names the one operator it lacks, nothing else)"""
    import onnx_export_ppdet_server as S
    from oracle import onnx_ref
    from pdf_table_amd.onnx_import import load_onnx
    from pdf_table_amd.onnx_proto import parse_model
    m = S.seeded_ppdet_server(S.HgnetLkpanDetLike(), 1)
    x = torch.randn(2, 3, 96, 128, generator=torch.Generator().manual_seed(0))
    blob = S.torch_export(m, x)
    layers = load_onnx(blob).layers()
    assert not [l.name for l in layers if l.op == "unsupported"]
    convs = [l for l in layers if l.op == "conv"]
    assert all(isinstance(l.attrs["kernel"], list) and isinstance(l.attrs["strides"], list) for l in convs)
    dense = [(tuple(l.attrs["kernel"]), tuple(l.attrs["strides"]), tuple(l.attrs["pads"])) for l in convs if l.attrs["group"] == 1]
    for k in ((9, 9), (7, 7), (5, 5), (7, 1), (1, 7), (5, 1), (1, 5), (3, 1), (1, 3)):
        assert (k, (1, 1), (k[0] // 2, k[1] // 2, k[0] // 2, k[1] // 2)) in dense, k
    assert dense.count(((9, 9), (1, 1), (4, 4, 4, 4))) == 8 and ((3, 3), (2, 2), (1, 1, 1, 1)) in dense
    assert {l.attrs["group"] for l in convs if l.attrs["group"] != 1} == {48, 96, 160}          # the depthwise down-samplers of stages 2 .. 4
    ops = [l.op for l in layers]
    assert ops.count("convT") == 2 and ops.count("gap") == 5 and ops.count("concat") == 7 and ops.count("maxpool") == 1
    assert max(len(l.inputs) for l in layers if l.op == "concat") == 7          # an HG block's Concat: the input and its six layers
    with torch.no_grad():
        want = m(x).numpy()
    assert want.shape == (2, 1, 96, 128)
    try:
        (ref,) = onnx_ref.run(parse_model(blob), {"x": x.numpy()})
    except NotImplementedError as e:
        pytest.fail(f"oracle/onnx_ref lacks an operator of the stand-in: {e}")
    assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-4


def test_binding_has_the_large_convolution():
    """an entry point added under ABI 19 without a bump (a stale library fails to bind by name); 20 added pt_op_mtl_*"""
    from pdf_table_amd import lib as L
    from pdf_table_amd.build import build
    build(verbose=False)
    L.load()
    assert L.EXPECTED_ABI == 21 and "pt_op_conv2d_large" in L.EXPORTS
    from pdf_table_amd.engine import HipEngine
    assert callable(getattr(HipEngine, "op_conv2d_large"))
