"""Host side of the per-axis operators (ABI 18): the weight tiles of 1x3 / 3x1 kernels, the recogniser stand-ins of tools/onnx_export_pprec.py through
the exporter, the importer and the CPU interpreter, and the binding's version."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def _old_tile(w, fmt):
    """a literal copy of weights.tile_conv_weight as it stood before kernels with kh != kw were tiled"""
    from pdf_table_amd.weights import to_bf16_bits
    n, cin, kh, kw = w.shape
    t = w.reshape(n // 64, 64, cin // 32, 32, kh, kw).permute(0, 2, 4, 5, 1, 3).contiguous()
    return to_bf16_bits(t, fmt).reshape(n // 64, cin // 32, kh * kw, 64, 32)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("kh,kw", [(1, 3), (3, 1), (3, 3), (1, 1)])
def test_tiles_are_the_explicit_permutation(kh, kw, fmt):
    """[N, Cin, kh, kw] -> [N/64][Cin/32][kh kw taps, row-major][64][32], element by element; 1x1 and 3x3 bit-identical to the old formula"""
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
    if kh == kw:
        assert np.array_equal(t, _old_tile(w, fmt))
    if fmt == "bf16":
        hi, lo = split_bf16(w)
        t3 = tile_conv_weight_x3(w)
        assert t3.shape == (n // 64, 3 * cin // 32, kh * kw, 64, 32)
        th, tl = tile_conv_weight(hi), tile_conv_weight(lo)
        k = cin // 32
        assert np.array_equal(t3[:, :k], th) and np.array_equal(t3[:, k:2 * k], th) and np.array_equal(t3[:, 2 * k:], tl)      # w_hi x_hi | w_hi x_lo | w_lo x_hi


STAND_INS = [("ResVdRecLike", (2, 3, 32, 48), False), ("SvtrLcnetRecLike", (2, 3, 48, 64), True), ("MobileV3RecLike", (3, 3, 48, 64), True)]


@pytest.mark.parametrize("cls,shape,dyn", STAND_INS, ids=[s[0] for s in STAND_INS])
def test_stand_ins_export_with_their_geometry(cls, shape, dyn):
    """the exporter writes the per-axis attributes, OnnxGraph.layers() keeps them as lists, and oracle/onnx_ref reproduces the module within 1e-4
    (SvtrLcnetRecLike: that interpreter has no ReduceMean for the exporter's decomposed LayerNorm -- it must say so, nothing else)"""
    import onnx_export_pprec as P
    from onnx_export import torch_export
    from oracle import onnx_ref
    from pdf_table_amd.onnx_import import load_onnx
    from pdf_table_amd.onnx_proto import parse_model
    torch.manual_seed(0)
    m = P.seeded_pprec(getattr(P, cls)(), 5)
    x = torch.randn(*shape)
    blob = torch_export(m, x, dynamic_batch=dyn)
    layers = load_onnx(blob).layers()
    assert not [l.name for l in layers if l.op == "unsupported"]
    convs = [l for l in layers if l.op == "conv"]
    geo = {(tuple(l.attrs["kernel"]), tuple(l.attrs["strides"]), tuple(l.attrs["pads"])) for l in convs}
    pools = {(l.op, tuple(l.attrs["kernel"]), tuple(l.attrs["strides"]), int(l.attrs.get("ceil_mode") or 0)) for l in layers if l.op in ("maxpool", "avgpool")}
    assert all(isinstance(l.attrs["kernel"], list) and isinstance(l.attrs["strides"], list) for l in convs)
    if cls == "ResVdRecLike":
        assert {((3, 3), (2, 1), (1, 1, 1, 1)), ((3, 1), (1, 1), (1, 0, 1, 0)), ((1, 1), (2, 1), (0, 0, 0, 0))} <= geo
        assert ("avgpool", (2, 1), (2, 1), 1) in pools
    elif cls == "SvtrLcnetRecLike":
        assert {((3, 3), (2, 1), (1, 1, 1, 1)), ((3, 3), (1, 2), (1, 1, 1, 1)), ((5, 5), (2, 1), (2, 2, 2, 2)), ((1, 3), (1, 1), (0, 1, 0, 1))} <= geo
        assert ("avgpool", (3, 2), (3, 2), 0) in pools
    else:
        assert {((3, 3), (2, 1), (1, 1, 1, 1)), ((5, 5), (2, 1), (2, 2, 2, 2))} <= geo
        assert ("maxpool", (2, 2), (2, 2), 0) in pools and [l.op for l in layers].count("lstm") == 2
    with torch.no_grad():
        want = m(x).numpy()
    assert want.shape == {"ResVdRecLike": (2, 8, 8, 48), "SvtrLcnetRecLike": (2, 8, 97), "MobileV3RecLike": (3, 16, 97)}[cls]
    try:
        (ref,) = onnx_ref.run(parse_model(blob), {"x": x.numpy()})
    except NotImplementedError as e:
        assert cls == "SvtrLcnetRecLike" and "ReduceMean" in str(e)
    else:
        assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-4 * max(1.0, float(np.abs(want).max()))


def test_binding_has_the_rectangular_entries():
    from pdf_table_amd import lib as L
    from pdf_table_amd.build import build
    build(verbose=False)
    L.load()
    assert L.EXPECTED_ABI == 21          # the rectangular entries came with 18; 19 added pt_op_cvit_*, 20 pt_op_mtl_*, 21 the Lore processor's op entries
    assert {"pt_op_conv2d_rect", "pt_op_dwconv_rect", "pt_op_pool_rect"} <= set(L.EXPORTS)
