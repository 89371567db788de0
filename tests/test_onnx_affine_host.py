"""The importer's constant-affine rules on the PP-OCRv4 mobile stand-ins (tools/onnx_export_ppdet.py), without a GPU: a Mul / Add / Sub / Div of a
feature map with a scalar or a per-channel constant becomes (s, b); behind a convolution it is folded into the weights (W' = s W, bias' = s bias + b,
float64, stored as fp32), everywhere else it is a layer of kind ``affine`` with the activation in front of it; chains collapse; c - x stays a ``sub``
layer for the executor to refuse.  Also: the ABI header declares the two new entry points, and the export tool runs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


@pytest.fixture(scope="module", params=["det", "rec"])
def stand_in(request):
    import onnx_export_ppdet as D
    from pdf_table_amd.onnx_import import load_onnx
    cls, shape = D.STAND_INS[request.param]
    net = D.seeded_ppdet(cls(), 3)
    blob = D.torch_export(net, torch.zeros(*shape), dynamic_batch=request.param == "rec")
    return request.param, D, net, load_onnx(blob).layers()


def test_first_lab_of_every_rep_layer_is_folded(stand_in):
    kind, D, net, layers = stand_in
    assert not [l.name for l in layers if l.op == "unsupported"]
    reps = [m for m in net.modules() if isinstance(m, D.Rep)]
    folded = [l for l in layers if l.attrs.get("affine_folded")]
    assert len(reps) == 28 and len(folded) == len(reps) and all(l.op == "conv" and l.attrs["affine_folded"] == 2 for l in folded)
    for rep, lay in zip(reps, folded):                       # modules() and the graph both follow the forward order
        s, b = rep.lab.scale.item(), rep.lab.bias.item()     # the fp32 parameters as float64
        assert (float(np.float32(s)), float(np.float32(b))) != (1.0, 0.0)
        w = rep.conv.weight.detach().double().numpy() * s
        bias = rep.conv.bias.detach().double().numpy() * s + b
        assert lay.weight.dtype == np.float32 and lay.bias.dtype == np.float32 and lay.weight.shape == w.shape
        assert lay.act == ("hardswish" if rep.act is not None else None)
        if lay.attrs.get("affine_folded_in"):                # a second affine folded into the INPUT side: test_remaining_affines_... has the numbers
            continue
        assert np.all(np.abs(lay.weight - w) <= 2.0 ** -23 * np.abs(w)) and np.all(np.abs(lay.bias - bias) <= 2.0 ** -23 * np.abs(bias) + 2.0 ** -149)


def test_remaining_affines_are_the_activation_labs(stand_in):
    """the LAB behind a hardswish: folded FORWARD into the 1x1 convolution that is its only reader (exact: nothing is padded), on the kernel in front
    of a padded depthwise convolution, an SE block or a second reader"""
    kind, D, net, layers = stand_in
    acts = [m for m in net.modules() if isinstance(m, D.Act)]
    aff = [l for l in layers if l.op == "affine"]
    labs = [l for l in aff if l.attrs["nodes"] == 2]
    fwd = [l for l in layers if l.attrs.get("affine_folded_in")]
    assert len(acts) == {"det": 24, "rec": 25}[kind] and len(fwd) == 10 and len(labs) + len(fwd) == len(acts)
    assert all(l.op == "conv" and l.attrs["kernel"] == [1, 1] and l.attrs["affine_folded_in"] == 2 for l in fwd)
    # the recogniser's two attention blocks multiply q by d ** -0.5: one node each, handed to the executor's view arithmetic
    rest = [l for l in aff if l.attrs["nodes"] != 2]
    assert len(rest) == {"det": 0, "rec": 2}[kind] and all(l.attrs["nodes"] == 1 and l.attrs["chain"][0][0] == "mul" for l in rest)
    known = {(a.lab.scale.item(), a.lab.bias.item()) for a in acts}
    for lay in labs:
        assert lay.attrs["act"] is None and lay.extra["s2"] is None
        assert lay.extra["s1"].dtype == np.float64 and lay.extra["s1"].shape == (1,)
        assert (float(lay.extra["s1"][0]), float(lay.extra["b1"][0])) in known
    # the first block: dw Rep (stride 1, no SE) -> its Act's LAB -> the pw Rep's 1x1 convolution, which also has its own LAB folded behind it
    if kind == "det":
        blk = net.stages[0][0]
    else:
        blk = net.blocks[0][0]
    s_in, b_in = blk.dw.act.lab.scale.item(), blk.dw.act.lab.bias.item()
    s_out, b_out = blk.pw.lab.scale.item(), blk.pw.lab.bias.item()
    w = blk.pw.conv.weight.detach().double().numpy()
    want_w = w * s_out * s_in
    want_b = (blk.pw.conv.bias.detach().double().numpy() + w[:, :, 0, 0].sum(1) * b_in) * s_out + b_out
    assert fwd[0].weight.shape == want_w.shape
    assert np.all(np.abs(fwd[0].weight - want_w) <= 2.0 ** -22 * np.abs(want_w)) and np.all(np.abs(fwd[0].bias - want_b) <= 2.0 ** -21 * (np.abs(want_b) + np.abs(w).sum((1, 2, 3)) * abs(b_in)))
    # nothing is left for the executor's "constant operand" refusals
    assert not [l.name for l in layers if l.op in ("add", "mul", "sub", "div") and l.extra and kind == "det"]


def test_rules_graph_layer_list():
    import onnx_export_ppdet as D
    from pdf_table_amd.onnx_import import load_onnx
    net = D.seeded_ppdet(D.AffineRulesLike(), 5)
    layers = load_onnx(D.torch_export(net, torch.zeros(1, 3, 16, 24))).layers()
    kinds = [(l.op, l.act, l.attrs.get("affine_folded"), l.attrs.get("act"), l.attrs.get("nodes")) for l in layers]
    assert kinds == [("conv", "hardswish", 2, None, None), ("affine", None, None, None, 2),           # conv -> LAB folds; hardswish -> LAB on the kernel
                     ("conv", None, None, None, None), ("add", None, None, None, None),
                     ("affine", None, None, "relu", 2),                                                # relu -> LAB: one launch
                     ("avgpool", None, None, None, None), ("affine", None, None, None, 5),             # the chain of five collapses
                     ("conv", None, None, None, None)], kinds
    chain = layers[6]
    a = net.a.detach().double().numpy().reshape(-1)
    s = a * 1.7 / 1.25
    b = ((0.3 * 1.7) - 0.2) / 1.25
    assert chain.extra["s1"].shape == (24,) and np.allclose(chain.extra["s1"], s, rtol=1e-6, atol=0) and np.allclose(chain.extra["b1"], b, rtol=1e-6, atol=0)
    x = torch.randn(2, 24, 3, 5, dtype=torch.float64)
    want = ((x * net.a.detach().double() + 0.3) * 1.7 - 0.2) / 1.25
    got = x * torch.from_numpy(chain.extra["s1"]).reshape(1, -1, 1, 1) + torch.from_numpy(np.broadcast_to(chain.extra["b1"], (24,)).copy()).reshape(1, -1, 1, 1)
    assert float((got - want).abs().max()) <= 1e-6
    # c - x is not an affine of this kind: it stays a `sub` layer with its constant, which the executor refuses by name
    rev = load_onnx(D.torch_export(D.seeded_ppdet(D.AffineRulesLike(reversed_sub=True), 5), torch.zeros(1, 3, 16, 24))).layers()
    subs = [l for l in rev if l.op == "sub"]
    assert len(subs) == 1 and subs[0].extra and subs[0].attrs["all_inputs"][0] not in subs[0].inputs


def test_header_declares_the_new_entry_points():
    with open(os.path.join(REPO, "include", "pdftable_hip.h")) as f:
        txt = f.read()
    for name in ("pt_op_affine_act", "pt_op_db_tail"):
        assert re.search(r"^int\s+" + name + r"\s*\(pt_engine\*", txt, flags=re.M), name
    from pdf_table_amd import lib as L
    import inspect
    src = inspect.getsource(L._proto)
    assert '"pt_op_affine_act"' in src and '"pt_op_db_tail"' in src          # bound by name: a library without them fails to load


def test_export_tool_runs(tmp_path):
    out = tmp_path / "det.onnx"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "onnx_export_ppdet.py"), "det", str(out)], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.stat().st_size > 1 << 20 and "affine x14" in r.stdout and "28 convolutions with a folded affine" in r.stdout, r.stdout
