"""Host side of the SLANet ONNX door (no GPU): graph-valued attributes through pdf_table_amd/onnx_proto.py, and onnx_import.split_sla_head on the
stand-in of tools/onnx_export_slanet.py -- the head's parameters come back role by role, by data flow."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

from pdf_table_amd import onnx_proto as P  # noqa: E402
from pdf_table_amd.onnx_import import UnsupportedOnnxGraph, split_sla_head  # noqa: E402
from pdf_table_amd.weights import SLA_HEAD_ROLES  # noqa: E402


@pytest.fixture(scope="module")
def net():
    from onnx_export_slanet import SlaNetLike, seeded_slanet
    return seeded_slanet(SlaNetLike(n_cls=30, n_loc=4, steps=24), 3)


@pytest.fixture(scope="module")
def exported(net):
    from onnx_export_slanet import export_slanet
    return export_slanet(net, 64, batch=2)


def test_graph_attribute_round_trip():
    body = P.OnnxModel(nodes=[P.OnnxNode("Add", ["a", "w"], ["b"], {"k": 3}, "inner")], initializers={"w": np.arange(4, dtype=np.float32).reshape(2, 2)},
                       inputs=[P.OnnxValueInfo("a", 1, ("n", 2))], outputs=[P.OnnxValueInfo("b", 1, ("n", 2))], graph_name="body")
    outer_body = P.OnnxModel(nodes=[P.OnnxNode("If", ["c"], ["y"], {"then_branch": body, "else_branch": body}, "nested")], graph_name="outer_body",
                             inputs=[P.OnnxValueInfo("c", 9, ())], outputs=[P.OnnxValueInfo("y", 1, ("n", 2))])
    m = P.OnnxModel(nodes=[P.OnnxNode("Loop", ["trip", "cond", "x"], ["y"], {"body": outer_body, "note": "s"}, "loop")], opset=13,
                    initializers={"trip": np.array(5, np.int64)}, inputs=[P.OnnxValueInfo("x", 1, (1, 2))], outputs=[P.OnnxValueInfo("y", 1, (1, 2))])
    data = P.serialize_model(m)
    back = P.parse_model(data)
    assert P.serialize_model(back) == data                                   # byte-stable
    ob = back.nodes[0].attrs["body"]
    assert isinstance(ob, P.OnnxModel) and ob.graph_name == "outer_body" and back.nodes[0].attrs["note"] == "s"
    inner = ob.nodes[0].attrs["then_branch"]
    assert isinstance(inner, P.OnnxModel) and inner.nodes[0].op_type == "Add" and inner.nodes[0].attrs == {"k": 3}
    assert np.array_equal(inner.initializers["w"], body.initializers["w"]) and [i.name for i in inner.inputs] == ["a"]
    assert inner.opset == ob.opset == 13                                     # nested graphs share the model's opset


def test_plain_graphs_serialize_as_before():
    """a graph without graph attributes goes through the writer byte for byte as it did: the TorchScript export of a small module round-trips"""
    from onnx_export import torch_export
    data = torch_export(torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, 1, 1), torch.nn.ReLU()), torch.zeros(1, 3, 8, 8))
    m = P.parse_model(data)
    once = P.serialize_model(m)
    assert P.serialize_model(P.parse_model(once)) == once


def test_split_returns_the_modules_weights_role_by_role(net, exported):
    prefix, hp = split_sla_head(P.parse_model(exported))
    want = net.head_params()
    assert set(hp.weights) == set(SLA_HEAD_ROLES)
    for k in SLA_HEAD_ROLES:
        assert hp.weights[k].dtype == np.float32 and np.array_equal(hp.weights[k], want[k]), k
    assert (hp.hidden, hp.channels, hp.n_cls, hp.n_loc, hp.steps) == (256, 96, 30, 4, 24)
    assert hp.outputs == ("loc_preds", "structure_probs")
    assert [o.name for o in prefix.outputs] == [hp.feature] and not any(n.op_type == "Loop" for n in prefix.nodes)
    # the prefix is the feed-forward part alone and computes the module's feature map
    from oracle.onnx_ref import run
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        ref = net.features(x).numpy()
    got = run(prefix, {prefix.inputs[0].name: x.numpy()})[0]
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_gemm_and_matmul_operands_alike(net):
    from onnx_export_slanet import export_slanet
    a = split_sla_head(P.parse_model(export_slanet(net, 64, gemm_gru=True)))[1]
    b = split_sla_head(P.parse_model(export_slanet(net, 64, gemm_gru=False)))[1]
    for k in SLA_HEAD_ROLES:
        assert np.array_equal(a.weights[k], b.weights[k]), k


def _loop(model):
    return [n for n in model.nodes if n.op_type == "Loop"][0]


def test_swapped_square_matrices_resolve_by_data_flow(net, exported):
    """the three [H, H] MatMul operands trade NAMES and POSITIONS in the initializer list (each node keeps reading its own values): a matcher that
    went by name or by order would hand them to the wrong roles"""
    m = P.parse_model(exported)
    body = _loop(m).attrs["body"]
    sq = [k for k, v in body.initializers.items() if v.shape == (256, 256)]
    assert len(sq) == 3
    ren = {sq[0]: sq[1], sq[1]: sq[2], sq[2]: sq[0]}
    items = [(ren.get(k, k), v) for k, v in body.initializers.items()]
    body.initializers = dict(reversed(items))
    for n in body.nodes:
        n.inputs = [ren.get(i, i) for i in n.inputs]
    hp = split_sla_head(P.parse_model(P.serialize_model(m)))[1]
    want = net.head_params()
    for k in ("h2h_w", "s1_w", "l1_w", "w_hh", "i2h_w"):
        assert np.array_equal(hp.weights[k], want[k]), k


def test_feedback_removed_is_refused_by_name(exported):
    m = P.parse_model(exported)
    body = _loop(m).attrs["body"]
    k = [i for i, n in enumerate(body.nodes) if n.op_type == "ArgMax"][0]
    body.nodes[k] = P.OnnxNode("Identity", ["prev_in"], list(body.nodes[k].outputs), {}, "no_feedback")
    with pytest.raises(UnsupportedOnnxGraph) as e:
        split_sla_head(m)
    assert "ArgMax" in str(e.value) and "prev_in" in str(e.value)


def test_second_softmax_in_the_body_is_refused(exported):
    m = P.parse_model(exported)
    body = _loop(m).attrs["body"]
    k = [i for i, n in enumerate(body.nodes) if n.op_type == "Sigmoid" and n.outputs == ["loc_step"]][0]
    body.nodes[k] = P.OnnxNode("Softmax", list(body.nodes[k].inputs), ["loc_step"], {"axis": 1}, "not_a_sigmoid")
    with pytest.raises(UnsupportedOnnxGraph) as e:
        split_sla_head(m)
    assert "not_a_sigmoid" in str(e.value)


def test_no_loop_is_refused():
    from onnx_export import torch_export
    data = torch_export(torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, 1, 1), torch.nn.ReLU()), torch.zeros(1, 3, 8, 8))
    with pytest.raises(UnsupportedOnnxGraph):
        split_sla_head(P.parse_model(data))
