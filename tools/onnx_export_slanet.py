"""Stand-in with the GEOMETRY of PaddleOCR's SLANet table-structure model (``{ch,en}_ppstructure_mobile_v2.0_SLANet_infer``) for the ONNX door of
``OcrTableStructureTask(model="SLANet")`` -- test / tooling code, not product.  The real files are not available offline: what is served here is their
layer geometry, written from PaddleOCR's published model definitions (ppocr/modeling/backbones/det_pp_lcnet.py, necks/csp_pan.py,
heads/table_att_head.py::SLAHead) and from memory -- still a stand-in, with seeded weights, not the shipped graphs.

  * ``SlaNetLike``  an LCNet-type backbone (the blocks of tools/onnx_export_ppdet.py) tapped at strides 8 / 16 / 32, a light CSP-PAN-type neck (1x1
                    laterals and the bottom-up pass: stride-2 depthwise 5x5, concat, 1x1 -> depthwise 5x5 -> 1x1; no up-sampling, so any input side
                    works -- 488 is not a multiple of 32; widths off the tile sizes) whose last level is 96 channels at 1/32, and SLAHead: an attention-GRU cell (``nn.Linear`` / ``nn.GRUCell`` parameters, hidden 256) walked ``steps``
                    times with the arg-max of step t fed back as the one-hot input of step t + 1.  [B, 3, S, S] -> (loc_preds [B, T, L],
                    structure_probs [B, T, V]), the order ``extract_predict_result`` reads.
  * ``export_slanet(net, size)``  the feed-forward part through the TorchScript exporter (tools/onnx_export.py::torch_export), the head appended as ONE
                    ONNX ``Loop`` node with the project's own writer (pdf_table_amd/onnx_proto.py).  Loop body, Paddle2ONNX style: Linear layers are
                    ``MatMul`` with an [in, out] operand + ``Add``; the GRU cell's two projections are ``Gemm`` (transB = 1, [out, in]); scan outputs
                    are the step's logits and boxes, transposed to batch-major behind the loop, the class soft-max behind that (SLAHead applies it
                    after the walk in eval mode).

    python tools/onnx_export_slanet.py [out.onnx]      # exports the stand-in and prints what split_sla_head makes of it
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onnx_export import torch_export  # noqa: E402
from onnx_export_ppdet import Block, Rep, seeded_ppdet  # noqa: E402
from pdf_table_amd.onnx_proto import OnnxModel, OnnxNode, OnnxValueInfo, parse_model, serialize_model  # noqa: E402


class _CspLevel(nn.Module):
    """concat -> 1x1 -> depthwise 5x5 -> 1x1 (a CSP layer reduced to its main branch)"""

    def __init__(self, cin, cout):
        super().__init__()
        self.a, self.dw, self.b = Rep(cin, cout, 1, 1, 1), Rep(cout, cout, 5, 1, cout), Rep(cout, cout, 1, 1, 1)

    def forward(self, x):
        return self.b(self.dw(self.a(x)))


class SlaNetLike(nn.Module):
    def __init__(self, n_cls: int = 30, n_loc: int = 4, steps: int = 501, hidden: int = 256, neck: int = 96):
        super().__init__()
        self.n_cls, self.n_loc, self.steps, self.hidden, self.neck_c = n_cls, n_loc, steps, hidden, neck
        self.stem = nn.Sequential(nn.Conv2d(3, 16, 3, 2, 1, bias=False), nn.BatchNorm2d(16))
        self.s4 = nn.Sequential(Block(16, 24, 3, 2, False))
        self.s8 = nn.Sequential(Block(24, 40, 3, 2, False), Block(40, 40, 3, 1, False))
        self.s16 = nn.Sequential(Block(40, 72, 3, 2, False), Block(72, 72, 5, 1, False))
        self.s32 = nn.Sequential(Block(72, 136, 5, 2, True), Block(136, 136, 5, 1, True))
        self.lat = nn.ModuleList([nn.Conv2d(c, neck, 1) for c in (40, 72, 136)])
        self.down8, self.down16 = Rep(neck, neck, 5, 2, neck), Rep(neck, neck, 5, 2, neck)
        self.bu16, self.bu32 = _CspLevel(2 * neck, neck), _CspLevel(2 * neck, neck)
        # SLAHead
        self.i2h = nn.Linear(neck, hidden, bias=False)
        self.h2h = nn.Linear(hidden, hidden)
        self.score = nn.Linear(hidden, 1, bias=False)
        self.rnn = nn.GRUCell(neck + n_cls, hidden)
        self.structure_generator = nn.Sequential(nn.Linear(hidden, hidden), nn.Linear(hidden, n_cls))
        self.loc_generator = nn.Sequential(nn.Linear(hidden, hidden), nn.Linear(hidden, n_loc))

    def features(self, x):
        """-> the neck's last level [B, 96, S / 32, S / 32]"""
        c8 = self.s8(self.s4(self.stem(x)))
        c16 = self.s16(c8)
        c32 = self.s32(c16)
        l8, l16, l32 = (m(t) for m, t in zip(self.lat, (c8, c16, c32)))
        b16 = self.bu16(torch.cat([self.down8(l8), l16], 1))
        return self.bu32(torch.cat([self.down16(b16), l32], 1))

    def head_params(self):
        """the head's parameters by role (pdf_table_amd.weights.SLA_HEAD_ROLES), float32 numpy, every matrix [out, in]"""
        g = lambda t: t.detach().float().numpy().copy()      # noqa: E731
        sg, lg = self.structure_generator, self.loc_generator
        return {"i2h_w": g(self.i2h.weight), "h2h_w": g(self.h2h.weight), "h2h_b": g(self.h2h.bias), "score_w": g(self.score.weight).reshape(-1),
                "w_ih": g(self.rnn.weight_ih), "b_ih": g(self.rnn.bias_ih), "w_hh": g(self.rnn.weight_hh), "b_hh": g(self.rnn.bias_hh),
                "s1_w": g(sg[0].weight), "s1_b": g(sg[0].bias), "s2_w": g(sg[1].weight), "s2_b": g(sg[1].bias),
                "l1_w": g(lg[0].weight), "l1_b": g(lg[0].bias), "l2_w": g(lg[1].weight), "l2_b": g(lg[1].bias)}

    def walk(self, fea_map, steps=None):
        """SLAHead.forward in eval mode on the feature map: -> (loc_preds [B, T, L], structure_probs [B, T, V], logits [B, T, V])"""
        B, C = fea_map.shape[:2]
        H = self.hidden
        fea = fea_map.reshape(B, C, -1).transpose(1, 2)
        P = self.i2h(fea)
        h = torch.zeros(B, H, dtype=fea.dtype)
        prev = torch.zeros(B, dtype=torch.long)
        locs, logits = [], []
        for _ in range(self.steps if steps is None else steps):
            e = self.score(torch.tanh(P + self.h2h(h)[:, None, :]))
            alpha = torch.softmax(e, dim=1)
            ctx = (alpha.transpose(1, 2) @ fea)[:, 0]
            x = torch.cat([ctx, F.one_hot(prev, self.n_cls).to(fea.dtype)], 1)
            gi, gh = F.linear(x, self.rnn.weight_ih, self.rnn.bias_ih), F.linear(h, self.rnn.weight_hh, self.rnn.bias_hh)
            r = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            c = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (h - c) * z + c
            s = self.structure_generator(h)
            locs.append(torch.sigmoid(self.loc_generator(h)))
            logits.append(s)
            prev = s.argmax(1)
        logits = torch.stack(logits, 1)
        return torch.stack(locs, 1), torch.softmax(logits, -1), logits

    def forward(self, x):
        return self.walk(self.features(x))[:2]


class _Features(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        return self.net.features(x)


def seeded_slanet(net: SlaNetLike, seed: int, example_size: int = 96, cell_ids=None, cell_bias: float = 4.0) -> SlaNetLike:
    """Seeded weights (tools/onnx_export_ppdet.py::seeded_ppdet for the convolutions, each scaled to unit output variance on a seeded batch), and a head
    whose walks END: hidden unit 0 is a leaky counter -- its GRU rows ignore the hidden state, its candidate is pinned near +1 and its update gate near
    0.9, moved a little by the context, so it climbs as 1 - 0.9^t at a table-dependent rate -- and the ``eos`` logit (the last class) reads it through
    unit 0 of the structure generator with a large gain and a seed-dependent threshold, so ``eos`` takes over after a seed-dependent number of cells
    and by a wide margin.  Elsewhere the head's matrices are uniform at a scale that keeps the top two logits well apart; the classes ``cell_ids``
    (default: the last class before ``eos``, where TableLabelDecode puts ``<td></td>`` for a dictionary without it) get ``cell_bias`` on their logits, so
    that walks hold cells and the door's boxes are exercised."""
    seeded_ppdet(nn.ModuleList([net.stem, net.s4, net.s8, net.s16, net.s32, net.lat, net.down8, net.down16, net.bu16, net.bu32]), seed)
    g = torch.Generator().manual_seed(seed + 77)
    ex = torch.randn(2, 3, example_size, example_size, generator=g)
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]

    def hook(m, _inp, out):
        f = 1.0 / max(float(out.std()), 1e-6)
        with torch.no_grad():
            m.weight.mul_(f)
            if m.bias is not None:
                m.bias.mul_(f)
        return out * f
    handles = [m.register_forward_hook(hook) for m in convs]
    with torch.no_grad():
        net.features(ex)
    for h in handles:
        h.remove()
    H, C, V = net.hidden, net.neck_c, net.n_cls

    def u(t, fan_in, k):
        t.copy_((torch.rand(t.shape, generator=g) * 2 - 1) * (k / fan_in ** 0.5))
    with torch.no_grad():
        u(net.i2h.weight, C, 2.0); u(net.h2h.weight, H, 2.0); u(net.h2h.bias, H, 1.0); u(net.score.weight, H, 8.0)
        u(net.rnn.weight_ih, C, 2.0); u(net.rnn.bias_ih, H, 1.0); u(net.rnn.weight_hh, H, 2.0); u(net.rnn.bias_hh, H, 1.0)
        sg, lg = net.structure_generator, net.loc_generator
        u(sg[0].weight, H, 2.0); u(sg[0].bias, H, 1.0); u(sg[1].weight, H, 12.0); u(sg[1].bias, 1, 0.5)
        u(lg[0].weight, H, 2.0); u(lg[0].bias, H, 1.0); u(lg[1].weight, H, 6.0); u(lg[1].bias, 1, 0.5)
        # the counter: unit 0 of the GRU (rows 0, H, 2H of the gate matrices)
        for row in (0, H, 2 * H):
            net.rnn.weight_ih[row].zero_(); net.rnn.weight_hh[row].zero_(); net.rnn.bias_ih[row] = 0.0; net.rnn.bias_hh[row] = 0.0
        net.rnn.bias_ih[H] = 2.2                                                   # z = sigmoid(2.2 + ...) ~ 0.9
        net.rnn.weight_ih[H, :C] = (torch.rand(C, generator=g) * 2 - 1) * 0.15     # ... moved by the context: the rate depends on the table
        net.rnn.bias_ih[2 * H] = 5.0                                               # c = tanh(5) ~ 1
        # eos reads it: s1[0] = h[0]; logit(eos) = gain (h[0] - theta); no other class reads s1[0]
        sg[0].weight[0].zero_(); sg[0].weight[0, 0] = 1.0; sg[0].bias[0] = 0.0
        sg[1].weight[:, 0] = 0.0
        sg[1].weight[V - 1].zero_()
        theta = 0.55 + 0.3 * float(torch.rand(1, generator=g))                     # 1 - 0.9^t crosses 0.55 .. 0.85 between t = 8 and t = 18
        sg[1].weight[V - 1, 0] = 120.0
        sg[1].bias[V - 1] = -120.0 * theta
        for k in ((V - 2,) if cell_ids is None else cell_ids):
            sg[1].bias[k] += cell_bias
        sg[1].weight[0] = sg[1].weight[0] * 0.0                                    # sos is never predicted by a trained head: keep it far below
        sg[1].bias[0] = -30.0
    return net.eval()


def loop_body(p, hidden: int, n_cls: int, fea_name: str, gemm_gru: bool = True) -> OnnxModel:
    """the Loop body of SLAHead over the outer-scope token rows ``fea_name`` [B, N, C]; p: the parameters by role ([out, in]).  gemm_gru False: the
    GRU projections as MatMul ([in, out]) + Add as well"""
    init = {}
    nodes = []

    def N(op, ins, outs, **attrs):
        nodes.append(OnnxNode(op, list(ins), list(outs), dict(attrs), name=f"sla_{len(nodes)}_{op}"))
        return outs[0]

    def linear(x, w, b, name, gemm=False):
        if gemm:
            init[name + ".w"] = np.ascontiguousarray(w, np.float32)
            init[name + ".b"] = np.asarray(b, np.float32)
            return N("Gemm", [x, name + ".w", name + ".b"], [name + ".y"], alpha=1.0, beta=1.0, transB=1)
        init[name + ".w"] = np.ascontiguousarray(np.asarray(w, np.float32).T)
        y = N("MatMul", [x, name + ".w"], [name + ".mm"])
        if b is None:
            return y
        init[name + ".b"] = np.asarray(b, np.float32)
        return N("Add", [y, name + ".b"], [name + ".y"])
    init["axes1"] = np.array([1], np.int64)
    init["onehot_depth"] = np.array(n_cls, np.int64)
    init["onehot_values"] = np.array([0.0, 1.0], np.float32)
    P = linear(fea_name, p["i2h_w"], None, "i2h")
    q = N("Unsqueeze", [linear("h_in", p["h2h_w"], p["h2h_b"], "h2h"), "axes1"], ["q3"])
    e = linear(N("Tanh", [N("Add", [P, q], ["pq"])], ["res"]), np.asarray(p["score_w"]).reshape(1, -1), None, "score")
    alpha = N("Transpose", [N("Softmax", [e], ["alpha"], axis=1)], ["alpha_t"], perm=[0, 2, 1])
    ctx = N("Squeeze", [N("MatMul", [alpha, fea_name], ["ctx3"]), "axes1"], ["ctx"])
    hot = N("OneHot", ["prev_in", "onehot_depth", "onehot_values"], ["hot"], axis=-1)
    x = N("Concat", [ctx, hot], ["x"], axis=1)
    gi = linear(x, p["w_ih"], p["b_ih"], "gru_ih", gemm=gemm_gru)
    gh = linear("h_in", p["w_hh"], p["b_hh"], "gru_hh", gemm=gemm_gru)
    N("Split", [gi], ["i_r", "i_z", "i_c"], axis=1)
    N("Split", [gh], ["h_r", "h_z", "h_c"], axis=1)
    r = N("Sigmoid", [N("Add", ["i_r", "h_r"], ["r_pre"])], ["r"])
    z = N("Sigmoid", [N("Add", ["i_z", "h_z"], ["z_pre"])], ["z"])
    c = N("Tanh", [N("Add", ["i_c", N("Mul", [r, "h_c"], ["rh"])], ["c_pre"])], ["c"])
    h = N("Add", [N("Mul", [N("Sub", ["h_in", c], ["hc"]), z], ["hcz"]), c], ["h_out"])
    s = linear(linear(h, p["s1_w"], p["s1_b"], "sg0"), p["s2_w"], p["s2_b"], "sg1")
    loc = N("Sigmoid", [linear(linear(h, p["l1_w"], p["l1_b"], "lg0"), p["l2_w"], p["l2_b"], "lg1")], ["loc_step"])
    N("ArgMax", [s], ["prev_out"], axis=1, keepdims=0)
    N("Identity", ["cond_in"], ["cond_out"])
    B = "batch"
    return OnnxModel(nodes=nodes, initializers=init, graph_name="sla_head_body",
                     inputs=[OnnxValueInfo("iter", 7, ()), OnnxValueInfo("cond_in", 9, ()), OnnxValueInfo("h_in", 1, (B, hidden)), OnnxValueInfo("prev_in", 7, (B,))],
                     outputs=[OnnxValueInfo("cond_out", 9, ()), OnnxValueInfo("h_out", 1, (B, hidden)), OnnxValueInfo("prev_out", 7, (B,)),
                              OnnxValueInfo(s, 1, (B, n_cls)), OnnxValueInfo(loc, 1, (B, len(p["l2_b"])))])


def append_head(model: OnnxModel, p, hidden: int, n_cls: int, steps: int, batch: int, gemm_gru: bool = True) -> OnnxModel:
    """model: a feed-forward graph ending in the [B, C, h, w] map -> the same graph with SLAHead behind it; outputs loc_preds, structure_probs"""
    fmap = model.outputs[0].name
    c = int(np.asarray(p["i2h_w"]).shape[1])
    n_loc = len(p["l2_b"])
    model.initializers.update({"sla.flat_shape": np.array([0, c, -1], np.int64), "sla.trip": np.array(steps, np.int64), "sla.cond": np.array(True),
                               "sla.h0": np.zeros((batch, hidden), np.float32), "sla.prev0": np.zeros((batch,), np.int64)})
    model.nodes.append(OnnxNode("Reshape", [fmap, "sla.flat_shape"], ["sla.flat"], {}, "sla_flatten"))
    model.nodes.append(OnnxNode("Transpose", ["sla.flat"], ["sla.fea"], {"perm": [0, 2, 1]}, "sla_tokens"))
    body = loop_body(p, hidden, n_cls, "sla.fea", gemm_gru)
    model.nodes.append(OnnxNode("Loop", ["sla.trip", "sla.cond", "sla.h0", "sla.prev0"], ["sla.h_last", "sla.prev_last", "sla.logits_tm", "sla.loc_tm"],
                                {"body": body}, "sla_loop"))
    model.nodes.append(OnnxNode("Transpose", ["sla.logits_tm"], ["sla.logits"], {"perm": [1, 0, 2]}, "sla_logits_bm"))
    model.nodes.append(OnnxNode("Softmax", ["sla.logits"], ["structure_probs"], {"axis": 2}, "sla_probs"))
    model.nodes.append(OnnxNode("Transpose", ["sla.loc_tm"], ["loc_preds"], {"perm": [1, 0, 2]}, "sla_loc_bm"))
    model.outputs = [OnnxValueInfo("loc_preds", 1, (batch, steps, n_loc)), OnnxValueInfo("structure_probs", 1, (batch, steps, n_cls))]
    return model


def export_slanet(net: SlaNetLike, size: int, batch: int = 1, gemm_gru: bool = True) -> bytes:
    """size: the side of the square network input (488 in the product; any multiple of 32)"""
    data = torch_export(_Features(net), torch.zeros(batch, 3, size, size), output_name="fea_map")
    model = append_head(parse_model(data), net.head_params(), net.hidden, net.n_cls, net.steps, batch, gemm_gru)
    return serialize_model(model)


if __name__ == "__main__":
    from pdf_table_amd.onnx_import import split_sla_head
    net = seeded_slanet(SlaNetLike(), 1)
    data = export_slanet(net, 488)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "wb") as f:
            f.write(data)
    prefix, hp = split_sla_head(parse_model(data))
    print(f"SlaNetLike: {len(data)} bytes; prefix of {len(prefix.nodes)} nodes ending in {prefix.outputs[0].name}; head H={hp.hidden} C={hp.channels} "
          f"V={hp.n_cls} L={hp.n_loc} T={hp.steps}")
