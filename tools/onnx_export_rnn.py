"""Recurrent stand-ins for the generic ONNX executor's LSTM layer (pdf_table_amd/onnx_exec.py, csrc/lstm_op.hip) -- test / tooling code, not product.

  * ``MobileCrnn``: a CRNN-type recogniser of the PP-OCR mobile family's shape (``en_ppocr_mobile_v2.0_table_rec`` = "PP-Table": a light conv
    backbone down to height 1, two BiLSTMs of 48 units, a linear CTC head with its Softmax).  The real files are not available offline; the
    graph comes from PyTorch's own exporter (tools/onnx_export.py::torch_export), which writes nn.LSTM as an ONNX LSTM node (gates i, o, f, c)
    followed by Transpose(0, 2, 1, 3) + Reshape, and -- with a dynamic batch -- zero initial states as a Shape -> ... -> Expand chain.
  * ``LstmOnly``: nothing but the recurrent layers on an input that is already a height-1 map [B, I, 1, T]: the operator-level graphs.
  * ``write_lstm_node``: a hand-built one-node graph through pdf_table_amd.onnx_proto.serialize_model, for what nn.LSTM cannot express
    (direction="reverse" on a one-direction node) or never emits (sequence_lens, a non-zero initial_h).

``onnx_lstm_params(nn.LSTM)`` gives the ONNX operands (W, R, B in gate order i, o, f, c) of a torch layer for the references.
"""
from __future__ import annotations

import os
import sys
from typing import Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pdf_table_amd.onnx_proto import OnnxModel, OnnxNode, OnnxValueInfo, serialize_model  # noqa: E402


class MobileCrnn(torch.nn.Module):
    """[B, 3, 48, W] -> four stride-2 convs (48 -> 3 rows) -> two MaxPool(3, 2, 1) (-> 1 row, ceil(W / 64) columns) -> squeeze / permute to
    [T, B, 40] -> BiLSTM(48) -> BiLSTM(48) -> Linear -> [B, T, classes] -> Softmax"""

    def __init__(self, classes: int = 97, hidden: int = 48, feat: int = 40):
        super().__init__()
        nn = torch.nn
        cbr = lambda i, o, act: nn.Sequential(nn.Conv2d(i, o, 3, 2, 1, bias=False), nn.BatchNorm2d(o), act)
        self.s1, self.s2 = cbr(3, 32, nn.Hardswish()), cbr(32, 64, nn.ReLU())
        self.s3, self.s4 = cbr(64, 96, nn.ReLU()), cbr(96, feat, nn.ReLU())
        self.pool = nn.MaxPool2d(3, 2, 1)
        self.rnn1 = nn.LSTM(feat, hidden, bidirectional=True)
        self.rnn2 = nn.LSTM(2 * hidden, hidden, bidirectional=True)
        self.head = nn.Linear(2 * hidden, classes)

    def logits(self, x):
        x = self.pool(self.pool(self.s4(self.s3(self.s2(self.s1(x))))))
        x = x.squeeze(2).permute(2, 0, 1)                       # [T, B, C]
        x, _ = self.rnn1(x)
        x, _ = self.rnn2(x)
        return self.head(x).permute(1, 0, 2)                    # [B, T, classes]

    def forward(self, x):
        return torch.softmax(self.logits(x), dim=-1)


class LstmOnly(torch.nn.Module):
    """[B, I, 1, T] -> [T, B, I] -> `layers` stacked nn.LSTM(hidden) (-> Linear(out) when out > 0) -> the time-major tensor [T, B, C] as it is"""

    def __init__(self, inp: int, hidden: int, bidirectional: bool = True, layers: int = 1, out: int = 0):
        super().__init__()
        d = 2 if bidirectional else 1
        self.rnns = torch.nn.ModuleList([torch.nn.LSTM(inp if k == 0 else d * hidden, hidden, bidirectional=bidirectional) for k in range(layers)])
        self.head = torch.nn.Linear(d * hidden, out) if out else None

    def forward(self, x):
        x = x.squeeze(2).permute(2, 0, 1)
        for r in self.rnns:
            x, _ = r(x)
        return x if self.head is None else self.head(x)


def seeded_rnn(module: torch.nn.Module, seed: int) -> torch.nn.Module:
    """tools/onnx_export.py::seeded for the convolutions and the BatchNorm statistics; recurrent and linear weights uniform in +-1 / sqrt(fan-in)
    scaled so that the gates leave their linear range (saturating sigmoids and tanhs are part of what is checked)"""
    import onnx_export as X
    X.seeded(module, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.LSTM):
                for n, p in m.named_parameters():
                    p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (2.5 / m.hidden_size ** 0.5 if "weight" in n else 0.5))
            elif isinstance(m, torch.nn.BatchNorm2d):        # scales around 2 instead of seeded()'s around 0: the image survives four layers
                m.weight.copy_(2.0 + 0.3 * torch.randn(m.weight.shape, generator=g))
            elif isinstance(m, torch.nn.Linear):
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * (3.0 / m.in_features ** 0.5))
                m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2 - 1) * 0.3)
    return module.eval()


def onnx_lstm_params(rnn: torch.nn.LSTM):
    """one-layer nn.LSTM -> (W [D, 4H, I], R [D, 4H, H], B [D, 8H], direction) as the ONNX operator defines them: gate order i, o, f, c
    (torch keeps i, f, g, o), B = [Wb | Rb]"""
    assert rnn.num_layers == 1
    H = rnn.hidden_size

    def regate(a):
        i, f, g, o = a[0:H], a[H:2 * H], a[2 * H:3 * H], a[3 * H:4 * H]
        return torch.cat([i, o, f, g], 0)
    W, R, B = [], [], []
    for sfx in ("", "_reverse") if rnn.bidirectional else ("",):
        W.append(regate(getattr(rnn, "weight_ih_l0" + sfx).detach()))
        R.append(regate(getattr(rnn, "weight_hh_l0" + sfx).detach()))
        B.append(torch.cat([regate(getattr(rnn, "bias_ih_l0" + sfx).detach()), regate(getattr(rnn, "bias_hh_l0" + sfx).detach())]))
    return torch.stack(W).numpy(), torch.stack(R).numpy(), torch.stack(B).numpy(), "bidirectional" if rnn.bidirectional else "forward"


def write_lstm_node(W: np.ndarray, R: np.ndarray, B: Optional[np.ndarray], direction: str, batch: int, steps: int, initial_h: Optional[np.ndarray] = None,
                    initial_c: Optional[np.ndarray] = None, sequence_lens: Optional[np.ndarray] = None) -> bytes:
    """x [batch, I, 1, steps] -> Squeeze(2) -> Transpose(2, 0, 1) -> LSTM(direction) -> Y [T, D, B, H] -> Transpose(0, 2, 1, 3) -> Reshape
    -> y [T, B, D H]"""
    D, H4, I = W.shape
    H = H4 // 4
    m = OnnxModel(producer="pdf_table_amd.tools.onnx_export_rnn", graph_name="lstm_node")
    init = m.initializers
    init["W"], init["R"] = np.asarray(W, np.float32), np.asarray(R, np.float32)
    names = ["xt", "W", "R", "", "", "", ""]
    for pos, key, v in ((3, "B", B), (4, "sequence_lens", sequence_lens), (5, "initial_h", initial_h), (6, "initial_c", initial_c)):
        if v is not None:
            init[key] = np.asarray(v, np.int32 if key == "sequence_lens" else np.float32)
            names[pos] = key
    while names and names[-1] == "":
        names.pop()
    init["sq_axes"] = np.asarray([2], np.int64)
    init["y_shape"] = np.asarray([0, 0, -1], np.int64)
    m.nodes.append(OnnxNode("Squeeze", ["x", "sq_axes"], ["xs"], {}, name="Squeeze_1"))
    m.nodes.append(OnnxNode("Transpose", ["xs"], ["xt"], {"perm": [2, 0, 1]}, name="Transpose_2"))
    m.nodes.append(OnnxNode("LSTM", names, ["Y"], {"hidden_size": int(H), "direction": direction}, name="LSTM_3"))
    m.nodes.append(OnnxNode("Transpose", ["Y"], ["Yt"], {"perm": [0, 2, 1, 3]}, name="Transpose_4"))
    m.nodes.append(OnnxNode("Reshape", ["Yt", "y_shape"], ["y"], {}, name="Reshape_5"))
    m.inputs = [OnnxValueInfo("x", 1, (batch, I, 1, steps))]
    m.outputs = [OnnxValueInfo("y", 1, (steps, batch, D * H))]
    return serialize_model(m)


if __name__ == "__main__":
    import onnx_export as X
    path = sys.argv[1]
    data = X.torch_export(seeded_rnn(MobileCrnn(), 1), torch.zeros(1, 3, 48, 320), dynamic_batch=True)
    with open(path, "wb") as f:
        f.write(data)
    print(path, len(data), "bytes")
