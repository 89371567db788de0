"""Stand-ins with the GEOMETRY of PaddleOCR's text-line recognisers for the generic ONNX executor (pdf_table_amd/onnx_exec.py, csrc/rect_ops.hip) --
test / tooling code, not product.  Every PaddleOCR recogniser shrinks the image height and keeps its width: depthwise and dense convolutions of stride
(2,1) (PP-LCNetV3 also (1,2)), a last pool on a map of three rows, 1x3 convolutions in the SVTR neck.  The real ``*_rec_infer`` files are not available
offline; these seeded modules reproduce the layer geometry of PaddleOCR's published model definitions (ppocr/modeling/backbones/rec_mobilenet_v3.py,
rec_lcnetv3.py, rec_resnet_vd.py, necks/rnn.py) with channel counts that are deliberately NOT multiples of the GEMM tiles (24, 40, 96, 120), and go
through PyTorch's own exporter (tools/onnx_export.py::torch_export).

  * ``MobileV3RecLike``   the v2.0 mobile / PP-Table recognisers: inverted-residual blocks with depthwise strides (2,1), MaxPool2d(2) on 3 rows,
                          two BiLSTMs of 48 units, a CTC head with its Softmax.  [B, 3, 48, W] -> [B, W / 4, classes]
  * ``SvtrLcnetRecLike``  the v3 / v4 recognisers: depthwise-separable blocks with strides (2,1) and (1,2), avg_pool2d (3, 2), the SVTR neck with its
                          [1,3] convolutions around two global-mixing blocks.  [B, 3, 48, W] -> [B, W / 8, classes]
  * ``ResVdRecLike``      the ResNet-vd server recognisers' blocks: dense 3x3 of stride (2,1), AvgPool((2,1)) + 1x1 shortcuts, one [3,1] kernel, one
                          shortcut written as a 1x1 convolution of stride (2,1).  [B, 3, H, W] -> [B, 8, H / 4, W]
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onnx_export import SvtrBlock, torch_export  # noqa: E402


def _act(name):
    return {"relu": nn.ReLU, "hardswish": nn.Hardswish, "swish": nn.SiLU, None: nn.Identity}[name]()


def _cba(ci, co, k, stride=1, act=None, groups=1):
    """conv (padding k // 2 per axis) + BatchNorm + activation; k and stride are ints or (h, w) pairs"""
    k2 = (k, k) if isinstance(k, int) else tuple(k)
    return nn.Sequential(nn.Conv2d(ci, co, k2, stride, (k2[0] // 2, k2[1] // 2), groups=groups, bias=False), nn.BatchNorm2d(co), _act(act))


class _SE(nn.Module):
    def __init__(self, c, r=4):
        super().__init__()
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc1, self.fc2 = nn.Conv2d(c, c // r, 1), nn.Conv2d(c // r, c, 1)

    def forward(self, x):
        return x * F.hardsigmoid(self.fc2(torch.relu(self.fc1(self.pool(x)))))


class _InvRes(nn.Module):
    """MobileNetV3 block: 1x1 expand, depthwise k x k (stride per axis), optional SE, 1x1 project, residual where shapes allow"""

    def __init__(self, ci, mid, co, k, stride, se, act):
        super().__init__()
        self.expand = _cba(ci, mid, 1, 1, act)
        self.dw = _cba(mid, mid, k, stride, act, groups=mid)
        self.se = _SE(mid) if se else None
        self.project = _cba(mid, co, 1, 1, None)
        self.res = ci == co and stride in (1, (1, 1))

    def forward(self, x):
        y = self.dw(self.expand(x))
        if self.se is not None:
            y = self.se(y)
        y = self.project(y)
        return x + y if self.res else y


class MobileV3RecLike(nn.Module):
    """48 -> 24 -> 12 -> 6 -> 3 rows by the stem and three depthwise strides (2,1), MaxPool2d(2) -> 1 row (3 // 2: the third row is dropped) and
    W / 4 columns, squeeze / permute -> [T, B, 120] -> BiLSTM(48) x 2 -> Linear -> Softmax"""

    def __init__(self, classes: int = 97, hidden: int = 48):
        super().__init__()
        self.stem = _cba(3, 16, 3, 2, "hardswish")
        self.blocks = nn.Sequential(_InvRes(16, 16, 16, 3, 1, False, "relu"), _InvRes(16, 72, 24, 3, (2, 1), False, "relu"),
                                    _InvRes(24, 96, 24, 3, 1, False, "relu"), _InvRes(24, 96, 40, 5, (2, 1), True, "hardswish"),
                                    _InvRes(40, 120, 40, 5, 1, True, "hardswish"), _InvRes(40, 120, 96, 5, (2, 1), False, "hardswish"))
        self.last = _cba(96, 120, 1, 1, "hardswish")
        self.pool = nn.MaxPool2d(2)
        self.rnn1 = nn.LSTM(120, hidden, bidirectional=True)
        self.rnn2 = nn.LSTM(2 * hidden, hidden, bidirectional=True)
        self.head = nn.Linear(2 * hidden, classes)

    def logits(self, x):
        x = self.pool(self.last(self.blocks(self.stem(x))))
        x = x.squeeze(2).permute(2, 0, 1)                       # [T, B, C]
        x, _ = self.rnn1(x)
        x, _ = self.rnn2(x)
        return self.head(x).permute(1, 0, 2)                    # [B, T, classes]

    def forward(self, x):
        return torch.softmax(self.logits(x), dim=-1)


class _DwSep(nn.Module):
    def __init__(self, ci, co, k, stride, se):
        super().__init__()
        self.dw = _cba(ci, ci, k, stride, "hardswish", groups=ci)
        self.se = _SE(ci) if se else None
        self.pw = _cba(ci, co, 1, 1, "hardswish")

    def forward(self, x):
        x = self.dw(x)
        if self.se is not None:
            x = self.se(x)
        return self.pw(x)


class SvtrLcnetRecLike(nn.Module):
    """PP-LCNet-type backbone (48 -> 3 rows, W -> W / 4 columns; strides 1, (2,1), (1,2), 5x5 (2,1) with SE, 5x5 (2,1)), avg_pool2d (3, 2) -> 1 row and
    W / 8 columns, the SVTR neck (EncoderWithSVTR: [1,3] conv C -> C/8, 1x1 -> D, two global-mixing blocks, 1x1 -> C, Concat with the neck input,
    [1,3] conv 2C -> C/8, 1x1 -> D), Linear, Softmax"""

    def __init__(self, classes: int = 97, dim: int = 64, c: int = 120):
        super().__init__()
        self.c, self.dim = c, dim
        self.stem = _cba(3, 16, 3, 2, "hardswish")
        self.blocks = nn.Sequential(_DwSep(16, 24, 3, 1, False), _DwSep(24, 40, 3, (2, 1), False), _DwSep(40, 40, 3, (1, 2), False),
                                    _DwSep(40, 96, 5, (2, 1), True), _DwSep(96, c, 5, (2, 1), False))
        self.conv1, self.conv2 = _cba(c, c // 8, (1, 3), 1, "swish"), _cba(c // 8, dim, 1, 1, "swish")
        self.mix = nn.ModuleList([SvtrBlock(dim, 4, 2.0, "swish"), SvtrBlock(dim, 4, 2.0, "swish")])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.conv3 = _cba(dim, c, 1, 1, "swish")
        self.conv4, self.conv1x1 = _cba(2 * c, c // 8, (1, 3), 1, "swish"), _cba(c // 8, dim, 1, 1, "swish")
        self.head = nn.Linear(dim, classes)

    def logits(self, x):
        h = F.avg_pool2d(self.blocks(self.stem(x)), (3, 2))      # [B, C, 1, T]
        z = self.conv2(self.conv1(h))
        t = z.flatten(2).transpose(1, 2)                         # [B, T, D]
        for b in self.mix:
            t = b(t)
        t = self.norm(t)
        z = self.conv3(t.transpose(1, 2).reshape(t.shape[0], self.dim, 1, t.shape[1]))
        z = self.conv1x1(self.conv4(torch.cat([h, z], 1)))
        return self.head(z.squeeze(2).permute(0, 2, 1))          # [B, T, classes]

    def forward(self, x):
        return torch.softmax(self.logits(x), dim=-1)


class ResVdRecLike(nn.Module):
    """two ResNet-vd basic blocks whose first 3x3 has stride (2,1).  Block 1: its second convolution has a [3,1] kernel, its shortcut is
    AvgPool2d((2,1), (2,1), ceil_mode=True) + 1x1; block 2: a plain 3x3 second convolution and a shortcut written as a 1x1 convolution of stride (2,1).
    Add + ReLU, then a 1x1 head"""

    def __init__(self):
        super().__init__()
        self.stem = _cba(3, 24, 3, 1, "relu")
        self.b1a, self.b1b = _cba(24, 40, 3, (2, 1), "relu"), _cba(40, 40, (3, 1), 1, None)
        self.s1 = nn.Sequential(nn.AvgPool2d((2, 1), (2, 1), ceil_mode=True), _cba(24, 40, 1, 1, None))
        self.b2a, self.b2b = _cba(40, 96, 3, (2, 1), "relu"), _cba(96, 96, 3, 1, None)
        self.s2 = _cba(40, 96, 1, (2, 1), None)
        self.out = nn.Conv2d(96, 8, 1)

    def forward(self, x):
        x = self.stem(x)
        x = torch.relu(self.b1b(self.b1a(x)) + self.s1(x))
        x = torch.relu(self.b2b(self.b2a(x)) + self.s2(x))
        return self.out(x)


def seeded_pprec(module: nn.Module, seed: int, head_scale: float = 3.0) -> nn.Module:
    """Seeded parameters that keep the signal at scale ~1 through some twenty layers: He-normal convolutions, BatchNorm scales in 0.8 .. 1.2 with
    non-trivial statistics, LayerNorm scales around 1, recurrent weights as onnx_export_rnn.seeded_rnn draws them (the gates leave their linear
    range), linear layers uniform in +-1 / sqrt(fan-in), the CTC head ``head_scale`` times that"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, m in module.named_modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight[0].numel()) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.8 + 0.4 * torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.7 + 0.6 * torch.rand(m.running_var.shape, generator=g))
            elif isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.LSTM):
                for pn, p in m.named_parameters():
                    p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (2.5 / m.hidden_size ** 0.5 if "weight" in pn else 0.5))
            elif isinstance(m, nn.Linear):
                sc = head_scale if n == "head" else 1.0
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * (sc / m.in_features ** 0.5))
                m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2 - 1) * 0.1)
    return module.eval()


STAND_INS = {"mobilev3": MobileV3RecLike, "svtr_lcnet": SvtrLcnetRecLike, "resvd": ResVdRecLike}


if __name__ == "__main__":
    kind, path = sys.argv[1], sys.argv[2]
    net = seeded_pprec(STAND_INS[kind](), 1)
    example = torch.zeros(1, 3, 32, 48) if kind == "resvd" else torch.zeros(1, 3, 48, 320)
    data = torch_export(net, example, dynamic_batch=True)
    with open(path, "wb") as f:
        f.write(data)
    print(path, len(data), "bytes")
