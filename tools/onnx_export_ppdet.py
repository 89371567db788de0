"""Stand-ins with the GEOMETRY of the PP-OCRv4 mobile models for the generic ONNX executor (pdf_table_amd/onnx_exec.py, csrc/det_ops.hip) -- test /
tooling code, not product.  The real ``ch_PP-OCRv4_det_infer`` / ``ch_PP-OCRv4_rec_infer`` files are not available offline: what is served here is
their LAYER GEOMETRY, written from PaddleOCR's published model definitions (ppocr/modeling/backbones/rec_lcnetv3.py, necks/db_fpn.py::RSEFPN,
heads/det_db_head.py) and from memory -- still a stand-in, with seeded weights, not the shipped graphs.  Exported through PyTorch's own exporter
(tools/onnx_export.py::torch_export).

  * ``LcnetV3DetLike``   the v4 mobile detector after re-parameterisation: PP-LCNetV3 x 0.75 (every re-parameterised convolution followed by a
                         LearnableAffineBlock ``scale x + bias`` with two learned scalars, every hardswish by a second one; SE with PaddleOCR's
                         HardSigmoid(0.2, 0.5)), taps at strides 4 .. 32 projected to 16 / 24 / 56 / 360 channels (off the GEMM tile sizes on
                         purpose), the RSE-FPN neck (96 channels, shortcut) and the DB head (Conv3x3 96 -> 24, two 2x2 transposed convolutions,
                         Sigmoid).  [B, 3, H, W] -> [B, 1, H, W], H and W multiples of 32
  * ``LcnetV3RecLike``   the same blocks with the recogniser's strides ((1,1), (2,1), (1,2), (2,1) where the detector has 2), the six remaining rows
                         averaged to one, and behind it the SVTR neck and CTC head of ``onnx_export_pprec.SvtrLcnetRecLike`` (inherited, not copied).
                         [B, 3, 48, W] -> [B, W / 8, classes]

    python tools/onnx_export_ppdet.py [det|rec] [out.onnx]      # exports the stand-in and prints the importer's layer inventory
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from onnx_export import torch_export  # noqa: E402
from onnx_export_pprec import SvtrLcnetRecLike, seeded_pprec  # noqa: E402


class _PaddleHardSigmoid(torch.autograd.Function):
    """PaddleOCR's hardsigmoid(slope 0.2, offset 0.5): an ONNX HardSigmoid node with those attributes (torch's own has 1 / 6)"""

    @staticmethod
    def forward(ctx, x):
        return torch.clamp(0.2 * x + 0.5, 0.0, 1.0)

    @staticmethod
    def symbolic(g, x):
        return g.op("HardSigmoid", x, alpha_f=0.2, beta_f=0.5)


class LAB(nn.Module):
    """LearnableAffineBlock: scale x + bias, two learned scalars"""

    def __init__(self):
        super().__init__()
        self.scale, self.bias = nn.Parameter(torch.ones(1)), nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return self.scale * x + self.bias


class Act(nn.Module):
    def __init__(self):
        super().__init__()
        self.act, self.lab = nn.Hardswish(), LAB()

    def forward(self, x):
        return self.lab(self.act(x))


class Rep(nn.Module):
    """a RepLayer after re-parameterisation: one convolution with bias, LAB, and the activation (with its own LAB) unless the layer strides"""

    def __init__(self, cin, cout, k, s, groups):
        super().__init__()
        s2 = (s, s) if isinstance(s, int) else tuple(s)
        self.conv, self.lab = nn.Conv2d(cin, cout, k, s2, k // 2, groups=groups, bias=True), LAB()
        self.act = Act() if s2 == (1, 1) else None

    def forward(self, x):
        x = self.lab(self.conv(x))
        return x if self.act is None else self.act(x)


class SE(nn.Module):
    def __init__(self, c, r=4):
        super().__init__()
        self.fc1, self.fc2 = nn.Conv2d(c, c // r, 1), nn.Conv2d(c // r, c, 1)

    def forward(self, x):
        g = self.fc2(torch.relu(self.fc1(F.adaptive_avg_pool2d(x, 1))))
        return x * _PaddleHardSigmoid.apply(g)


class Block(nn.Module):
    def __init__(self, cin, cout, k, s, se):
        super().__init__()
        self.dw = Rep(cin, cin, k, s, cin)
        self.se = SE(cin) if se else None
        self.pw = Rep(cin, cout, 1, 1, 1)

    def forward(self, x):
        x = self.dw(x)
        if self.se is not None:
            x = self.se(x)
        return self.pw(x)


#           k  cin  cout  se     (x 0.75, channels rounded to 16); a stage = the blocks up to the next stride
_STAGES = [[(3, 16, 32, False)],
           [(3, 32, 48, False), (3, 48, 48, False)],
           [(3, 48, 96, False), (3, 96, 96, False)],
           [(3, 96, 192, False)] + [(5, 192, 192, False)] * 4,
           [(5, 192, 384, True), (5, 384, 384, True), (5, 384, 384, False), (5, 384, 384, False)]]


def _stages(strides):
    """strides: of the FIRST block of stages 1 .. 4 (stage 0 does not stride)"""
    out = []
    for si, blocks in enumerate(_STAGES):
        out.append(nn.Sequential(*[Block(ci, co, k, (strides[si - 1] if (bi == 0 and si > 0) else 1), se) for bi, (k, ci, co, se) in enumerate(blocks)]))
    return nn.ModuleList(out)


class _RseLevel(nn.Module):
    """RSELayer with shortcut: conv (no bias), out = conv + SE(conv)"""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv, self.se = nn.Conv2d(cin, cout, k, 1, k // 2, bias=False), SE(cout)

    def forward(self, x):
        c = self.conv(x)
        return c + self.se(c)


class LcnetV3DetLike(nn.Module):
    def __init__(self):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 16, 3, 2, 1, bias=False), nn.BatchNorm2d(16))
        self.stages = _stages((2, 2, 2, 2))
        self.proj = nn.ModuleList([nn.Conv2d(ci, co, 1) for ci, co in ((48, 16), (96, 24), (192, 56), (384, 360))])
        self.ins = nn.ModuleList([_RseLevel(c, 96, 1) for c in (16, 24, 56, 360)])
        self.inp = nn.ModuleList([_RseLevel(96, 24, 3) for _ in range(4)])
        self.head = nn.Sequential(nn.Conv2d(96, 24, 3, 1, 1, bias=False), nn.BatchNorm2d(24), nn.ReLU(),
                                  nn.ConvTranspose2d(24, 24, 2, 2), nn.BatchNorm2d(24), nn.ReLU(), nn.ConvTranspose2d(24, 1, 2, 2), nn.Sigmoid())

    def neck(self, x):
        x = self.stages[0](self.stem(x))
        taps = []
        for st, pr in zip(self.stages[1:], self.proj):
            x = st(x)
            taps.append(pr(x))
        i2, i3, i4, i5 = (m(t) for m, t in zip(self.ins, taps))
        up = lambda t, f: F.interpolate(t, scale_factor=f, mode="nearest")      # noqa: E731
        i4 = i4 + up(i5, 2)
        i3 = i3 + up(i4, 2)
        i2 = i2 + up(i3, 2)
        p2, p3, p4, p5 = (m(t) for m, t in zip(self.inp, (i2, i3, i4, i5)))
        return torch.cat([up(p5, 8), up(p4, 4), up(p3, 2), p2], 1)

    def forward(self, x):
        return self.head(self.neck(x))


class LcnetV3RecLike(SvtrLcnetRecLike):
    """SvtrLcnetRecLike with the PP-LCNetV3 backbone: 48 -> 6 rows and W -> W / 4 columns by the stem and the strides (1,1), (2,1), (1,2), (2,1); the six
    rows are averaged in two steps -- AvgPool (2,1) here, the (3, 2) pool of the inherited ``logits`` (which also halves the width: T = W / 8) -- an
    average of averages over equal windows.  Neck, head and forward are the base class's."""

    def __init__(self, classes: int = 97, dim: int = 64):
        super().__init__(classes=classes, dim=dim, c=384)
        self.stem = nn.Sequential(nn.Conv2d(3, 16, 3, 2, 1, bias=False), nn.BatchNorm2d(16))
        self.blocks = nn.Sequential(*_stages(((1, 1), (2, 1), (1, 2), (2, 1))), nn.AvgPool2d((2, 1)))


class AffineRulesLike(nn.Module):
    """three blocks, one per rule of the importer's constant-affine handling, then a zero-padded 3x3 convolution:
      1. conv -> LAB -> hardswish -> LAB      the first LAB folds into the convolution, the hardswish fuses into its epilogue, the second is a kernel
      2. relu(conv(x) + x) -> LAB             a stand-alone activation in front of a LAB: one launch
      3. pool -> * a[C,1,1] -> + 0.3 -> * 1.7 -> - 0.2 -> / 1.25     a chain collapses into one (s, b); x - c and x / c fold
    ``reversed_sub``: the last convolution reads 1 - w instead (c - x: refused by name)"""

    def __init__(self, reversed_sub: bool = False):
        super().__init__()
        self.reversed_sub = reversed_sub
        self.conv1, self.lab1, self.act1 = nn.Conv2d(3, 24, 3, 1, 1), LAB(), Act()
        self.conv2, self.lab2 = nn.Conv2d(24, 24, 3, 1, 1), LAB()
        self.pool = nn.AvgPool2d(2)
        self.a = nn.Parameter(torch.ones(24, 1, 1))
        self.conv3 = nn.Conv2d(24, 8, 3, 1, 1)

    def forward(self, x):
        x = self.act1(self.lab1(self.conv1(x)))
        y = self.lab2(torch.relu(self.conv2(x) + x))
        w = ((self.pool(y) * self.a + 0.3) * 1.7 - 0.2) / 1.25
        return self.conv3(1.0 - w if self.reversed_sub else w)


def seeded_ppdet(module: nn.Module, seed: int, head_scale: float = 3.0, example: torch.Tensor = None, blob_map: bool = False) -> nn.Module:
    """``onnx_export_pprec.seeded_pprec`` plus what these modules add: every LAB drawn AWAY from the identity (scale in 0.7 .. 0.9 or 1.1 .. 1.3, bias of
    magnitude 0.05 .. 0.25), the transposed convolutions He-normal, and -- for the two PP-LCNetV3 stand-ins -- every convolution scaled to unit output
    variance on ``example`` (default: a seeded random batch; see _unit_scale).

    ``blob_map`` (detector only): a probability map made of regions instead of pixel noise, as a trained text detector's is, so that the box stage behind
    it has components to work on.  A seeded head answers every pixel on its own: its transposed convolutions draw independent weights for the four
    sub-positions (a 4 x 4 checkerboard), and the stride-4 / stride-8 levels of the neck carry pixel-scale detail.  With the flag the transposed convolutions
    up-sample smoothly -- the weights of the four sub-positions are their common mean (doubled) plus a twentieth of the drawn deviation, so still different
    per sub-position -- the head's 3x3 convolution reads the two coarse levels only (its weights on the stride-8 and stride-4 channels are zero), and the
    logits are centred: their mean on ``example`` is ``logit_shift``."""
    seeded_pprec(module, seed, head_scale=head_scale)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, LAB):
                sg = 1.0 if float(torch.rand(1, generator=g)) < 0.5 else -1.0
                m.scale.fill_(1.0 + sg * (0.1 + 0.2 * float(torch.rand(1, generator=g))))
                sg = 1.0 if float(torch.rand(1, generator=g)) < 0.5 else -1.0
                m.bias.fill_(sg * (0.05 + 0.2 * float(torch.rand(1, generator=g))))
            elif isinstance(m, nn.ConvTranspose2d):
                w = torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight.shape[0]) ** 0.5
                if blob_map:
                    mean = w.mean((2, 3), keepdim=True)
                    w = 2.0 * mean + 0.05 * (w - mean)
                m.weight.copy_(w)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, AffineRulesLike):
                m.a.copy_(0.5 + torch.rand(m.a.shape, generator=g))
        if blob_map:
            module.head[0].weight[:, 48:] = 0.0           # the concat is [up8(p5), up4(p4), up2(p3), p2], 24 channels each
    module.eval()
    if isinstance(module, (LcnetV3DetLike, LcnetV3RecLike)):
        _unit_scale(module, torch.randn(2, 3, 48 if isinstance(module, LcnetV3RecLike) else 64, 96, generator=g) if example is None else example, centre=blob_map)
    return module


def _unit_scale(module: nn.Module, example: torch.Tensor, logit_scale: float = 2.0, logit_shift: float = -3.0, centre: bool = False) -> None:
    """Data-dependent scaling of the seeded weights, as a trained network's normalisation would leave them: in ONE forward pass of a fixed random batch every
    convolution's weights and bias are divided by the standard deviation of its own output (layer-sequential unit variance), so that some sixty layers of
    LABs, SE gates and FPN sums neither blow the signal up nor let it die -- without it the detector's logits saturate the sigmoid everywhere.  The last
    transposed convolution of a detector head is left at ``logit_scale`` and its bias moved by ``logit_shift``: probabilities that spread over (0, 1) with
    a minority above 0.3, as a text map has (``centre``: the bias is set so that the logits' mean on ``example`` IS ``logit_shift``, whatever the mean of
    the seeded layer was)."""
    convs = [m for m in module.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
    last = convs[-1] if isinstance(module, LcnetV3DetLike) else None

    def hook(m, _inp, out):
        sd = float(out.std())
        f = (logit_scale if m is last else 1.0) / max(sd, 1e-6)
        move = (logit_shift - (float(out.mean()) * f if centre else 0.0)) if m is last else 0.0
        with torch.no_grad():
            m.weight.mul_(f)
            if m.bias is not None:
                m.bias.mul_(f)
                if m is last:
                    m.bias.add_(move)
        return out * f + move
    handles = [m.register_forward_hook(hook) for m in convs]
    with torch.no_grad():
        module(example)
    for h in handles:
        h.remove()


STAND_INS = {"det": (LcnetV3DetLike, (1, 3, 64, 96)), "rec": (LcnetV3RecLike, (1, 3, 48, 320))}


if __name__ == "__main__":
    from pdf_table_amd.onnx_import import load_onnx
    kind = sys.argv[1] if len(sys.argv) > 1 else "det"
    cls, shape = STAND_INS[kind]
    net = seeded_ppdet(cls(), 1)
    data = torch_export(net, torch.zeros(*shape), dynamic_batch=(kind == "rec"))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "wb") as f:
            f.write(data)
    layers = load_onnx(data).layers()
    inv = {}
    for lay in layers:
        inv[lay.op] = inv.get(lay.op, 0) + 1
    folded = sum(1 for lay in layers if lay.attrs.get("affine_folded"))
    print(f"{cls.__name__}: {len(data)} bytes, {len(layers)} layers: " + ", ".join(f"{k} x{v}" for k, v in sorted(inv.items()))
          + f"; {folded} convolutions with a folded affine")
