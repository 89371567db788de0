"""A stand-in with the GEOMETRY of the PP-OCRv4 SERVER detector for the generic ONNX executor (pdf_table_amd/onnx_exec.py, csrc/large_conv.hip) -- test /
tooling code, not product.  The real ``ch_PP-OCRv4_det_server_infer`` file is not available offline: what is served here is its LAYER GEOMETRY, written
from PaddleOCR's published model definitions (ppocr/modeling/backbones/rec_hgnet.py / det PP-HGNet, necks/db_fpn.py::LKPAN with necks/intracl.py,
heads/det_db_head.py::PFHeadLocal) and from memory -- still a stand-in, with seeded weights and reduced widths, not the shipped graph.  Exported through
PyTorch's own exporter (tools/onnx_export.py::torch_export).

  * ``HgnetLkpanDetLike``   PP-HGNet-like backbone: a stem of three 3x3 ConvBNReLU (the first of stride 2) and MaxPool(3, 2, 1), then four stages of HG
                            blocks -- six 3x3 ConvBNReLU, a Concat of the input and all six outputs, a 1x1 aggregation, an ESE gate (global mean -> 1x1
                            -> sigmoid -> multiply), an identity residual in all but a stage's first block -- with a depthwise 3x3 / stride-2
                            down-sampler (BN, no activation) in front of stages 2 .. 4 (the published detector backbone does not down-sample its first
                            stage: the taps are at strides 4, 8, 16, 32); mid widths off the GEMM tile sizes.
                            LKPAN neck ("large" mode): 1x1 laterals, nearest x2 top-down adds, a 9x9 ``inp_conv`` per level (C -> C/4), 3x3 / stride-2
                            ``pan_head`` with adds, a 9x9 ``pan_lat`` per level, an IntraCL block per level (1x1 reduce to half the channels, three
                            rounds of c_kxk + v_kx1 + q_1xk for k = 7, 5, 3, 1x1 back, BN, ReLU, plus the input), nearest x8 / x4 / x2 and a Concat.
                            PFHeadLocal: the DB head (3x3, ConvT 2x2 / 2 + ReLU, ConvT 2x2 / 2, Sigmoid) and the local branch (nearest x2 of the first
                            ConvT's output concatenated with the base map, 3x3 + ReLU, 1x1, Sigmoid); output 0.5 (base + local).
                            [B, 3, H, W] -> [B, 1, H, W], H and W multiples of 32

    python tools/onnx_export_ppdet_server.py [out.onnx]      # exports the stand-in and prints the importer's layer inventory
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
from onnx_export_pprec import seeded_pprec  # noqa: E402


def _cbr(cin, cout, k, s=1, groups=1, act=True):
    mods = [nn.Conv2d(cin, cout, k, s, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout)]
    return nn.Sequential(*(mods + [nn.ReLU()] if act else mods))


class HgBlock(nn.Module):
    def __init__(self, cin, mid, cout, identity, layers=6):
        super().__init__()
        self.identity = identity
        self.layers = nn.ModuleList([_cbr(cin if i == 0 else mid, mid, 3) for i in range(layers)])
        self.agg = _cbr(cin + layers * mid, cout, 1)
        self.ese = nn.Conv2d(cout, cout, 1)

    def forward(self, x):
        outs = [x]
        for lay in self.layers:
            outs.append(lay(outs[-1]))
        y = self.agg(torch.cat(outs, 1))
        y = y * torch.sigmoid(self.ese(F.adaptive_avg_pool2d(y, 1)))
        return y + x if self.identity else y


class HgStage(nn.Module):
    def __init__(self, cin, mid, cout, blocks, down):
        super().__init__()
        self.down = _cbr(cin, cin, 3, 2, groups=cin, act=False) if down else None
        self.blocks = nn.Sequential(*[HgBlock(cin if i == 0 else cout, mid, cout, identity=i > 0) for i in range(blocks)])

    def forward(self, x):
        return self.blocks(x if self.down is None else self.down(x))


class IntraCL(nn.Module):
    def __init__(self, c, reduce_factor=2):
        super().__init__()
        r = c // reduce_factor
        self.reduce, self.back, self.bn = nn.Conv2d(c, r, 1), nn.Conv2d(r, c, 1), nn.BatchNorm2d(c)
        self.c = nn.ModuleList([nn.Conv2d(r, r, k, 1, k // 2) for k in (7, 5, 3)])
        self.v = nn.ModuleList([nn.Conv2d(r, r, (k, 1), 1, (k // 2, 0)) for k in (7, 5, 3)])
        self.q = nn.ModuleList([nn.Conv2d(r, r, (1, k), 1, (0, k // 2)) for k in (7, 5, 3)])

    def forward(self, x):
        y = self.reduce(x)
        for c, v, q in zip(self.c, self.v, self.q):
            y = c(y) + v(y) + q(y)
        return x + torch.relu(self.bn(self.back(y)))


#          cin  mid  cout blocks down      (the real net: mid 32 .. 224 with 160 / 192 / 224 off the tile sizes, out 128 .. 1024)
_STAGES = [(24, 20, 48, 1, False), (48, 28, 96, 1, True), (96, 40, 160, 2, True), (160, 56, 256, 1, True)]


class HgnetLkpanDetLike(nn.Module):
    def __init__(self, neck: int = 96, stages=_STAGES):
        super().__init__()
        c, q = neck, neck // 4
        self.q = q
        self.stem = nn.Sequential(_cbr(3, 16, 3, 2), _cbr(16, 16, 3), _cbr(16, stages[0][0], 3), nn.MaxPool2d(3, 2, 1))
        self.stages = nn.ModuleList([HgStage(*s) for s in stages])
        taps = [s[2] for s in stages]
        self.ins = nn.ModuleList([nn.Conv2d(t, c, 1, bias=False) for t in taps])
        self.inp = nn.ModuleList([nn.Conv2d(c, q, 9, 1, 4, bias=False) for _ in taps])
        self.pan_head = nn.ModuleList([nn.Conv2d(q, q, 3, 2, 1, bias=False) for _ in taps[1:]])
        self.pan_lat = nn.ModuleList([nn.Conv2d(q, q, 9, 1, 4, bias=False) for _ in taps])
        self.incl = nn.ModuleList([IntraCL(q) for _ in taps])
        # PFHeadLocal: binarize = 3x3 + BN + ReLU, convT + BN + ReLU (-> f), convT (-> base logits); local = 3x3 + BN + ReLU on [base | up2(f)], 1x1
        self.head = nn.Sequential(nn.Conv2d(c, q, 3, 1, 1, bias=False), nn.BatchNorm2d(q), nn.ReLU())
        self.up1 = nn.Sequential(nn.ConvTranspose2d(q, q, 2, 2), nn.BatchNorm2d(q), nn.ReLU())
        self.up2 = nn.ConvTranspose2d(q, 1, 2, 2)
        self.local3 = _cbr(q + 1, q, 3)
        self.local1 = nn.Conv2d(q, 1, 1)

    def neck(self, x):
        x = self.stem(x)
        taps = []
        for st in self.stages:
            x = st(x)
            taps.append(x)
        i2, i3, i4, i5 = (m(t) for m, t in zip(self.ins, taps))
        up = lambda t, f: F.interpolate(t, scale_factor=f, mode="nearest")      # noqa: E731
        o4 = i4 + up(i5, 2)
        o3 = i3 + up(o4, 2)
        o2 = i2 + up(o3, 2)
        f2, f3, f4, f5 = (m(t) for m, t in zip(self.inp, (o2, o3, o4, i5)))
        pan3 = f3 + self.pan_head[0](f2)
        pan4 = f4 + self.pan_head[1](pan3)
        pan5 = f5 + self.pan_head[2](pan4)
        p2, p3, p4, p5 = (ic(m(t)) for ic, m, t in zip(self.incl, self.pan_lat, (f2, pan3, pan4, pan5)))
        return torch.cat([up(p5, 8), up(p4, 4), up(p3, 2), p2], 1)

    def forward(self, x):
        f = self.up1(self.head(self.neck(x)))
        base = torch.sigmoid(self.up2(f))
        both = torch.cat([base, F.interpolate(f, scale_factor=2, mode="nearest")], 1)
        local = torch.sigmoid(self.local1(self.local3(both)))
        return 0.5 * (base + local)


def seeded_ppdet_server(module: HgnetLkpanDetLike, seed: int, example: torch.Tensor = None, blob_map: bool = False, logit_scale: float = 2.0,
                        logit_shift: float = -3.0) -> HgnetLkpanDetLike:
    """``onnx_export_pprec.seeded_pprec`` (He-normal convolutions, BatchNorm away from the identity) plus He-normal transposed convolutions, and every
    convolution scaled to unit output variance on ``example`` (default: a seeded random batch) in one forward pass, as ``onnx_export_ppdet._unit_scale``
    does for the mobile stand-in: some ninety layers of gates and pyramid sums then neither blow the signal up nor let it die.  The two logit layers (the
    second transposed convolution and the local branch's 1x1) are left at ``logit_scale`` with a bias of ``logit_shift``.

    ``blob_map``: a probability map made of regions instead of pixel noise, as a trained text detector's is, so that the box stage behind it has components
    to work on -- the transposed convolutions up-sample smoothly (the four sub-positions share their mean, doubled, plus a twentieth of the drawn
    deviation), the head's 3x3 convolution reads the two coarse levels only, the local branch's 3x3 reads its centre tap only, and both logit layers are
    centred: their mean on ``example`` is ``logit_shift``."""
    seeded_pprec(module, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.ConvTranspose2d):
                w = torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight.shape[0]) ** 0.5
                if blob_map:
                    mean = w.mean((2, 3), keepdim=True)
                    w = 2.0 * mean + 0.05 * (w - mean)
                m.weight.copy_(w)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
        if blob_map:
            module.head[0].weight[:, 2 * module.q:] = 0.0         # the concat is [up8(p5), up4(p4), up2(p3), p2], q channels each
            w3 = module.local3[0].weight
            centre = w3[:, :, 1, 1].clone()
            w3.zero_()
            w3[:, :, 1, 1] = centre
    module.eval()
    if example is None:
        example = torch.randn(2, 3, 64, 96, generator=g)
    convs = [m for m in module.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
    logits = (module.up2, module.local1)

    def hook(m, _inp, out):
        sd = float(out.std())
        f = (logit_scale if m in logits else 1.0) / max(sd, 1e-6)
        move = (logit_shift - (float(out.mean()) * f if blob_map else 0.0)) if m in logits else 0.0
        with torch.no_grad():
            m.weight.mul_(f)
            if m.bias is not None:
                m.bias.mul_(f)
                if m in logits:
                    m.bias.add_(move)
        return out * f + move
    handles = [m.register_forward_hook(hook) for m in convs]
    with torch.no_grad():
        module(example)
    for h in handles:
        h.remove()
    return module


if __name__ == "__main__":
    from pdf_table_amd.onnx_import import load_onnx
    net = seeded_ppdet_server(HgnetLkpanDetLike(), 1)
    data = torch_export(net, torch.zeros(1, 3, 64, 96))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "wb") as f:
            f.write(data)
    layers = load_onnx(data).layers()
    inv = {}
    for lay in layers:
        inv[lay.op] = inv.get(lay.op, 0) + 1
    large = sorted({"%dx%d" % tuple(lay.attrs["kernel"]) for lay in layers if lay.op == "conv" and lay.attrs.get("group", 1) == 1 and max(lay.attrs["kernel"]) >= 5})
    print(f"HgnetLkpanDetLike: {len(data)} bytes, {len(layers)} layers: " + ", ".join(f"{k} x{v}" for k, v in sorted(inv.items()))
          + "; large dense kernels: " + ", ".join(large))
