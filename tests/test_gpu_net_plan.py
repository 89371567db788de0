"""The plumbing every net forward shares (csrc/net_ctx.h): the arena plan that is grown and re-planned, the missing-tensor error, the
weights-not-loaded error.  Results are compared bit for bit -- the same input on the same kernels -- so there is no tolerance here."""
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd import synth_weights as S
from pdf_table_amd import weights as Wt
from test_gpu_det import _x4

pytestmark = pytest.mark.gpu


def _engine():
    from pdf_table_amd.engine import HipEngine
    return HipEngine(0)


def _image(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, hw, hw, generator=g)


def _img4(n, hw, seed):
    return _x4(_image(n, hw, seed)).cuda()


def _img_f32(n, hw, seed):
    return _image(n, hw, seed).cuda()


def _lines_bf16(n, hw, seed):      # CRNN: gray lines [n, 32, 640]; the size is fixed, the batch grows
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 32, 640, generator=g).to(torch.bfloat16).cuda()


def _lines_f32(n, hw, seed):       # ConvNextViT: gray lines [n, 32, 804]
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 32, 804, generator=g).cuda()


def _tensors(out):
    """a net's result as a flat list of host tensors"""
    if isinstance(out, dict):
        return [out[k].cpu() for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [o.cpu() if torch.is_tensor(o) else torch.as_tensor(o) for o in out]
    return [out.cpu()]


def _decode(e, x):
    """tsr_forward_decode: rows past a table's count are never written, so only the counted rows are compared"""
    counts, dets, logi = e.tsr_forward_decode(x)
    dets, logi = dets.cpu(), logi.cpu()
    out = [torch.as_tensor(counts)]
    for i, c in enumerate(counts):
        out += [dets[i, :c].clone(), logi[i, :c].clone()]
    return out


_LORE = dict(seed=2, hm_bias=(-1.2, -0.6))      # heat-map biases at which the synthetic detector finds cells

# name -> (weights to load: [(kind, blob maker)], input maker, forward); A = input(1 or 2, 64), B = input(2 or 8, 128)
NETS = {
    "det_db_resnet18": ([(L.PT_MODEL_DB_RESNET18, lambda: Wt.pack_db_resnet18(S.db_resnet18_state_dict(seed=11)))], _img4,
                        lambda e, x: e.det_forward_net(x, want_logits=True)),
    "det_db_nas": ([(L.PT_MODEL_DB_NAS, lambda: Wt.pack_db_nas(S.db_nas_state_dict(seed=5)))], _img4, lambda e, x: e.det_forward_net(x, want_logits=True)),
    "layout": ([(L.PT_MODEL_PICODET, lambda: Wt.pack_picodet(S.picodet_state_dict(seed=4, num_classes=5), 5))], _img4, lambda e, x: e.layout_forward_net(x)),
    "cls": ([(L.PT_MODEL_PPLCNET, lambda: Wt.pack_pplcnet(S.pplcnet_state_dict(21, 2)))], _img4, lambda e, x: e.cls_forward_net(x, slot=0, textline=False)),
    "cls_textline": ([(L.PT_MODEL_PPLCNET, lambda: Wt.pack_pplcnet(S.pplcnet_state_dict(21, 2)))], _img4,
                     lambda e, x: e.cls_forward_net(x, slot=0, textline=True)),
    "tsr_dla34": ([(L.PT_MODEL_LORE_DLA34, lambda: Wt.pack_lore_dla34(S.lore_dla34_state_dict(**_LORE)))], _img4,
                  lambda e, x: e.tsr_forward_net(x, wireless=False)),
    "tsr_wireless": ([(L.PT_MODEL_LORE_RESNET18, lambda: Wt.pack_lore_wireless(S.lore_wireless_state_dict(seed=3)))], _img4,
                     lambda e, x: e.tsr_forward_net(x, wireless=True)),
    "tsr_decode": ([(L.PT_MODEL_LORE_DLA34, lambda: Wt.pack_lore_dla34(S.lore_dla34_state_dict(**_LORE)))], _img4, _decode),
    "centernet": ([(L.PT_MODEL_CENTERNET_DLA34, lambda: Wt.pack_centernet_dla34(S.centernet_dla34_state_dict(seed=3)))], _img4,
                  lambda e, x: e.centernet_forward_net(x)),
    "mtl_backbone": ([(L.PT_MODEL_MTL_BACKBONE, lambda: Wt.pack_mtl_backbone(S.mtl_tabnet_backbone_state_dict(seed=41)))], _img_f32,
                     lambda e, x: e.mtl_backbone_forward(x)),
    "rec_crnn": ([(L.PT_MODEL_CRNN, lambda: Wt.pack_crnn(S.crnn_state_dict(seed=1)))], _lines_bf16, lambda e, x: e.rec_forward_net(x)),
    "rec_cvit": ([(L.PT_MODEL_CONVNEXT_VIT, lambda: Wt.pack_convnext_vit(S.convnext_vit_state_dict(seed=29)))], _lines_f32,
                 lambda e, x: e.rec_cvit_forward_net(x)),
}


@pytest.mark.parametrize("name", list(NETS))
def test_replan_after_grow_is_bit_identical(name):
    """A (small), B (twice the batch at 128 x 128, 8 lines for the recognisers: a larger arena, so the plan grows it), A again: the first and
    the third result are the same bits, and the bits of an engine that never saw B.  Fails if the grow frees memory a pointer of the
    planning pass still refers to, or if the planning and the launching pass disagree on an offset."""
    loads, make, fwd = NETS[name]
    rec = name.startswith("rec_")
    a = make(2 if rec else 1, 64, 100)
    b = make(8 if rec else 2, 128, 101)
    blobs = [(kind, mk()) for kind, mk in loads]
    e1, e2 = _engine(), _engine()
    try:
        for e in (e1, e2):
            for kind, blob in blobs:
                e.load_weights(kind, blob)
        first = _tensors(fwd(e1, a))
        _tensors(fwd(e1, b))
        third = _tensors(fwd(e1, a))
        fresh = _tensors(fwd(e2, a))
    finally:
        e1.close()
        e2.close()
    assert len(first) == len(third) == len(fresh) and len(first) > 0
    if name == "tsr_decode":
        assert int(first[0].sum()) > 0, "the synthetic detector finds no cell: nothing would be compared"
    for i, (x, y, z) in enumerate(zip(first, third, fresh)):
        assert x.shape == y.shape == z.shape, (name, i)
        assert torch.equal(x, y), f"{name}: output {i} differs after the arena grew for a larger input"
        assert torch.equal(x, z), f"{name}: output {i} differs from an engine that never grew"


def _pack_without(pack, drop):
    """pack()'s blob with the tensor `drop` left out of the container"""
    orig = Wt.write_blob
    seen = []

    def write(items):
        seen.append(drop in items)
        return orig({k: v for k, v in items.items() if k != drop})

    Wt.write_blob = write
    try:
        blob = pack()
    finally:
        Wt.write_blob = orig
    assert seen == [True], f"the packer writes no tensor '{drop}'"
    return blob


# one net per context family: DlaCtx, the layout Ctx, a model file's conv lambda
MISSING = {
    "centernet": (L.PT_MODEL_CENTERNET_DLA34, lambda: Wt.pack_centernet_dla34(S.centernet_dla34_state_dict(seed=3)), "dla_up.ida_1.node_1.b",
                  "CenterNet DLA-34", _img4, lambda e, x: e.centernet_forward_net(x)),
    "picodet": (L.PT_MODEL_PICODET, lambda: Wt.pack_picodet(S.picodet_state_dict(seed=4, num_classes=5), 5), "neck.td1.dp.dw.wf32", "PicoDet", _img4,
                lambda e, x: e.layout_forward_net(x)),
    "mtl_backbone": (L.PT_MODEL_MTL_BACKBONE, lambda: Wt.pack_mtl_backbone(S.mtl_tabnet_backbone_state_dict(seed=41)), "layer2.0.conv2.b",
                     "MtlTabNet backbone", _img_f32, lambda e, x: e.mtl_backbone_forward(x)),
}


@pytest.mark.parametrize("name", list(MISSING))
def test_missing_tensor_names_net_and_tensor(name):
    kind, pack, drop, what, make, fwd = MISSING[name]
    x = make(1, 64, 7)
    e = _engine()
    try:
        e.load_weights(kind, _pack_without(pack, drop))
        with pytest.raises(L.PtError) as ei:
            fwd(e, x)
        msg = str(ei.value)
        assert what in msg and f"lacks tensor '{drop}'" in msg, msg
        e.load_weights(kind, pack())      # the latched error left nothing behind: the complete blob runs on the same engine
        out = _tensors(fwd(e, x))
        assert len(out) > 0 and all(bool(torch.isfinite(o.float()).all()) for o in out)
    finally:
        e.close()


def test_centernet_not_loaded_fails_loudly():
    e = _engine()
    try:
        with pytest.raises(L.PtError, match="CenterNet DLA-34 weights not loaded"):
            e.centernet_forward_net(_img4(1, 64, 0))
    finally:
        e.close()
