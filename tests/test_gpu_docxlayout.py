"""DocXLayout's network and pre-process on the engine: pt_docx_forward_net against the reference's fixture and the CPU restatement
(tests/docxlayout_ref.py, pinned by tests/test_docxlayout_host.py), pt_docx_preprocess against the warpAffine restatement in oracle/."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docxlayout_ref as R  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.docxlayout_stage import DOCX_MEAN, DOCX_STD  # noqa: E402
from pdf_table_amd.engine import TSR_TABLE_DTYPE  # noqa: E402
from pdf_table_amd.synth_weights import docxlayout_dla34_state_dict  # noqa: E402
from pdf_table_amd.weights import pack_docxlayout_dla34  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_REL = 1e-3      # relative to max(1, max|head|): the bound tests/test_gpu_centernet.py holds the same kernels to


def _x4(x, split=False, dtype=torch.bfloat16):
    n, _, H, W = x.shape
    nhwc = x.permute(0, 2, 3, 1)
    if not split:
        x4 = torch.zeros(n, H, W, 4)
        x4[..., :3] = nhwc
        return x4.to(dtype)
    hi = nhwc.to(torch.bfloat16).float()
    lo = (nhwc - hi).to(torch.bfloat16).float()
    x8 = torch.zeros(n, H, W, 8)
    x8[..., :3] = hi
    x8[..., 4:7] = lo
    return x8.to(torch.bfloat16)


@pytest.fixture(scope="module")
def gold_sd(golden_dir):
    return docxlayout_dla34_state_dict(seed=int(np.load(os.path.join(golden_dir, "docxlayout_dla34.npz"))["seed"]))


@pytest.fixture(scope="module")
def eng(gold_sd):
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    e.load_weights(L.PT_MODEL_DOCX_DLA34, pack_docxlayout_dla34(gold_sd))
    yield e
    e.close()


def _rel(got, ref):
    worst = 0.0
    for k, c in R.HEADS.items():
        g = got[k].cpu()[..., :c].permute(0, 3, 1, 2)
        r = ref[k].float()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        worst = max(worst, (g - r).abs().max().item() / max(1.0, r.abs().max().item()))
    return worst


def test_net_x3_matches_reference_golden(eng, golden_dir):
    gold = np.load(os.path.join(golden_dir, "docxlayout_dla34.npz"))
    eng.set_precision(L.PT_PRECISION_BF16X3)
    try:
        for tag in ("a", "b"):
            got = eng.docx_forward_net(_x4(torch.from_numpy(gold[f"x_{tag}"]), split=True).cuda())
            torch.cuda.synchronize()
            assert got["hm"].shape[-1] == 16 and all(got[k].shape[-1] == 8 for k in R.HEADS if k != "hm")
            rel = _rel(got, {k: torch.from_numpy(gold[f"{k}_{tag}"]) for k in R.HEADS})
            print(f"docxlayout x3 vs reference [{tag}]: {rel:.2e}")
            assert rel <= TOL_REL, (tag, rel)
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)


def test_net_x3_matches_restatement_at_the_batch_seam(eng, gold_sd):
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(596))
    with torch.no_grad():
        ref = R.docx_forward(gold_sd, x)
    eng.set_precision(L.PT_PRECISION_BF16X3)
    try:
        got = eng.docx_forward_net(_x4(x, split=True).cuda())
        torch.cuda.synchronize()
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    rel = _rel(got, ref)
    print(f"docxlayout x3 (2, 64, 96): {rel:.2e}")
    assert rel <= TOL_REL


def test_net_bf16_and_f16_drift(eng, gold_sd):
    """the bound is 4 x the distance of the restatement run in that dtype on the CPU from its fp32 run on the same input, measured here"""
    from pdf_table_amd.engine import HipEngine
    x = torch.randn(1, 3, 128, 160, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).float()      # exact in both 16-bit formats' range
    x = x.to(torch.float16).float().to(torch.bfloat16).float()
    with torch.no_grad():
        ref = R.docx_forward(gold_sd, x)
        cpu = {}
        for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            z = R.docx_forward(gold_sd, x.to(dt))
            cpu[name] = max((z[k].float() - ref[k]).abs().max().item() / max(1.0, ref[k].abs().max().item()) for k in R.HEADS)
    rel = _rel(eng.docx_forward_net(_x4(x).cuda()), ref)
    e16 = HipEngine(0)
    try:
        e16.set_precision(L.PT_PRECISION_F16)
        e16.load_weights(L.PT_MODEL_DOCX_DLA34, pack_docxlayout_dla34(gold_sd, fmt="f16"))
        rel16 = _rel(e16.docx_forward_net(_x4(x, dtype=torch.float16).cuda()), ref)
    finally:
        e16.close()
    print(f"docxlayout drift: bf16 engine {rel:.3e} (CPU bf16 {cpu['bf16']:.3e}, bound {4 * cpu['bf16']:.3e}); "
          f"f16 engine {rel16:.3e} (CPU f16 {cpu['f16']:.3e}, bound {4 * cpu['f16']:.3e})")
    assert rel <= 4 * cpu["bf16"] and rel16 <= 4 * cpu["f16"]


def _tables(n, ph, pw, inp_h, inp_w):
    from pdf_table_amd.tsr_stage import lore_geometry
    minv, _ = lore_geometry(ph, pw, inp_h, inp_w)
    tb = np.zeros(n, dtype=TSR_TABLE_DTYPE)
    tb["minv"], tb["page"], tb["crop_w"], tb["crop_h"] = minv.reshape(1, 6), np.arange(n), pw, ph
    return tb


def _words(t):
    return t.cpu().view(torch.int16).numpy()


@pytest.mark.parametrize("page_hw", [(90, 130), (130, 90)])
@pytest.mark.parametrize("inp", [(64, 96), (128, 128)])
@pytest.mark.parametrize("bgr", [True, False])
def test_preprocess_matches_warp_restatement(eng, page_hw, inp, bgr):
    """B = 3 pages; stored 16-bit words compared, as the Lore pre-process test does; pt_tsr_preprocess on the same inputs is unchanged"""
    from oracle import lore_pre
    ph, pw = page_hw
    inp_h, inp_w = inp
    rng = np.random.default_rng(ph * 1000 + inp_h + int(bgr))
    pages = rng.integers(0, 256, (3, ph, pw, 3), dtype=np.uint8)
    tb = _tables(3, ph, pw, inp_h, inp_w)
    d_pages = torch.from_numpy(pages).cuda()
    lore_before = _words(eng.tsr_preprocess(d_pages, tb, inp_h, inp_w, bgr=bgr))
    got = eng.docx_preprocess(d_pages, tb, inp_h, inp_w, bgr=bgr, mean=DOCX_MEAN, std=DOCX_STD)
    torch.cuda.synchronize()
    assert got.shape == (3, inp_h, inp_w, 4) and got.dtype == torch.bfloat16
    trans, _ = lore_pre.lore_preprocess_geometry(ph, pw, inp_h, inp_w, False)
    mean = np.array(DOCX_MEAN, np.float32).reshape(1, 1, 3)
    std = np.array(DOCX_STD, np.float32).reshape(1, 1, 3)
    for i in range(3):
        img = np.ascontiguousarray(pages[i][:, :, ::-1]) if bgr else pages[i]
        warped = lore_pre.warp_affine_u8(img, trans, inp_w, inp_h)
        ref = ((warped / 255. - mean) / std).astype(np.float32)
        want = torch.zeros(inp_h, inp_w, 4)
        want[..., :3] = torch.from_numpy(ref)
        assert np.array_equal(_words(got[i]), _words(want.to(torch.bfloat16))), (i, page_hw, inp, bgr)
    # the Lore pre-process shares the kernel and keeps its own table: same words before and after, and not the DocXLayout ones
    lore_after = _words(eng.tsr_preprocess(d_pages, tb, inp_h, inp_w, bgr=bgr))
    assert np.array_equal(lore_before, lore_after)
    x_ref, _ = lore_pre.lore_preprocess(np.ascontiguousarray(pages[0][:, :, ::-1]) if bgr else pages[0], inp_h, inp_w)
    want = torch.zeros(inp_h, inp_w, 4)
    want[..., :3] = x_ref[0].permute(1, 2, 0)
    assert np.array_equal(lore_after[0], _words(want.to(torch.bfloat16)))
    assert not np.array_equal(lore_after, _words(got))


def test_preprocess_pair_mode_and_changed_constants(eng):
    """BF16X3: hi + lo reproduce the fp32 value to 2^-16 relative; other constants rebuild the table, the first ones come back bit for bit"""
    rng = np.random.default_rng(5)
    pages = torch.from_numpy(rng.integers(0, 256, (2, 70, 50, 3), dtype=np.uint8)).cuda()
    tb = _tables(2, 70, 50, 64, 64)
    first = _words(eng.docx_preprocess(pages, tb, 64, 64))
    other = _words(eng.docx_preprocess(pages, tb, 64, 64, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25)))
    assert not np.array_equal(first, other)
    assert np.array_equal(first, _words(eng.docx_preprocess(pages, tb, 64, 64)))
    eng.set_precision(L.PT_PRECISION_BF16X3)
    try:
        x8 = eng.docx_preprocess(pages, tb, 64, 64).float().cpu()
    finally:
        eng.set_precision(L.PT_PRECISION_BF16)
    assert x8.shape[-1] == 8 and np.array_equal(_words(x8[..., :4].to(torch.bfloat16)), first)
    full = (x8[..., :3] + x8[..., 4:7]).numpy()
    lut = ((np.arange(256)[None] / 255. - np.array(DOCX_MEAN, np.float32)[:, None]) / np.array(DOCX_STD, np.float32)[:, None]).astype(np.float32)
    # every value is an entry of the channel's table, up to the pair's 16 significant bits
    for c in range(3):
        d = np.abs(full[..., c][..., None] - lut[c][None, None, None]).min(-1)
        assert (d <= 2.0 ** -15 * np.abs(full[..., c]).clip(1e-3)).all(), c
