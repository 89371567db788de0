"""The SLANet door on the GPU: OcrTableStructureTask(model="SLANet", task_path=<dir with model.onnx and the dictionaries>) -- pt_slanet_preprocess,
the graph's feed-forward prefix on the generic executor, the Loop head as one pt_op_sla_decode launch, TableLabelDecode on the host.

The graph is the stand-in of tools/onnx_export_slanet.py (``SlaNetLike``: still a stand-in -- the shipped PaddleOCR files are not available offline) at a
reduced input (crops of 96 x 128 pixels, network input 128 x 128, T = 24) plus one case at the product's 488 x 488 with T = 501.

Reference: the same torch module on the CPU in fp32 on the pre-processing restatement of tests/slanet_ref.py, decoded by the TableLabelDecode that
tests/test_slanet_host.py pins to the reference's.  precision="fp32" (the engine's (hi | lo) pair mode): the token list must be identical and the polygons
within a bound that is measured, not chosen: the module's activations and weights are rounded to the pair format (two bf16 values, 16 significant
bits) after every leaf layer of the feed-forward part -- the arithmetic the executor computes in -- and compared with the float64 module on the same
inputs; the door gets 4 x that figure (in box units, times the crop's side).  The same run gives the logit error the margin pre-condition uses: every
walked step's top-two margin of the REFERENCE exceeds 4 x it, no step left out."""
import copy
import os
import shutil
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slanet_ref as R  # noqa: E402
from pdf_table_amd.rec_postprocess import TableLabelDecode, slanet_shape_result  # noqa: E402

pytestmark = pytest.mark.gpu

DICTS = os.path.join(REPO, "tests", "golden", "slanet")
SEED, CELL_BIAS = 2, 9.0


def crops(n, h, w, seed):
    """seeded table-like crops: a light ground with darker ruled lines and blocks"""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        img = np.full((h, w, 3), 235, np.uint8) - g.integers(0, 20, (h, w, 3), dtype=np.uint8)
        for y in g.choice(np.arange(4, h - 4), 4, replace=False):
            img[y:y + 2] = g.integers(0, 80, 3, dtype=np.uint8)
        for x in g.choice(np.arange(4, w - 4), 4, replace=False):
            img[:, x:x + 2] = g.integers(0, 80, 3, dtype=np.uint8)
        for _ in range(6):
            y, x = int(g.integers(0, h - 10)), int(g.integers(0, w - 16))
            img[y:y + 8, x:x + 14] = g.integers(0, 255, 3, dtype=np.uint8)
        out.append(img)
    return out


def pair_round(t):
    hi = t.to(torch.bfloat16).to(t.dtype)
    return hi + (t - hi).to(torch.bfloat16).to(t.dtype)


def pair_model(net):
    """the module in the executor's pair arithmetic: parameters and every leaf layer's output rounded to two bf16 values"""
    m = copy.deepcopy(net).float()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(pair_round(p))
    feat = [m.stem, m.s4, m.s8, m.s16, m.s32, m.lat, m.down8, m.down16, m.bu16, m.bu32]
    for part in feat:
        for leaf in part.modules():
            if not list(leaf.children()):
                leaf.register_forward_hook(lambda _m, _i, out: pair_round(out))
    return m


class Case:
    def __init__(self, tmp, size, steps, n, crop_hw):
        from onnx_export_slanet import SlaNetLike, export_slanet, seeded_slanet
        self.size, self.steps = size, steps
        self.dir = str(tmp)
        for name in ("table_structure_dict.txt", "table_structure_dict_ch.txt"):
            shutil.copy(os.path.join(DICTS, name), self.dir)
        self.decode = TableLabelDecode(os.path.join(DICTS, "table_structure_dict.txt"), merge_no_span_structure=True)
        cells = (self.decode.dict["<td"], self.decode.dict["<td></td>"])
        self.net = seeded_slanet(SlaNetLike(n_cls=30, n_loc=4, steps=steps), SEED, cell_ids=cells, cell_bias=CELL_BIAS)
        with open(os.path.join(self.dir, "model.onnx"), "wb") as f:
            f.write(export_slanet(self.net, size))
        self.images = crops(n, crop_hw[0], crop_hw[1], 11)
        pre = [R.slanet_preprocess(im, size) for im in self.images]
        self.x = torch.from_numpy(np.stack([p[0] for p in pre]))
        self.shapes = np.stack([p[1] for p in pre])
        with torch.no_grad():
            self.loc32, self.probs32, self.logits32 = self.net.walk(self.net.features(self.x))
            d = copy.deepcopy(self.net).double()
            loc64, _, logits64 = d.walk(d.features(self.x.double()))
            pm = pair_model(self.net)
            locp, _, logitsp = pm.walk(pm.features(self.x))
        ids = self.probs32.argmax(-1).numpy()
        eos = self.decode.end_idx
        self.walked = np.array([next((t + 1 for t in range(1, steps) if ids[b, t] == eos), steps) for b in range(n)])
        mask = np.arange(steps)[None, :] < self.walked[:, None]
        self.loc_yard = float((locp.double() - loc64).abs().numpy()[mask].max())
        self.logit_yard = float((logitsp.double() - logits64).abs().numpy()[mask].max())
        self.margin = float(R.top2_margin(self.logits32.numpy())[mask].min())
        res = self.decode({"structure_probs": self.probs32.numpy(), "loc_preds": self.loc32.numpy().copy()}, [self.shapes])
        self.want = [slanet_shape_result(res["structure_batch_list"][b][0], res["bbox_batch_list"][b]) for b in range(n)]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("slanet_small"), 128, 24, 3, (96, 128))


def task_for(case, precision, engine=None):
    from pdf_table_amd.ocr_table_structure_task import OcrTableStructureTask
    kw = {"engine": engine} if engine is not None else {}
    return OcrTableStructureTask(model="SLANet", task_path=case.dir, lang="en", precision=precision, table_max_len=case.size, **kw)


def check_against_reference(case, out):
    print(f"slanet door size {case.size} T {case.steps}: walked {case.walked.tolist()}, smallest top-two margin {case.margin:.3e}, pair-arithmetic logit "
          f"error {case.logit_yard:.3e}, box error {case.loc_yard:.3e}")
    assert case.margin > 4.0 * case.logit_yard, (case.margin, case.logit_yard)              # the pre-condition, on the reference alone
    assert (case.walked < case.steps).any()                                                  # the seeded head does end its walks
    for b, (got, want) in enumerate(zip(out, case.want)):
        assert got["structure_str_list"] == want["structure_str_list"], b
        assert got["structure_str_list"][:3] == ["<html>", "<body>", "<table>"] and len(got["structure_str_list"]) > 6
        h, w = case.images[b].shape[:2]
        gp, wp = np.asarray(got["polygons"], np.float64), np.asarray(want["polygons"], np.float64)
        assert gp.shape == wp.shape and (len(wp) == 0 or wp.shape[1] == 8)
        if len(wp):
            err = float(np.abs(gp - wp).max())
            bound = 4.0 * case.loc_yard * max(h, w)
            print(f"  table {b}: {len(wp)} cells, polygon error {err:.3e} pixels, bound {bound:.3e}")
            assert err <= bound, (b, err, bound)


def test_task_door_fp32_matches_the_module(small):
    task = task_for(small, "fp32")
    out = task(list(small.images))
    assert len(out) == 3 and all(set(r) == {"polygons", "structure_str_list", "inputs"} for r in out)
    assert out[0]["inputs"] is small.images[0]
    check_against_reference(small, out)
    again = task(small.images[1])                                                             # the replayed graph gives the eager walk's result
    assert again[0]["structure_str_list"] == out[1]["structure_str_list"] and np.array_equal(again[0]["polygons"], out[1]["polygons"])


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_task_door_16bit_is_well_formed(small, precision):
    out = task_for(small, precision)(list(small.images))
    for r in out:
        toks = r["structure_str_list"]
        assert toks[:3] == ["<html>", "<body>", "<table>"] and toks[-3:] == ["</table>", "</body>", "</html>"]
        ncell = sum(1 for t in toks if t in ("<td>", "<td", "<td></td>"))
        assert len(r["polygons"]) == ncell and (ncell == 0 or np.asarray(r["polygons"]).shape == (ncell, 8))
        assert np.isfinite(np.asarray(r["polygons"], np.float64)).all()


def test_lang_falls_back_to_en(small):
    from pdf_table_amd.ocr_table_structure_task import OcrTableStructureTask
    t = OcrTableStructureTask(model="SLANet", task_path=small.dir, lang="fr", precision="fp32", table_max_len=small.size)
    assert t.lang == "en" and len(t._sla_decode.character) == 30


def test_recognize_tables_shifts_to_the_page_frame(small):
    """two resident pages, three boxes: the task door's results per crop, shifted by the crop's corner"""
    task = task_for(small, "fp32")
    pages = np.full((2, 160, 200, 3), 255, np.uint8)
    boxes = [np.array([[10, 20, 138, 116], [60, 50, 188, 146]]), np.array([[0, 0, 128, 96]])]
    k = 0
    for p, bs in enumerate(boxes):
        for (x1, y1, x2, y2) in bs:
            pages[p, y1:y2, x1:x2] = small.images[k][:y2 - y1, :x2 - x1]
            k += 1
    single = [task(np.ascontiguousarray(pages[p, y1:y2, x1:x2]))[0] for p, bs in enumerate(boxes) for (x1, y1, x2, y2) in bs]
    res = task.recognize_tables(torch.from_numpy(pages).cuda(), boxes)
    assert [len(r) for r in res] == [2, 1]
    flat = [r for page in res for r in page]
    corners = [(b[0], b[1]) for bs in boxes for b in bs]
    for got, one, (x0, y0) in zip(flat, single, corners):
        assert got["structure_str_list"] == one["structure_str_list"]
        if len(one["polygons"]):
            want = np.asarray(one["polygons"]) + np.tile(np.array([x0, y0], np.float32), 4)[None]
            assert np.allclose(np.asarray(got["polygons"]), want, rtol=0, atol=1e-3)
    unshifted = task.recognize_tables(torch.from_numpy(pages).cuda(), boxes, page_frame=False)
    for got, one in zip([r for page in unshifted for r in page], single):
        assert np.array_equal(np.asarray(got["polygons"]), np.asarray(one["polygons"]))


def test_full_size_501_steps(tmp_path_factory):
    """the product's geometry: 488 x 488 input, 16 x 16 = 256 tokens at the 1/32 level, T = 501"""
    case = Case(tmp_path_factory.mktemp("slanet_full"), 488, 501, 2, (300, 488))
    out = task_for(case, "fp32")(list(case.images))
    check_against_reference(case, out)


def test_pipeline_constructor_refuses_slanet():
    from pdf_table_amd.pipeline import OcrTablePipeline
    with pytest.raises(ValueError, match="out of scope"):
        OcrTablePipeline(table_structure=True, table_structure_model="SLANet", synthetic_seed=0)
