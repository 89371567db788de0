"""Fixtures of DocXLayout's layout detector, from the reference's own docx_layout modules (imported by path, run on CPU):

  docxlayout_dla34.npz   DLASeg('dla34', eight heads, down_ratio 4, head_conv 256) on seeded weights (synth_weights.docxlayout_dla34_state_dict,
                         loaded strict=True: the proof of the key names), float64 forward, heads stored float32, inputs 128 x 160 and 64 x 64
  docxlayout_post.npz    for the REF_CASES of tests/docxlayout_synth.py at both map sizes: the reference's per-branch ``dets`` (top-100 rows
                         of ctdet_4ps_decode with the arg-max columns) and the rows pnms keeps
  docxlayout_post.json   the final lists of DocXLayoutImagePostProcessor.post_process for the same cases

    python tests/golden/make_golden_docxlayout.py

cv2 and shapely are not installed: cv2.getAffineTransform is the float64 three-point solve oracle.lore_decode.get_affine_transform_3pt, and
``shapely.geometry.Polygon`` is a stand-in on the product's own ``quad_intersection_rate`` -- so the polygon overlap is NOT pinned by these
fixtures (README says so beside the claim).

Every case written is checked first (``check_margins``): the threshold tests, peak equality, the rank at the top-100 boundary, every NMS
score comparison, every arg-max, every .5 rounding of a final coordinate and every x.xx5 rounding of a final score must be decided by more
than 4 x the largest difference between torch's float32 sigmoid and a float64 sigmoid on the case's own logits.  A case that fails is a bug
in tests/docxlayout_synth.py (pick another seed there), never something for the tests to skip."""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden import REF_SRC, _pkg, ref_import, stub_env  # noqa: E402
from oracle.lore_decode import get_affine_transform_3pt  # noqa: E402


def docx_env():
    from pdf_table_amd.docxlayout_stage import quad_intersection_rate
    cv2 = types.ModuleType("cv2")
    cv2.getAffineTransform = lambda src, dst: get_affine_transform_3pt(np.asarray(src, np.float64), np.asarray(dst, np.float64))
    sys.modules["cv2"] = cv2

    class _Area:
        def __init__(self, area):
            self.area = area

    class Polygon:      # what pts_intersection_rate needs: .area and .intersection(other).area
        def __init__(self, pts):
            self.flat = [float(v) for p in pts for v in p]

        @property
        def area(self):
            p = np.asarray(self.flat, np.float64).reshape(-1, 2)
            return abs(0.5 * float(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])))

        def intersection(self, other):
            return _Area(quad_intersection_rate(self.flat, other.flat) * self.area)

    sg = types.ModuleType("shapely.geometry")
    sg.Polygon = Polygon
    sh = types.ModuleType("shapely")
    sh.geometry = sg
    sys.modules["shapely"], sys.modules["shapely.geometry"] = sh, sg
    stub_env()
    for sub in ("model", "model/docx_layout"):
        name = "pdftable." + sub.replace("/", ".")
        if name not in sys.modules:
            _pkg(name, os.path.join(REF_SRC, "pdftable", sub))
    cfg = ref_import("pdftable.model.docx_layout.configuration_docxlayout")
    sys.modules["pdftable.model.docx_layout"].DocXLayoutConfig = cfg.DocXLayoutConfig
    return cfg


def gen_docxlayout_dla34():
    from pdf_table_amd.synth_weights import DOCX_HEADS, docxlayout_dla34_state_dict
    docx_env()
    m = ref_import("pdftable.model.docx_layout.model_dla")
    model = m.DLASeg("dla34", dict(DOCX_HEADS), pretrained=False, down_ratio=4, head_conv=256).eval()
    sd = docxlayout_dla34_state_dict(seed=41)
    model.load_state_dict(sd, strict=True)
    model.double()
    rng = np.random.default_rng(141)
    out = {"seed": np.array(41)}
    for tag, (h, w) in {"a": (128, 160), "b": (64, 64)}.items():
        x = rng.standard_normal((1, 3, h, w)).astype(np.float32)
        with torch.no_grad():
            z = model(torch.from_numpy(x).double())[0]
        out[f"x_{tag}"] = x
        for k, v in z.items():
            out[f"{k}_{tag}"] = v.float().numpy()
    np.savez_compressed(os.path.join(HERE, "docxlayout_dla34.npz"), **out)
    print("docxlayout_dla34.npz", {k: v.shape for k, v in out.items()})


def sigmoid_bound(z) -> float:
    """4 x the largest |torch float32 sigmoid - float64 sigmoid| over the case's sigmoid inputs (the rule of tests/layout_decode_ref.py)"""
    worst = 0.0
    for k in ("hm", "hm_sub", "cls", "ftype"):
        x = torch.from_numpy(np.ascontiguousarray(z[k]))
        worst = max(worst, float((torch.sigmoid(x).double() - torch.sigmoid(x.double())).abs().max()))
    return 4.0 * worst


def check_margins(name, size, z, finals) -> float:
    """the condition of the module docstring, on one case; returns the bound"""
    import docxlayout_ref as R
    bound = sigmoid_bound(z)
    for b, (hm, cls, ft) in enumerate(((z["hm"][0], z["cls"][0], z["ftype"][0]), (z["hm_sub"][0], None, None))):
        sig = R.sigmoid32(hm).astype(np.float64)
        c, h, w = sig.shape
        pad = np.pad(sig, ((0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
        nb = np.stack([pad[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1)])
        cand = sig >= 0.299 - bound
        # threshold tests (0.3 and the device's 0.3 - 1e-3), peak equality: a candidate differs from each neighbour by more than the bound
        assert not (np.abs(sig[cand] - 0.3) <= bound).any() and not (np.abs(sig[cand] - float(R.THR_LO)) <= bound).any(), (name, size, "threshold")
        assert not (np.abs(nb[:, cand] - sig[cand][None]) <= bound).any(), (name, size, "peak equality")
        peaks = np.sort(np.where((nb < sig[None]).all(0) & cand, sig, 0.0).reshape(-1))[::-1]
        peaks = peaks[peaks > 0]
        # ranks: all listed scores distinct by more than the bound (covers the top-100 boundary and every NMS score comparison)
        assert not (np.abs(np.diff(peaks)) <= bound).any(), (name, size, "rank")
        if cls is not None:
            for t in (cls, ft):
                s2 = np.sort(R.sigmoid32(t).astype(np.float64), 0)
                at = cand.any(0)      # the pixels a listed row can sit on
                assert not ((s2[-1] - s2[-2])[at] <= bound).any(), (name, size, "arg-max")
    for it in finals:
        frac = np.abs(np.asarray(it["raw_pts"], np.float64) % 1.0 - 0.5)
        assert (frac > 1e-3).all(), (name, size, "coordinate .5")
        assert abs((it["raw_score"] * 1000.0) % 10.0 - 5.0) > 1000.0 * bound, (name, size, "score x.xx5")
    return bound


def gen_docxlayout_post():
    import docxlayout_synth as S
    cfgm = docx_env()
    pu = ref_import("pdftable.model.docx_layout.processor_utils")
    ip = ref_import("pdftable.model.docx_layout.image_processing_docxlayout")
    cfg = cfgm.DocXLayoutConfig()
    post = ip.DocXLayoutImagePostProcessor(cfg)
    npz, js = {}, {}
    for size in S.SIZES:
        for name in S.REF_CASES:
            z = S.make_case(name, size)
            ph, pw = S.page_hw(size)
            meta = {"c": np.array([pw / 2.0, ph / 2.0], dtype=np.float32), "s": max(ph, pw) * 1.0, "out_height": size[0], "out_width": size[1]}
            outputs = {k: torch.from_numpy(v.copy()) for k, v in z.items()}
            _, dets, dets_sub, _, _ = post.post_process_model(outputs={k: v.clone() for k, v in outputs.items()})
            tag = f"{name}_{size[0]}x{size[1]}"
            for b, d in (("main", dets), ("sub", dets_sub)):
                npz[f"dets_{b}_{tag}"] = d[0].astype(np.float32)
                kept = pu.pnms(d[0], cfg.scores_thresh)
                npz[f"kept_{b}_{tag}"] = np.asarray(kept, np.float64).reshape(-1, 12).astype(np.float32)
            # the raw (unrounded) final rows for the margin check: post_process_bbox + merge_outputs, as post_process runs them
            d2, _ = post.post_process_bbox(dets.copy(), dets_sub.copy(), 0, meta)
            merged = post.merge_outputs([d2])
            raw = [{"raw_pts": box[:8].tolist(), "raw_score": float(box[8])} for j in merged for box in merged[j] if not box[8] < cfg.scores_thresh]
            bound = check_margins(name, size, z, raw)
            res = post.post_process({k: v.clone() for k, v in outputs.items()}, meta)
            js[tag] = [{"bbox": [float(v) for v in it["bbox"]], "label": it["label"], "score": float(it["score"]), "category_id": int(it["category_id"])}
                       for it in res]
            print(tag, "rows >= 0.3:", int((dets[0][:, 8] >= 0.3).sum()), int((dets_sub[0][:, 8] >= 0.3).sum()), "kept:",
                  len(npz[f"kept_main_{tag}"]), len(npz[f"kept_sub_{tag}"]), "final:", len(res), f"bound {bound:.2e}")
    np.savez_compressed(os.path.join(HERE, "docxlayout_post.npz"), **npz)
    with open(os.path.join(HERE, "docxlayout_post.json"), "w") as f:
        json.dump(js, f, indent=0)


if __name__ == "__main__":
    gen_docxlayout_dla34()
    gen_docxlayout_post()
