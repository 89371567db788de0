"""tools/fit_textline_head.py [out.json]: fits the `fc` layer (1280 -> 2) of the synthetic text-line orientation classifier so that it tells the
generator's text lines from their 180-degree copies (the text-line orientation vote of OcrTablePipeline, predict() and predict_stream(orientation_vote=True)).

A seeded random-init PP-LCNet (synth_weights.pplcnet_state_dict(seed=5, class_num=2): the pipeline's synthetic_seed 0 + 5) scores few lines above the
vote's 0.9, so every page would vote "not upright" and flip, and no test could show both outcomes.  This script keeps the seeded random backbone and
last_conv, computes with the CPU oracle (oracle/pplcnet.py, textline strides) the post-hardswish 1280-d features of the line crops of pages
PAGES of the generator -- upright and rotated by 180 degrees; the crops are the boxes of the DB oracle on each page (PP-OCR post-process) and the
generator's own line rectangles grown by a few pixels, cut with the oracle's cv2.warpPerspective and resized like the classifier's pre-processor --
and fits fc in closed form (ridge regression of the logit difference onto +-TARGET).

What it is and is not: a WORKLOAD DEVICE.  The generator draws glyphs symmetric in distribution under a 180-degree rotation, so the head memorises
the lines of these pages; it is not an orientation classifier.  Output: pdf_table_amd/data/pplcnet_synth_textline_head.json (text: the float32
half-vector w / 2 and bias c / 2 of the logit difference, written exactly; seed, class_num, pages); pplcnet_state_dict(..., textline_head=True)
overlays it as fc.weight = [w / 2, -w / 2], fc.bias = [c / 2, -c / 2].  Prints the training margins and the per-page votes
of the fp32 oracle."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import crnn as ocrnn                                       # noqa: E402
from oracle import db_net, db_post, db_pre, pil_resize                 # noqa: E402
from oracle import pplcnet as opl                                       # noqa: E402
from pdf_table_amd.synth_pages import make_page                        # noqa: E402
from pdf_table_amd.synth_weights import db_resnet18_state_dict, pplcnet_state_dict   # noqa: E402

SEED, NCLS = 5, 2
PAGES = (0, 1, 2, 3, 4, 5)
TARGET, RIDGE = 6.0, 1e-2
GROW = 4
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pdf_table_amd", "data", "pplcnet_synth_textline_head.json")


def page_quads(img, det_sd):
    """DB oracle boxes (PP-OCR post-process) and the generator-like line rectangles are both used: -> float [k, 8]"""
    chw, shape_list = db_pre.preprocess_db_pp(img)
    with torch.no_grad():
        prob = db_net.db_forward_fp32(det_sd, torch.from_numpy(np.ascontiguousarray(chw))[None])[0, 0].numpy()
    return db_post.db_postprocess(prob, shape_list, img.shape, 0.3, 0.6, 1.5, False, 1000).reshape(-1, 8).astype(np.float64)


def rect_quads(rects, size, flipped):
    r = np.asarray(rects, np.float64).reshape(-1, 4) + np.array([-GROW, -GROW, GROW, GROW])
    if flipped:
        r = np.stack([size - r[:, 2], size - r[:, 3], size - r[:, 0], size - r[:, 1]], 1)
    x1, y1, x2, y2 = r.T
    return np.stack([x1, y1, x2, y1, x2, y2, x1, y2], 1)


def line_inputs(img, quads):
    """the classifier's network input of every quad: crop (cv2.warpPerspective) -> Pillow resize 80x160 -> normalise, f32 [k, 3, 80, 160]"""
    xs = []
    for q in quads:
        crop = ocrnn.crop_image(img, ocrnn.order_point(q.reshape(4, 2)))
        if crop.size == 0:
            continue
        xs.append(pil_resize.pplcnet_preprocess(crop, 80, 160))
    return np.stack(xs).astype(np.float32) if xs else np.zeros((0, 3, 80, 160), np.float32)


def features(sd, x, chunk=64):
    """post-hardswish 1280-d features: the oracle's forward with fc replaced by the identity"""
    f_sd = dict(sd)
    f_sd["fc.weight"] = torch.eye(1280)
    f_sd["fc.bias"] = torch.zeros(1280)
    out = [opl.pplcnet_forward(f_sd, torch.from_numpy(x[i:i + chunk]), textline=True) for i in range(0, len(x), chunk)]
    return torch.cat(out).numpy().astype(np.float64) if out else np.zeros((0, 1280))


def oracle_votes(sd, img, quads):
    """per-page vote of OcrSystemTask.text_line_orientation with the fp32 oracle over the given quads"""
    x = line_inputs(img, quads)
    if not len(x):
        return False, 0, 0
    res = opl.topk_postprocess(opl.pplcnet_forward(sd, torch.from_numpy(x), textline=True).numpy(), "textline_orientation")
    up = sum(1 for r in res if r["scores"][0] > 0.9 and r["label_names"][0] == "0_degree")
    down = sum(1 for r in res if r["scores"][0] > 0.9 and r["label_names"][0] != "0_degree")
    return up > down, up, down


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = {k: torch.as_tensor(np.asarray(v)).float() for k, v in pplcnet_state_dict(seed=SEED, class_num=NCLS).items()}
    det_sd = db_resnet18_state_dict(seed=0, text_signal=True)
    feats, labels, per_page = [], [], []
    for i in PAGES:
        img, meta = make_page(i)
        for flipped in (False, True):
            im = np.ascontiguousarray(img[::-1, ::-1]) if flipped else img
            q = np.concatenate([page_quads(im, det_sd), rect_quads(meta["lines"], img.shape[0], flipped)], 0)
            f = features(sd, line_inputs(im, q))
            feats.append(f)
            labels.append(np.full(len(f), 1 if flipped else 0))
            per_page.append((i, flipped, im, q))
            print(f"page {i} {'flipped' if flipped else 'upright'}: {len(f)} lines", flush=True)
    F, y = np.concatenate(feats), np.concatenate(labels)
    t = np.where(y == 0, TARGET, -TARGET)
    mu = F.mean(0)
    Fc = F - mu
    lam = RIDGE * np.trace(Fc.T @ Fc) / Fc.shape[1]
    w = np.linalg.solve(Fc.T @ Fc + lam * np.eye(Fc.shape[1]), Fc.T @ (t - t.mean()))
    c = float(t.mean() - mu @ w)
    d = F @ w + c
    print(f"{len(F)} lines: sign correct {np.mean(np.sign(d) == np.sign(t)):.4f}, |margin| > ln 9 and correct {np.mean((d * np.sign(t)) > np.log(9)):.4f}, "
          f"margin quantiles {np.quantile(d * np.sign(t), [0.01, 0.1, 0.5]).round(2).tolist()}")
    # logit difference l0 - l1 = d: class 0 ("0_degree") gets +d/2, class 1 -d/2
    W = np.stack([w / 2, -w / 2]).astype(np.float32)
    b = np.array([c / 2, -c / 2], np.float32)
    # float32 -> float64 is exact and json writes a float64 that reads back to the same value: the file holds the float32 weights exactly
    doc = {"seed": SEED, "class_num": NCLS, "pages": list(PAGES),
           "note": "fc of pplcnet_state_dict(seed, class_num): weight = [half, -half], bias = [bias0, -bias0] (tools/fit_textline_head.py)",
           "bias0": float(b[0]), "half": [float(v) for v in W[0]]}
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    sd["fc.weight"], sd["fc.bias"] = torch.from_numpy(W), torch.from_numpy(b)
    for i, flipped, im, q in per_page:
        up, nu, nd = oracle_votes(sd, im, q)
        print(f"oracle vote page {i} {'flipped' if flipped else 'upright'}: upright={up} ({nu} up, {nd} down of {len(q)})")
    print("wrote", out)


if __name__ == "__main__":
    main()
