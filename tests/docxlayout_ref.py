"""CPU restatement of DocXLayout for the tests: the network (DLASeg with dla34, DLAUp and eight heads, docx_layout/model_dla.py:448-652) in
torch on oracle.lore_net's DLA-34 base, the decode of one branch (ctdet_4ps_decode + pnms, processor_utils.py:22-158) with the engine's
tie rule, and the host chain (DocXLayoutImagePostProcessor.post_process, image_processing_docxlayout.py:223-459) in numpy, written out
step by step, loops where the reference loops.  Pinned against the reference itself by tests/golden/docxlayout_dla34.npz and
docxlayout_post.npz / .json (test_docxlayout_host.py).  The polygon overlap is the product's (the reference's needs shapely, which is
not installed; the golden generator injects the same function)."""
from __future__ import annotations

import math
from functools import cmp_to_key
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from centernet_ref import _ida
from oracle.lore_net import dla34_forward
from pdf_table_amd.centernet_stage import centernet_decode_affine
from pdf_table_amd.docxlayout_stage import DOCX_LABELS, quad_intersection_rate

HEADS = {"cls": 4, "ftype": 3, "hm": 11, "hm_sub": 2, "reg": 2, "reg_sub": 2, "wh": 8, "wh_sub": 8}
K, THRESH, NUM_CLASSES = 100, 0.3, 13
THR_LO = np.float32(0.3 - 1e-3)


def docx_forward(sd: Dict[str, torch.Tensor], x: torch.Tensor) -> Dict[str, torch.Tensor]:
    """x NCHW (already normalised) -> the eight head maps NCHW at a quarter of the input size (pre-sigmoid); computes in x's dtype"""
    sd = {k: (v.to(x.dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    layers = dla34_forward(sd, x)[2:]
    width = [64, 128, 256, 512]
    for i in range(3):
        layers[-i - 1:] = _ida(sd, f"dla_up.ida_{i}", layers[-i - 2:], width[-i - 2])
    feat = layers[-1]
    return {h: F.conv2d(F.relu(F.conv2d(feat, sd[f"{h}.0.weight"], sd[f"{h}.0.bias"], padding=1)), sd[f"{h}.2.weight"], sd[f"{h}.2.bias"])
            for h in HEADS}


def sigmoid32(x: np.ndarray) -> np.ndarray:
    """torch's float32 sigmoid on the CPU (what the reference's ``.sigmoid_()`` computes)"""
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def branch_list(hm: np.ndarray, wh: np.ndarray, reg: np.ndarray, cls: np.ndarray = None, ftype: np.ndarray = None, k: int = K,
                thr_lo=THR_LO) -> Tuple[np.ndarray, np.ndarray]:
    """one page, one branch: hm [C, h, w] logits, wh [8, h, w], reg [2, h, w] (cls [4, h, w], ftype [3, h, w]: main branch) -> (records
    float32 [m, 12], flat indices int64 [m]): the first k peaks with sigmoid >= thr_lo by (score descending, class * h * w + pixel
    ascending), as pt_docx_decode lists them"""
    sig = sigmoid32(hm)
    c, h, w = sig.shape
    pooled = F.max_pool2d(torch.from_numpy(sig)[None], 3, stride=1, padding=1)[0].numpy()
    flat = np.where(pooled == sig, sig, np.float32(0)).reshape(-1)
    cand = np.nonzero(flat >= thr_lo)[0]
    cand = cand[np.lexsort((cand, -flat[cand].astype(np.float64)))][:k]
    pix = cand % (h * w)
    ys, xs = pix // w, pix % w
    px = xs.astype(np.float32) + reg[0, ys, xs].astype(np.float32)
    py = ys.astype(np.float32) + reg[1, ys, xs].astype(np.float32)
    rec = np.zeros((len(cand), 12), np.float32)
    for i in range(4):
        rec[:, 2 * i] = px - wh[2 * i, ys, xs].astype(np.float32)
        rec[:, 2 * i + 1] = py - wh[2 * i + 1, ys, xs].astype(np.float32)
    rec[:, 8] = flat[cand]
    rec[:, 9] = (cand // (h * w)).astype(np.float32)
    if cls is not None:
        rec[:, 10] = np.argmax(sigmoid32(cls)[:, ys, xs], 0)
        rec[:, 11] = np.argmax(sigmoid32(ftype)[:, ys, xs], 0)
    return rec, cand


def pnms_keep(rec: np.ndarray, thresh: float = THRESH) -> np.ndarray:
    """the rows pnms keeps, as flags, with its loop: float64 on the float32 rows"""
    d = rec.astype(np.float64)
    keep = np.zeros(len(d), bool)
    for i in range(len(d)):
        if d[i, 8] < thresh:
            continue
        cx = (d[i, 0] + d[i, 2] + d[i, 4] + d[i, 6]) / 4
        cy = (d[i, 1] + d[i, 3] + d[i, 5] + d[i, 7]) / 4
        state = -1
        for j in range(len(d)):
            if i == j or d[j, 8] < thresh:
                continue
            q = d[j, :8].reshape(4, 2)
            cr = [(q[(e + 1) % 4, 0] - q[e, 0]) * (cy - q[e, 1]) - (q[(e + 1) % 4, 1] - q[e, 1]) * (cx - q[e, 0]) for e in range(4)]
            if all(v > 0 for v in cr) or all(v < 0 for v in cr):
                if d[i, 8] > d[j, 8] and state < 0:
                    state = i
                elif d[i, 8] < d[j, 8]:
                    state = -2
                    break
        keep[i] = state != -2
    return keep


def _angle(pts_list):
    wide, rest = [], []
    for p in pts_list:
        a = math.atan2(p[3] - p[1], p[2] - p[0])
        if math.sqrt((p[2] - p[0]) ** 2 + (p[3] - p[1]) ** 2) > math.sqrt((p[4] - p[2]) ** 2 + (p[5] - p[3]) ** 2) * 3:
            wide.append(a)
        else:
            rest.append(a)
    for lst in (wide, rest):
        if lst:
            lst.sort()
            return lst[len(lst) // 2]
    return 0


def _axis(a_lo, a_len, b_lo, b_len):
    a_hi, b_hi = a_lo + a_len, b_lo + b_len
    first = (a_lo < b_lo) - (a_lo > b_lo)
    last = (a_hi > b_hi) - (a_hi < b_hi)
    if a_hi < b_lo + 1e-4 and a_hi < b_hi - 1e-4:
        return 1
    if a_lo > b_hi - 1e-4 and a_lo > b_lo + 1e-4:
        return 2
    if first == 1 and last == -1:
        return 3
    if first == -1 and last == 1:
        return 4
    if first >= 0 and last >= 0:
        return 5
    if first <= 0 and last <= 0:
        return 6
    return 0


def sort_pts(blocks: List[Dict]) -> None:
    """the reference's sort: rectangles recomputed inside every comparison, as there"""
    ang = _angle([b["pts"] for b in blocks])
    sn, cs = math.sin(ang), math.cos(ang)

    def rect(pts):
        xs = [pts[i] * cs + pts[i + 1] * sn for i in range(0, len(pts), 2)]
        ys = [pts[i + 1] * cs - pts[i] * sn for i in range(0, len(pts), 2)]
        return [min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)]

    def cmp(a, b):
        ra, rb = rect(a["pts"]), rect(b["pts"])
        ax0, ay0, ax1, ay1 = ra[0], ra[1], ra[0] + ra[2], ra[1] + ra[3]
        bx0, by0, bx1, by1 = rb[0], rb[1], rb[0] + rb[2], rb[1] + rb[3]
        xt, yt = _axis(ra[0], ra[2], rb[0], rb[2]), _axis(ra[1], ra[3], rb[1], rb[3])
        near = 0.0
        if yt == 3:
            near = (ay1 - by0) / min(ay1 - ay0, by1 - by0)
        elif yt == 4:
            near = (by1 - ay0) / min(ay1 - ay0, by1 - by0)
        if yt == 1:
            return -1
        if yt == 2:
            return 1
        if yt == 3:
            if xt in (2, 4):
                return -1 if near < 0.5 else 1
            return -1
        if yt == 4:
            if xt in (1, 3):
                return 1 if near < 0.5 else -1
            return 1
        if xt in (1, 3):
            return -1
        if xt in (2, 4):
            return 1
        if abs(0.5 * (ay0 + ay1) - 0.5 * (by0 + by1)) / max(ay1 - ay0, by1 - by0) < 0.1:
            return (ax0 + ax1 > bx0 + bx1) - (ax0 + ax1 < bx0 + bx1)
        return (ay0 + ay1 > by0 + by1) - (ay0 + ay1 < by0 + by1)

    blocks.sort(key=cmp_to_key(cmp))


def page_result(main: np.ndarray, sub: np.ndarray, page_hw, map_hw) -> List[Dict]:
    """records of the two branches behind pnms (float32 [m, 12], the sub branch's classes still 0-based) -> the final list"""
    inv = centernet_decode_affine(page_hw[0], page_hw[1], map_hw[0], map_hw[1])
    per = []
    for rows, shift in ((main, 0), (sub, 11)):
        d = np.asarray(rows, np.float32).reshape(-1, 12).astype(np.float64)
        d[:, 9] += shift
        for p in range(len(d)):
            for v in range(4):
                pt = np.array([d[p, 2 * v], d[p, 2 * v + 1], 1.0], dtype=np.float32)
                d[p, 2 * v:2 * v + 2] = np.dot(inv, pt)[:2]
        cls_rows = {}
        for j in range(NUM_CLASSES):
            r = d[d[:, 9] == j].astype(np.float32).reshape(-1, 12)
            r = np.array([b for b in r if b[8] > THRESH], dtype=np.float32).reshape(-1, 12)
            cls_rows[j + 1] = r if len(r) else np.zeros((1, 12), np.float32)
        per.append(cls_rows)
    dets = per[0]
    dets[12], dets[13] = per[1][12], per[1][13]
    scores = np.hstack([dets[j][:, 8] for j in range(1, NUM_CLASSES + 1)])
    if len(scores) > K:
        kth = len(scores) - K
        cut = np.partition(scores, kth)[kth]
        for j in dets:
            dets[j] = dets[j][dets[j][:, 8] >= cut]
    lay, subs = [], []
    for j in range(1, NUM_CLASSES + 1):
        for box in dets[j]:
            if box[8] < THRESH:
                continue
            it = {"category": DOCX_LABELS[int(box[9])], "pts": np.round(box).tolist()[:8], "confidence": float("{:.2f}".format(box[8]))}
            (subs if j in (12, 13) else lay).append(it)
    fields = [dict(s, layouts=[]) for s in subs]
    sort_pts(fields)
    if fields:
        other = {"category": "other", "pts": [0] * 8, "confidence": 0, "layouts": []}
        for it in lay:
            best, idx = 0.0, -1
            for k_, f in enumerate(fields):
                r = quad_intersection_rate(it["pts"], f["pts"])
                if r > best:
                    best, idx = r, k_
            if idx >= 0 and best > 0.1:
                fields[idx]["layouts"].append(it)
            else:
                other["layouts"].append(it)
        if other["layouts"]:
            fields.append(other)
    else:
        fields = [{"category": "other", "pts": [0] * 8, "confidence": 0, "layouts": list(lay)}]
    for f in fields:
        sort_pts(f["layouts"])
    blocks = []
    for f in fields:
        if f["category"] != "other":
            blocks.append(f)
        else:
            blocks += [dict(it, layouts=[it]) for it in f["layouts"]]
    sort_pts(blocks)
    out = []
    for b in blocks:
        for it in b["layouts"]:
            out.append({"bbox": np.array([it["pts"][0], it["pts"][1], it["pts"][4], it["pts"][5]]), "label": it["category"],
                        "score": it["confidence"], "category_id": DOCX_LABELS.index(it["category"])})
    return out


def page_chain(heads: Dict[str, np.ndarray], page_hw, i: int = 0) -> List[Dict]:
    """head maps NCHW (one batch entry) -> the final list: both branch lists, pnms, the host chain"""
    m, _ = branch_list(heads["hm"][i], heads["wh"][i], heads["reg"][i], heads["cls"][i], heads["ftype"][i])
    s, _ = branch_list(heads["hm_sub"][i], heads["wh_sub"][i], heads["reg_sub"][i])
    return page_result(m[pnms_keep(m)], s[pnms_keep(s)], page_hw, heads["hm"].shape[2:])


# ---- which decisions of the chain a small error in the head maps could turn -----------------------------------------------------------------
# The engine's BF16X3 mode stores every activation as a bf16 pair: 16 significant bits, a relative rounding of at most 2^-17 per stored map.
# The longest path through the net has 44 stored maps (the input, 34 base layers, the up-path's projections, up-samplers and nodes, the head's
# hidden map).  The roundings are independent and of either sign, so they add in quadrature: sqrt(44) x 2^-17 = 5e-5 of a head's largest value is
# the size to expect (fp32 accumulation differences are smaller still), and REL is four times that, 2e-4 -- a fifth of the 1e-3 the net tests
# allow.  chain_margins() names the first decision of the chain that a perturbation of that size could turn; a page on which it returns None
# gives the same final list for every set of head maps within REL of the restatement's.
REL = 4.0 * math.sqrt(44.0) * 2.0 ** -17


def chain_margins(heads: Dict[str, np.ndarray], page_hw, i: int = 0, rel: float = REL, score_bound: float = None):
    """None, or the name of the first decision not settled by more than rel * max(1, max|head|) on this page.  score_bound: the golden
    generator's rule instead -- the head maps are taken as given and only the sigmoid may differ, by score_bound (a logit margin of four
    times that: the sigmoid's slope is at most 1/4)"""
    d = {k: rel * max(1.0, float(np.abs(v[i]).max())) for k, v in heads.items()}
    if score_bound is not None:
        d = {k: (4.0 * score_bound if k.startswith("hm") else 0.0) for k in heads}
    h, w = heads["hm"].shape[2:]
    scale = float(np.abs(centernet_decode_affine(page_hw[0], page_hw[1], h, w)[:, :2]).max())
    t_hi = math.log(0.3 / 0.7)
    for hm_k, wh_k, reg_k in (("hm", "wh", "reg"), ("hm_sub", "wh_sub", "reg_sub")):
        x = heads[hm_k][i].astype(np.float64)
        dx, eps = d[hm_k], d[wh_k] + d[reg_k]
        ds = dx / 4.0                                                   # the sigmoid's slope is at most 1/4
        pad = np.pad(x, ((0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
        nb = np.stack([pad[:, a:a + h, b:b + w] for a in range(3) for b in range(3) if (a, b) != (1, 1)]).max(0)
        # only peaks that can reach 0.3 matter: one between the device's thr_lo and 0.3 is listed or not, and dropped downstream either way
        cand = x >= t_hi - dx
        sure_peak, sure_not = (x > nb + 2 * dx) & cand, (nb > x + 2 * dx) & cand
        if (cand & ~sure_peak & ~sure_not).any():
            return f"{hm_k}: a peak test within the margin"
        if (np.abs(x[sure_peak] - t_hi) <= dx).any():
            return f"{hm_k}: a peak's score within the margin of the threshold"
        if int(sure_peak.sum()) >= K:
            return f"{hm_k}: {int(sure_peak.sum())} peaks reach the top-{K} cut"
        rec, _ = branch_list(heads[hm_k][i], heads[wh_k][i], heads[reg_k][i])
        rec = rec[rec[:, 8].astype(np.float64) >= THRESH].astype(np.float64)
        for a in range(len(rec)):
            cx, cy = rec[a, 0:8:2].sum() / 4, rec[a, 1:8:2].sum() / 4
            for b in range(len(rec)):
                if a == b:
                    continue
                q = rec[b, :8].reshape(4, 2)
                cr, tol = [], []
                for e in range(4):
                    (x1, y1), (x2, y2) = q[e], q[(e + 1) % 4]
                    cr.append((x2 - x1) * (cy - y1) - (y2 - y1) * (cx - x1))
                    tol.append(4 * eps * (abs(cy - y1) + abs(x2 - x1) + abs(y2 - y1) + abs(cx - x1) + eps))
                clear = [abs(c) > t for c, t in zip(cr, tol)]
                if all(clear) and (all(c > 0 for c in cr) or all(c < 0 for c in cr)):
                    if abs(rec[a, 8] - rec[b, 8]) <= 2 * ds:
                        return f"{hm_k}: an NMS score comparison within the margin"
                elif not any(c1 and c2 and (u > 0) != (v > 0) for u, c1 in zip(cr, clear) for v, c2 in zip(cr, clear)):
                    return f"{hm_k}: a centre within the margin of a quad's edge"
        kept = rec[pnms_keep(rec.astype(np.float32))]
        inv = centernet_decode_affine(page_hw[0], page_hw[1], h, w)
        for r in kept:
            for v in range(4):
                p = inv @ np.array([r[2 * v], r[2 * v + 1], 1.0])
                if (np.abs(np.abs(p % 1.0) - 0.5) <= 2 * scale * eps).any():
                    return f"{hm_k}: a final coordinate within the margin of .5"
            if abs((r[8] * 1000.0) % 10.0 - 5.0) <= 1000.0 * ds:
                return f"{hm_k}: a final score within the margin of x.xx5"
    return None


def chain_headroom(heads: Dict[str, np.ndarray], page_hw, i: int = 0) -> float:
    """the largest rel (to a factor of 2) at which chain_margins() still passes on this page; 0 when it fails at 1e-8"""
    rel, last = 1e-8, 0.0
    while rel < 1e-1 and chain_margins(heads, page_hw, i, rel) is None:
        last, rel = rel, rel * 2.0
    return last
