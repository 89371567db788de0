"""References for the layout decode on the device (csrc/layout_decode.hip), shared by test_layout_decode_host.py and the GPU tests.

decode64()        LayoutStage.decode_page restated with EVERY step in float64 from the float32 record values: the yardstick both the host's
                  float32 soft-max and the device are measured against.  Equal scores are ordered by (level, anchor), the device's rule.
margins_ok()      walks that decode and says whether any of its decisions could flip within (d_box, d_score).
case builders     seeded; records as the candidate kernels write them (int32 level / anchor words, zero padding to 48 floats, shuffled arrival).
"""
import numpy as np

from pdf_table_amd.layout_stage import LayoutStage, PicodetConfig

REC = 48
CANDIDATE_SIZE = 200
TASK_OF_NCLS = {1: "table", 5: "en", 10: "ch"}


def make_cfg(ncls=5, strides=(8, 16, 32, 64), inp=(800, 608), score_threshold=0.5, nms_threshold=0.5, nms_top_k=1000, keep_top_k=100):
    cfg = PicodetConfig(task_type=TASK_OF_NCLS[ncls])
    cfg.strides, cfg.img_height, cfg.img_width = tuple(strides), inp[0], inp[1]
    cfg.score_threshold, cfg.nms_threshold, cfg.nms_top_k, cfg.keep_top_k = score_threshold, nms_threshold, nms_top_k, keep_top_k
    return cfg


def host_stage(cfg):
    """a LayoutStage for decode_page alone: no engine, no device (pt_hard_nms is host code of the library)"""
    st = LayoutStage.__new__(LayoutStage)
    st.config = cfg
    return st


def host_decode(case):
    return host_stage(case["cfg"]).decode_page(case["rec"].copy(), case["org"], probs=case["probs"])


def _iou64(b, c, eps=1e-5):
    w = max(min(b[2], c[2]) - max(b[0], c[0]), 0.0)
    h = max(min(b[3], c[3]) - max(b[1], c[1]), 0.0)
    inter = w * h
    ab = max(b[2] - b[0], 0.0) * max(b[3] - b[1], 0.0)
    ac = max(c[2] - c[0], 0.0) * max(c[3] - c[1], 0.0)
    return inter / (ab + ac - inter + eps)


def _walk64(rec, cfg, probs):
    """the float64 decode up to the picks -> (picks [(class, box[4], score, level, anchor)], decisions) ; decisions: what margins_ok() inspects"""
    ncls = len(cfg.labels)
    dec = {"scores": [], "cut": [], "class_scores": [], "iou": []}
    if len(rec) == 0:
        return [], dec
    rec = np.ascontiguousarray(rec, np.float32)
    level, anchor = rec[:, 0].view(np.int32).astype(np.int64), rec[:, 1].view(np.int32).astype(np.int64)
    x = rec[:, 2:2 + ncls].astype(np.float64)
    with np.errstate(over="ignore"):
        scores = x if probs else 1.0 / (1.0 + np.exp(-x))
    reg = rec[:, 2 + ncls:2 + ncls + 32].astype(np.float64).reshape(-1, 4, 8)
    e = np.exp(reg - reg.max(-1, keepdims=True))
    dist = ((e / e.sum(-1, keepdims=True)) * np.arange(8.0)).sum(-1)
    keep = np.zeros(len(rec), bool)
    boxes = np.zeros((len(rec), 4))
    smax = np.where(np.isnan(scores), -np.inf, scores).max(1)
    for l, stride in enumerate(cfg.strides):
        m = np.nonzero(level == l)[0]
        if not len(m):
            continue
        fm_w = -(-cfg.img_width // stride)
        cx, cy = (anchor[m] % fm_w + 0.5) * stride, (anchor[m] // fm_w + 0.5) * stride
        d = dist[m] * stride
        boxes[m] = np.stack([cx - d[:, 0], cy - d[:, 1], cx + d[:, 2], cy + d[:, 3]], 1)
        order = m[np.lexsort((anchor[m], -smax[m]))]
        if len(order) > cfg.nms_top_k:
            dec["cut"].append((smax[order[cfg.nms_top_k - 1]], smax[order[cfg.nms_top_k]]))
        keep[order[:cfg.nms_top_k]] = True
    thr = float(np.float32(cfg.score_threshold))
    dec["scores"] = scores[keep][~np.isnan(scores[keep])]
    picks = []
    for c in range(ncls):
        s = scores[:, c]
        idx = np.nonzero(keep & (s > thr))[0]
        if not len(idx):
            continue
        idx = idx[np.lexsort((anchor[idx], level[idx], -s[idx]))]
        dec["class_scores"].append(s[idx])
        idx = list(idx[:CANDIDATE_SIZE])
        n_pick = 0
        while idx:
            cur = idx.pop(0)
            picks.append((c, boxes[cur].copy(), s[cur], int(level[cur]), int(anchor[cur])))
            n_pick += 1
            if 0 < cfg.keep_top_k == n_pick:
                break
            rest = []
            for j in idx:
                dec["iou"].append((boxes[j], boxes[cur]))
                if _iou64(boxes[j], boxes[cur]) <= cfg.nms_threshold:
                    rest.append(j)
            idx = rest
    return picks, dec


def decode64(rec, cfg, org, probs):
    """decode_page in float64 -> [{"bbox", "label", "score", "category_id", "src": (level, anchor)}], in decode_page's order"""
    picks, _ = _walk64(rec, cfg, probs)
    oh, ow = float(org[0]), float(org[1])
    sf_h, sf_w = cfg.img_height / oh, cfg.img_width / ow
    out = []
    for c, b, s, l, a in picks:
        x0, x1 = sorted((b[0], b[2]))
        y0, y1 = sorted((b[1], b[3]))
        bb = np.array([np.clip(x0, 0, ow) / sf_w, np.clip(y0, 0, oh) / sf_h, np.clip(x1, 0, ow) / sf_w, np.clip(y1, 0, oh) / sf_h])
        out.append({"bbox": bb, "label": cfg.id2label[c], "score": float(s), "category_id": c, "src": (l, a)})
    return out


def margin_report(case, d_box, d_score):
    """how many decisions of the float64 decode could flip within the tolerances, by kind: a class score within d_score of the threshold, two
    candidate scores of one class within 2 d_score, a level's top-K cut between two best scores within 2 d_score, an IoU test whose interval
    -- both boxes grown, and both shrunk, by d_box -- contains the NMS threshold"""
    cfg = case["cfg"]
    _, dec = _walk64(case["rec"], cfg, case["probs"])
    thr = float(np.float32(cfg.score_threshold))
    rep = {"threshold": 0, "order": 0, "cut": 0, "iou": 0}
    if len(dec["scores"]):
        rep["threshold"] = int((np.abs(dec["scores"] - thr) <= d_score).sum())
    for s in dec["class_scores"]:
        if len(s) > 1:
            rep["order"] += int((np.abs(np.diff(s)) <= 2 * d_score).sum())      # sorted descending: neighbours are the closest pairs
    for hi, lo in dec["cut"]:
        rep["cut"] += int(abs(hi - lo) <= 2 * d_score)
    g = np.array([-d_box, -d_box, d_box, d_box])
    for b, c in dec["iou"]:
        v = [_iou64(b, c), _iou64(b + g, c + g), _iou64(b - g, c - g)]
        rep["iou"] += int(min(v) <= cfg.nms_threshold <= max(v))
    return rep


def margins_ok(case, d_box, d_score):
    """False if any decision counted by margin_report() could flip"""
    return not any(margin_report(case, d_box, d_score).values())


def host_vs_64(case):
    """(largest |box| difference, largest |score| difference, same picks?) of decode_page against decode64 on one case"""
    h, r = host_decode(case), decode64(case["rec"], case["cfg"], case["org"], case["probs"])
    same = len(h) == len(r) and all(a["category_id"] == b["category_id"] for a, b in zip(h, r))
    if not same or not h:
        return 0.0, 0.0, same
    d_box = max(float(np.abs(a["bbox"] - b["bbox"]).max()) for a, b in zip(h, r))
    d_score = max(abs(float(a["score"]) - b["score"]) for a, b in zip(h, r))
    same = same and d_box < 1e-2      # the same boxes, not merely the same classes
    return d_box, d_score, same


# ---- records ------------------------------------------------------------------------------------------------------------------------------------
def dfl_logits(v):
    """8 bin logits whose soft-max expectation is v (0 .. 7): the mass on the two bins around v"""
    lo = int(np.floor(min(max(v, 0.0), 7.0)))
    f = min(max(v, 0.0), 7.0) - lo
    x = np.full(8, -40.0)
    if f <= 0 or lo == 7:
        x[lo] = 0.0
    else:
        x[lo], x[lo + 1] = np.log(1 - f), np.log(f)
    return x


def record(ncls, level, anchor, cls_values, sides=None, dist_logits=None):
    """one 48-float record: cls_values [ncls] as stored (logits or probabilities); sides: 4 expected bins (l, t, r, b), or dist_logits [32]"""
    r = np.zeros(REC, np.float32)
    r[0:1] = np.array([level], np.int32).view(np.float32)
    r[1:2] = np.array([anchor], np.int32).view(np.float32)
    r[2:2 + ncls] = cls_values
    r[2 + ncls:2 + ncls + 32] = np.concatenate([dfl_logits(v) for v in sides]) if dist_logits is None else dist_logits
    return r


def _case(name, recs, cfg, org, probs, rng):
    rec = np.stack(recs).astype(np.float32) if len(recs) else np.zeros((0, REC), np.float32)
    if len(rec) > 1:
        rec = rec[rng.permutation(len(rec))]
    return {"name": name, "rec": rec, "cfg": cfg, "org": tuple(org), "probs": bool(probs)}


def _sigmoid32(x):
    import torch
    return torch.sigmoid(torch.from_numpy(np.asarray(x, np.float32))).numpy()


def random_case(name, seed, n, cfg, org, probs, level_counts=None, hot=0.6, region=12):
    """n records on distinct anchors of a small region of every level's map (so that boxes overlap), random peaked distributions, per record one or
    two classes that may pass the threshold.  level_counts: records per level (default: spread evenly)"""
    rng = np.random.default_rng(seed)
    ncls, nl = len(cfg.labels), len(cfg.strides)
    if level_counts is None:
        level_counts = [n // nl + (1 if l < n % nl else 0) for l in range(nl)]
    recs = []
    for l, k in enumerate(level_counts):
        stride = cfg.strides[l]
        fm_w, fm_h = -(-cfg.img_width // stride), -(-cfg.img_height // stride)
        rw, rh = min(fm_w, max(region, int(np.ceil(np.sqrt(k))) + 1)), min(fm_h, max(region, int(np.ceil(np.sqrt(k))) + 1))
        cells = rng.permutation(rw * rh)[:k]
        assert len(cells) == k, (name, l, k)
        for cell in cells:
            anchor = int(cell // rw) * fm_w + int(cell % rw)
            logits = rng.uniform(-5.0, -1.5, ncls)
            if rng.random() < hot:
                logits[rng.integers(ncls)] = rng.uniform(0.1, 4.0)
            if rng.random() < 0.25:
                logits[rng.integers(ncls)] = rng.uniform(0.1, 4.0)
            dl = rng.normal(0.0, 1.5, 32)
            dl[np.arange(4) * 8 + rng.integers(1, 7, 4)] += rng.uniform(2.0, 6.0, 4)
            recs.append(record(ncls, l, anchor, _sigmoid32(logits) if probs else logits, dist_logits=dl))
    return _case(name, recs, cfg, org, probs, rng)


def chain_case():
    """A suppresses B (iou 0.54), B would have suppressed C (0.54), A and C overlap by 0.25: C survives"""
    cfg = make_cfg(ncls=5, strides=(8, 16, 32))
    rng = np.random.default_rng(5)
    recs = []
    for col, p in ((10, 0.9), (13, 0.8), (16, 0.7)):
        cls = np.full(5, 0.01, np.float32)
        cls[2] = p
        recs.append(record(5, 0, 10 * 76 + col, cls, sides=(5, 5, 5, 5)))
    return _case("chain", recs, cfg, (800, 608), True, rng)


def zero_width_case():
    """all distribution mass in bin 0: boxes of no area, nothing suppresses anything"""
    cfg = make_cfg(ncls=5, strides=(8, 16, 32))
    rng = np.random.default_rng(6)
    recs = []
    for k in range(6):
        cls = np.full(5, 0.02, np.float32)
        cls[k % 2] = 0.6 + 0.05 * k
        recs.append(record(5, k % 3, 80 + (k // 3), cls, sides=(0, 0, 0, 0)))
    return _case("zero_width", recs, cfg, (800, 608), True, rng)


def clip_case():
    """boxes over all four page edges; a page smaller than, and shaped differently from, the network input"""
    cfg = make_cfg(ncls=5, strides=(8, 16, 32, 64))
    rng = np.random.default_rng(7)
    org = (500, 410)
    recs = []
    for k, (level, anchor, sides) in enumerate(((0, 0, (6.5, 6.25, 3, 3)),               # top-left corner: negative x0, y0
                                                (1, 3 * 38 + 25, (2, 2, 6.75, 1.5)),     # stride 16: centre x 408, right edge beyond 410
                                                (2, 15 * 19 + 4, (1, 2, 2, 5.5)),        # stride 32: centre y 496, bottom beyond 500
                                                (3, 7 * 10 + 6, (6.9, 6.9, 6.9, 6.9)))):  # stride 64: everything beyond
        cls = np.full(5, 0.03, np.float32)
        cls[k] = 0.55 + 0.1 * k
        recs.append(record(5, level, anchor, cls, sides=sides))
    return _case("clip", recs, cfg, org, True, rng)


def tenth_column_case():
    """inp_w = 608 at stride 64: ceil(9.5) = 10 columns, an anchor in the tenth"""
    cfg = make_cfg(ncls=5, strides=(8, 16, 32, 64))
    rng = np.random.default_rng(8)
    recs = []
    for k, anchor in enumerate((3 * 10 + 9, 4 * 10 + 0, 12 * 10 + 9)):
        cls = np.full(5, -3.0, np.float32)
        cls[3] = 0.7 + k
        recs.append(record(5, 3, anchor, cls, sides=(1.5, 2.25, 0.5, 1.75)))
    return _case("tenth_column", recs, cfg, (1000, 760), False, rng)


def threshold_edge_case():
    """probabilities one float32 step above (kept) and below (dropped) the threshold: with probabilities the host is exact, the margin is 0"""
    cfg = make_cfg(ncls=5, strides=(8, 16, 32))
    rng = np.random.default_rng(9)
    t = np.float32(cfg.score_threshold)
    recs = []
    for k, p in enumerate((np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), np.float32(0.75), np.float32(0.625))):
        cls = np.full(5, 0.04, np.float32)
        cls[1] = p
        recs.append(record(5, 1, 200 + 9 * k, cls, sides=(2, 2, 2, 2)))
    return _case("threshold_edge", recs, cfg, (800, 608), True, rng)


def nan_case():
    """a NaN class score is never a candidate; the record's other classes are"""
    cfg = make_cfg(ncls=5, strides=(8, 16, 32))
    rng = np.random.default_rng(10)
    recs = []
    for k in range(4):
        cls = np.full(5, 0.05, np.float32)
        cls[0] = 0.6 + 0.07 * k
        if k == 1:
            cls[0], cls[4] = np.nan, 0.9
        if k == 2:
            cls[3] = np.nan
        recs.append(record(5, k % 3, 300 + 11 * k, cls, sides=(3, 2, 3, 2)))
    return _case("nan", recs, cfg, (800, 608), True, rng)


def tie_case():
    """two exactly equal scores in one class on overlapping boxes: whichever is taken first suppresses the other.  No host order to match"""
    cfg = make_cfg(ncls=5, strides=(8, 16, 32))
    rng = np.random.default_rng(11)
    recs = []
    for col, p in ((20, 0.8), (22, 0.8), (40, 0.7)):
        cls = np.full(5, 0.01, np.float32)
        cls[2] = p
        recs.append(record(5, 0, 20 * 76 + col, cls, sides=(5, 5, 5, 5)))
    return _case("tie", recs, cfg, (800, 608), True, rng)


def batches():
    """name -> (cases of one op_layout_decode call: same configuration, B = 3 pages of different counts)"""
    c1 = make_cfg(ncls=1, strides=(8,), inp=(320, 320))
    c5 = make_cfg(ncls=5, strides=(8, 16, 32))
    c10 = make_cfg(ncls=10, strides=(8, 16, 32, 64))
    c5x4 = make_cfg(ncls=5, strides=(8, 16, 32, 64))
    cut = make_cfg(ncls=5, strides=(8, 16, 32), nms_top_k=16, keep_top_k=3)
    return {
        "one_class_one_level": [random_case("n260", 101, 260, c1, (400, 300), False, hot=1.0, region=20),      # > candidate_size in the class
                                random_case("n0", 102, 0, c1, (400, 300), False),
                                random_case("n1", 103, 1, c1, (400, 300), False, hot=1.0)],
        "five_classes_three_levels": [random_case("n37", 104, 37, c5, (1000, 760), False, hot=0.9),
                                      random_case("n90", 105, 90, c5, (1000, 760), False, hot=0.9),
                                      random_case("n5", 106, 5, c5, (1000, 760), False, hot=1.0)],
        "ten_classes_four_levels_probs": [random_case("p150", 107, 150, c10, (1100, 850), True, hot=0.9),
                                          random_case("p37", 108, 37, c10, (1100, 850), True, hot=0.9),
                                          random_case("p260", 109, 260, c10, (1100, 850), True, hot=0.9)],
        "both_cuts": [random_case("cut40", 110, 60, cut, (800, 608), False, level_counts=[40, 12, 8], hot=1.0),
                      random_case("cut17", 111, 30, cut, (800, 608), False, level_counts=[17, 13, 0], hot=1.0),
                      random_case("cut3", 112, 3, cut, (800, 608), False, hot=1.0)],
        "crafted": [chain_case(), zero_width_case(), threshold_edge_case()],
        "crafted2": [nan_case(), random_case("n12", 113, 12, c5, (800, 608), True, hot=1.0), random_case("n0b", 114, 0, c5, (800, 608), True)],
        "clip": [clip_case(), random_case("c37", 115, 37, c5x4, (500, 410), True, hot=0.9), random_case("c9", 116, 9, c5x4, (500, 410), True, hot=1.0)],
        "tenth_column": [tenth_column_case(), random_case("t37", 117, 37, c5x4, (1000, 760), False, hot=0.9),
                         random_case("t2", 118, 2, c5x4, (1000, 760), False, hot=1.0)],
    }


def all_cases():
    return [c for cs in batches().values() for c in cs]
