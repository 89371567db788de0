"""Restatement of PaddleOCR's SLAHead (eval mode) + AttentionGRUCell in plain torch on the CPU, in any floating dtype: the reference of
pt_op_sla_decode (csrc/sla_head.hip; contract in include/pdftable_hip.h).  float64 is the reference, float32 the yardstick of the tests.

Parameters are a dict of numpy arrays by role (pdf_table_amd.weights.SLA_HEAD_ROLES), every matrix [out, in], GRU gates in the order r, z, c."""
import numpy as np
import torch

from pdf_table_amd.weights import FORMATS, SLA_HEAD_ROLES


def make_head(seed, H, C, V, L, gain=1.0):
    """float64 parameters of a random head: every matrix uniform in +-gain / sqrt(fan_in) x a per-role factor that keeps the walk lively
    (logits a few units apart, attention neither flat nor one-hot)"""
    g = np.random.default_rng(seed)

    def u(shape, fan_in, k=1.0):
        return g.uniform(-1.0, 1.0, shape) * (k * gain / np.sqrt(fan_in))
    p = {"i2h_w": u((H, C), C, 2.0), "h2h_w": u((H, H), H, 2.0), "h2h_b": u((H,), H), "score_w": u((H,), H, 8.0),
         "w_ih": u((3 * H, C + V), C, 2.0), "b_ih": u((3 * H,), H), "w_hh": u((3 * H, H), H, 2.0), "b_hh": u((3 * H,), H),
         "s1_w": u((H, H), H, 2.0), "s1_b": u((H,), H), "s2_w": u((V, H), H, 12.0), "s2_b": u((V,), 1, 0.5),
         "l1_w": u((H, H), H, 2.0), "l1_b": u((H,), H), "l2_w": u((L, H), H, 6.0), "l2_b": u((L,), 1, 0.5)}
    assert set(p) == set(SLA_HEAD_ROLES)
    return p


def make_fea(seed, B, N, C):
    return np.random.default_rng(seed).normal(0.0, 1.0, (B, N, C))


def storable(x, mode):
    """float64 array -> (value float64 that the storage mode holds exactly, (hi, lo) float64 parts; lo is zeros outside the pair mode)"""
    dt = FORMATS["f16" if mode == "f16" else "bf16"]
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(torch.float32)
    hi = t.to(dt).to(torch.float32)
    lo = (t - hi).to(dt).to(torch.float32) if mode == "split" else torch.zeros_like(hi)
    return (hi.double() + lo.double()).numpy(), (hi.double().numpy(), lo.double().numpy())


MATRICES = ("i2h_w", "h2h_w", "w_ih", "w_hh", "s1_w", "s2_w", "l1_w", "l2_w")


def storable_head(p, mode):
    """the head as the kernel reads it: matrices rounded to the 16-bit storage of `mode` (hi + lo in the pair mode), vectors rounded to fp32"""
    return {k: (storable(v, mode)[0] if k in MATRICES else np.asarray(v, np.float32).astype(np.float64)) for k, v in p.items()}


def sla_walk(p, fea, T, dtype=torch.float64, force_ids=None, eos_id=-1):
    """-> dict(probs [B, T, V], loc [B, T, L], logits [B, T, V], ids [B, T], steps [B]) as float64 / int64 numpy, computed in `dtype`.
    force_ids [B, T]: the id fed to step t + 1 (ids still report the arg-max).  eos_id >= 0: rows after a table's first id == eos_id at t > 0
    are zeros and steps[b] counts the rows written."""
    q = {k: torch.from_numpy(np.asarray(v, np.float64)).to(dtype) for k, v in p.items()}
    f = torch.from_numpy(np.asarray(fea, np.float64)).to(dtype)
    B, N, C = f.shape
    H, V, L = q["h2h_w"].shape[0], q["s2_w"].shape[0], q["l2_w"].shape[0]
    P = f @ q["i2h_w"].T                                                   # [B, N, H]
    h = torch.zeros(B, H, dtype=dtype)
    prev = torch.zeros(B, dtype=torch.long)
    out = {"probs": np.zeros((B, T, V)), "loc": np.zeros((B, T, L)), "logits": np.zeros((B, T, V)), "ids": np.zeros((B, T), np.int64)}
    steps = np.full(B, T, np.int64)
    live = np.ones(B, bool)
    w_ctx, w_hot = q["w_ih"][:, :C], q["w_ih"][:, C:]
    for t in range(T):
        qq = h @ q["h2h_w"].T + q["h2h_b"]
        e = torch.tanh(P + qq[:, None, :]) @ q["score_w"]                   # [B, N]
        alpha = torch.softmax(e, dim=1)
        ctx = (alpha[:, :, None] * f).sum(1)                               # [B, C]
        gi = ctx @ w_ctx.T + w_hot[:, prev].T + q["b_ih"]
        gh = h @ q["w_hh"].T + q["b_hh"]
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        c = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (h - c) * z + c
        s = (h @ q["s1_w"].T + q["s1_b"]) @ q["s2_w"].T + q["s2_b"]
        loc = torch.sigmoid((h @ q["l1_w"].T + q["l1_b"]) @ q["l2_w"].T + q["l2_b"])
        ids = np.argmax(s.double().numpy(), -1)                            # the lowest index among equal values
        for b in range(B):
            if live[b]:
                out["probs"][b, t] = torch.softmax(s[b], 0).double().numpy()
                out["loc"][b, t] = loc[b].double().numpy()
                out["logits"][b, t] = s[b].double().numpy()
                out["ids"][b, t] = ids[b]
                if eos_id >= 0 and t > 0 and ids[b] == eos_id:
                    live[b] = False
                    steps[b] = t + 1
        prev = torch.from_numpy(np.asarray(force_ids[:, t] if force_ids is not None else ids, np.int64))
    out["steps"] = steps
    return out


def top2_margin(logits):
    """[.., V] -> the gap between the largest and the second largest logit of every row (inf when V == 1)"""
    if logits.shape[-1] < 2:
        return np.full(logits.shape[:-1], np.inf)
    s = np.sort(logits, -1)
    return s[..., -1] - s[..., -2]


# ---- SLANetPreprocessor (model/slanet/processor_slanet.py:32-53 over db_pp/table_ops.py + image_operators.py), restated ----------------------------
def slanet_preprocess(img_rgb, max_len=488):
    """RGB uint8 [h, w, 3] -> (float32 [3, max_len, max_len] in B, G, R order, shape [h, w, ratio, ratio, max_len, max_len]):
    the image read as BGR, ratio = max_len / max(h, w), cv2.resize (bilinear) to (int(w ratio), int(h ratio)), (x * (1 / 255) - mean) / std in
    float32 with mean / std indexed in that BGR order, zero padding at the bottom and the right"""
    from oracle.db_pre import cv2_resize_linear_u8
    img = np.ascontiguousarray(np.asarray(img_rgb)[:, :, ::-1])
    h, w = img.shape[:2]
    ratio = max_len / (max(h, w) * 1.0)
    rh, rw = int(h * ratio), int(w * ratio)
    res = cv2_resize_linear_u8(img, rw, rh)
    mean = np.array([0.485, 0.456, 0.406]).reshape(1, 1, 3).astype("float32")
    std = np.array([0.229, 0.224, 0.225]).reshape(1, 1, 3).astype("float32")
    norm = (res.astype("float32") * np.float32(1.0 / 255.0) - mean) / std
    pad = np.zeros((max_len, max_len, 3), dtype=np.float32)
    pad[:rh, :rw] = norm
    return pad.transpose(2, 0, 1), np.array([h, w, ratio, ratio, max_len, max_len])
