"""References for the generic executor's LSTM layer (helper, not a test), written from the ONNX operator definition of LSTM (opset 7 / 14):

    X [T, B, I], W [D, 4H, I], R [D, 4H, H], B [D, 8H] = [Wb | Rb], gates in the order i, o, f, c, zero initial states,
    i = sigmoid(X Wi^T + h Ri^T + Wbi + Rbi), o, f alike, g = tanh(X Wc^T + h Rc^T + Wbc + Rbc), c = f c + i g, h = o tanh(c),
    direction 1 of a bidirectional node (and a node with direction="reverse") walks t = T - 1 .. 0 and writes Y[t]; Y [T, D, B, H].

``lstm_fp64``: that, in float64.  ``lstm_emulated``: the same recurrence with the roundings of the engine's single-pass modes placed where the
engine has them -- the operands of the matrix products (X, W, R) and the stored intermediate values (the pre-gates X W^T + Wb + Rb, h once
per step) rounded to the 16-bit storage format (round to nearest even), products accumulated wider than fp32 and the sums kept in fp32, the
gate arithmetic and c in fp32 -- and exact sigmoid / tanh.  ``fmt=None`` switches every rounding off (then it is oracle/onnx_ref._lstm up to
fp32 round-off).  Its error against ``lstm_fp64`` is what 16-bit storage costs on a given case, computed on the CPU; the GPU tests bound the
engine's error by twice that (MFMA summation order, fast exponentials)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

_DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def round_to(a, fmt: Optional[str]) -> torch.Tensor:
    """fp32 tensor of the values after one rounding to the storage format (None: fp32 as it is)"""
    t = torch.as_tensor(np.asarray(a, np.float32) if not torch.is_tensor(a) else a).to(torch.float32)
    return t if fmt is None else t.to(_DT[fmt]).to(torch.float32)


def _walk(direction: str, d: int, T: int):
    return range(T - 1, -1, -1) if (d == 1 or direction == "reverse") else range(T)


def lstm_fp64(X, W, R, B, direction: str = "forward") -> np.ndarray:
    X, W, R = (torch.as_tensor(np.asarray(v, np.float64)) for v in (X, W, R))
    D, H = W.shape[0], R.shape[2]
    T, Bn, _ = X.shape
    Bv = torch.zeros(D, 8 * H, dtype=torch.float64) if B is None else torch.as_tensor(np.asarray(B, np.float64))
    Y = torch.zeros(T, D, Bn, H, dtype=torch.float64)
    for d in range(D):
        h = torch.zeros(Bn, H, dtype=torch.float64)
        c = torch.zeros(Bn, H, dtype=torch.float64)
        b = Bv[d, :4 * H] + Bv[d, 4 * H:]
        for t in _walk(direction, d, T):
            g = X[t] @ W[d].T + h @ R[d].T + b
            i, o, f, cc = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(cc)
            h = torch.sigmoid(o) * torch.tanh(c)
            Y[t, d] = h
    return Y.numpy()


def lstm_emulated(X, W, R, B, direction: str = "forward", fmt: Optional[str] = "bf16") -> np.ndarray:
    """-> Y [T, D, B, H] float32 (values representable in the storage format when fmt is given)"""
    Xr, Wr, Rr = round_to(X, fmt).double(), round_to(W, fmt).double(), round_to(R, fmt).double()
    D, H = Wr.shape[0], Rr.shape[2]
    T, Bn, _ = Xr.shape
    Bv = torch.zeros(D, 8 * H) if B is None else torch.as_tensor(np.asarray(B, np.float32))
    Y = torch.zeros(T, D, Bn, H, dtype=torch.float32)
    for d in range(D):
        b = (Bv[d, :4 * H].double() + Bv[d, 4 * H:].double()).float()
        pre = round_to(((Xr.reshape(T * Bn, -1) @ Wr[d].T).float() + b).reshape(T, Bn, 4 * H), fmt)       # the row GEMM's stored output
        h = torch.zeros(Bn, H, dtype=torch.float32)
        c = torch.zeros(Bn, H, dtype=torch.float32)
        for t in _walk(direction, d, T):
            g = pre[t] + (h.double() @ Rr[d].T).float()
            i, o, f, cc = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(cc)
            h = round_to(torch.sigmoid(o) * torch.tanh(c), fmt)
            Y[t, d] = h
    return Y.numpy()


def merge_directions(Y: np.ndarray) -> np.ndarray:
    """Y [T, D, B, H] -> [T, B, D H], forward units first (the exporter's Transpose(0, 2, 1, 3) + Reshape)"""
    T, D, Bn, H = Y.shape
    return np.ascontiguousarray(Y.transpose(0, 2, 1, 3)).reshape(T, Bn, D * H)


def linear_fp64(x, w, b) -> np.ndarray:
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)


def linear_emulated(x, w, b, fmt: Optional[str] = "bf16") -> np.ndarray:
    """the row GEMM: 16-bit operands, fp32 sum + fp32 bias, the stored result rounded"""
    y = (round_to(x, fmt).double() @ round_to(w, fmt).double().T).float() + torch.as_tensor(np.asarray(b, np.float32))
    return round_to(y, fmt).numpy()


def stack_fp64(x, layers, head=None) -> np.ndarray:
    """layers: [(W, R, B, direction)] applied in turn to x [T, B, I] (+ head = (w, b)) -> float64 [T, B, C]"""
    for W, R, B, direction in layers:
        x = merge_directions(lstm_fp64(x, W, R, B, direction))
    return x if head is None else linear_fp64(x, *head)


def stack_emulated(x, layers, head=None, fmt: Optional[str] = "bf16") -> np.ndarray:
    x = round_to(x, fmt).numpy()
    for W, R, B, direction in layers:
        x = merge_directions(lstm_emulated(x, W, R, B, direction, fmt))
    return x if head is None else linear_emulated(x, *head, fmt=fmt)
