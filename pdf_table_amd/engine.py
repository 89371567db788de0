"""Python handle on one MI355X engine (one per GPU / per process).

PyTorch is used here only as plumbing: it owns the caller-side device buffers (inputs / outputs) and
the HIP stream; every compute call goes through the C ABI of libpdftable_hip.so.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import threading
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L

__all__ = ["HipEngine", "REC_LINE_DTYPE", "CLS_IMAGE_DTYPE", "REC_PP_ITEM_DTYPE"]

# mirrors struct pt_rec_line in include/pdftable_hip.h (88 bytes)
TSR_TABLE_DTYPE = np.dtype([("minv", "<f8", (6,)), ("page", "<i4"), ("x0", "<i4"), ("y0", "<i4"),
                            ("crop_w", "<i4"), ("crop_h", "<i4"), ("reserved", "<i4")])   # struct pt_tsr_table
CLS_IMAGE_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])      # pt_cls_image
REC_LINE_DTYPE = np.dtype([("minv", np.float64, (9,)), ("page", np.int32), ("crop_w", np.int32), ("crop_h", np.int32),
                           ("reserved", np.int32)])


REC_PP_ITEM_DTYPE = np.dtype([("line", "<i4"), ("resized_w", "<i4"), ("img_w", "<i4"), ("reserved", "<i4"),
                              ("out_off", "<i8")])                               # struct pt_rec_pp_item (24 bytes)


def _upload(arr: np.ndarray, device) -> torch.Tensor:
    """small host array -> device through pinned memory, asynchronously: a pageable `.to(device)` would block the host
    until everything already queued on the stream has run"""
    return torch.from_numpy(np.ascontiguousarray(arr)).pin_memory().to(device, non_blocking=True)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def mtl_pick_split(ntiles: int, hw: int) -> Tuple[int, int]:
    """pt_op_mtl_pick_split: (nsplit, keys_per_split) of the MtlTabNet decoders' source attention for `ntiles` query tiles over hw keys.  Host
    arithmetic of the library: needs no device and no engine."""
    ns, kps = C.c_int(), C.c_int()
    L.check(L.load().pt_op_mtl_pick_split(int(ntiles), int(hw), C.byref(ns), C.byref(kps)), "pt_op_mtl_pick_split")
    return ns.value, kps.value


def teds_scratch_bytes(n1: int, n2: int) -> int:
    """pt_op_teds_scratch_bytes: the scratch pt_op_teds_dist needs for one pair of trees with n1 and n2 nodes (1 .. 4096 each).  Host arithmetic of the
    library: needs no device and no engine."""
    n = C.c_longlong()
    L.check(L.load().pt_op_teds_scratch_bytes(int(n1), int(n2), C.byref(n)), "pt_op_teds_scratch_bytes")
    return int(n.value)


class HipEngine:
    def __init__(self, device: int = 0):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.PtError("no HIP device visible: the engine has no CPU fallback")
        self.device = int(device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        L.check(self.lib.pt_engine_create(self.device, C.byref(h)), "pt_engine_create")
        self._h = h
        self._tdev = torch.device("cuda", self.device)
        self.precision = L.PT_PRECISION_BF16
        # Precision is engine-wide HOST state that every call reads when it is queued (the dispatcher picks the pt_bf16 / pt_f16 namespace and the
        # pair layout from it).  The C ABI leaves serialising calls on one engine to the caller; this handle does it: every public method takes
        # this re-entrant lock, and precision_scope() holds it across {set, queue the stage's calls, restore}, so that a call from another host
        # thread (MtlStage.stream's worker, a user's own) can never be queued in somebody else's temporary precision.
        self._lock = threading.RLock()

    @contextlib.contextmanager
    def precision_scope(self, precision: Optional[int]):
        """``with eng.precision_scope(L.PT_PRECISION_BF16X3): eng.layout_forward(...)`` -- the calls QUEUED inside run in `precision` (None: no
        change), the engine's own precision is back afterwards; other threads' engine calls wait outside the scope."""
        with self._lock:
            keep = self.precision
            if precision is not None and int(precision) != keep:
                self.set_precision(int(precision))
            try:
                yield
            finally:
                if self.precision != keep:
                    self.set_precision(keep)

    def set_precision(self, precision: int):
        """L.PT_PRECISION_BF16 (throughput), L.PT_PRECISION_BF16X3 (fp32-class parity mode: three bf16 passes), L.PT_PRECISION_F16X2 (the
        same activation pairs against single fp16 weights: two fp16 passes, weight rounding ~1.5e-4 of the logit scale) or L.PT_PRECISION_F16
        (single-pass IEEE half, the reference's own GPU arithmetic: same speed as BF16 with 11 significant bits instead of 8; the weight blobs
        must be packed with ``fmt="f16"`` -- ``weight_fmt`` -- and the 16-bit tensors of the API are torch.float16)."""
        L.check(self.lib.pt_engine_set_precision(self._h, int(precision)), "pt_engine_set_precision")
        self.precision = int(precision)

    @property
    def split(self) -> bool:
        """activations cross the ABI as (hi | lo) bf16 pairs (twice the channels): the two pair modes"""
        return self.precision in (L.PT_PRECISION_BF16X3, L.PT_PRECISION_F16X2)

    @property
    def act_dtype(self):
        """torch dtype of the 16-bit activation tensors of the current precision (csrc/act16.h): float16 under PT_PRECISION_F16, else bfloat16"""
        return torch.float16 if self.precision == L.PT_PRECISION_F16 else torch.bfloat16

    @property
    def weight_fmt(self) -> str:
        """the ``fmt`` argument weights.pack_* need for blobs this engine will accept under its current precision"""
        return "f16" if self.precision == L.PT_PRECISION_F16 else "bf16"

    def set_mtl_kv_fp8(self, on: bool):
        """MtlTabNet, bf16 mode: stream the structure loop's source-attention keys / values as fp8 (half the bytes of the loop's dominant
        HBM stream; a throughput option with recorded drift, off by default)"""
        L.check(self.lib.pt_engine_set_mtl_kv_fp8(self._h, 1 if on else 0), "pt_engine_set_mtl_kv_fp8")

    def set_dcn_mfma(self, on):
        """Lore detector, bf16 mode: deformable convolutions with the bilinear blend on the matrix pipe (on) or on the VALU with fp32
        weights (off, the default); see include/pdftable_hip.h"""
        L.check(self.lib.pt_engine_set_dcn_mfma(self._h, int(on)), "pt_engine_set_dcn_mfma")      # 0 VALU blend, 1 dcn_mfma_kernel, 2 dcn_mfma2_kernel (64-output layers)

    def set_lstm_cluster(self, on: bool):
        """False: the streaming LSTM kernel (no co-residency requirement) -- whenever the recogniser shares the GPU with
        work on another stream; True (default): the weight-stationary cluster kernel."""
        L.check(self.lib.pt_engine_set_lstm_cluster(self._h, 1 if on else 0), "pt_engine_set_lstm_cluster")

    def check(self):
        """Raise PtError if the device flagged a failure in work already executed (pt_engine_check): call after the
        stream was synchronised, before consuming recognition results."""
        L.check(self.lib.pt_engine_check(self._h), "pt_engine_check")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pt_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- plumbing -------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self._tdev).cuda_stream)

    def _chk(self, t: torch.Tensor, dtype, name):
        if not (t.is_cuda and t.device.index == self.device and t.dtype == dtype and t.is_contiguous()):
            raise L.PtError(f"{name}: expected contiguous {dtype} tensor on cuda:{self.device}, got "
                            f"{t.dtype} on {t.device} (contiguous={t.is_contiguous()})")

    # ---- weights ----------------------------------------------------------------------------------
    def load_weights(self, kind: int, blob: bytes):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        L.check(self.lib.pt_weights_load(self._h, kind, C.cast(buf, C.c_void_p), len(blob)), "pt_weights_load")

    def load_weights_device(self, kind: int, blob_u8: torch.Tensor):
        self._chk(blob_u8, torch.uint8, "blob")
        L.check(self.lib.pt_weights_load_device(self._h, kind, _ptr(blob_u8), blob_u8.numel(), self._stream()),
                "pt_weights_load_device")

    # ---- detection --------------------------------------------------------------------------------
    def det_plan(self, h: int, w: int, flavour: int = L.PT_DET_PRE_DB_PP) -> Tuple[int, int]:
        nh, nw = C.c_int(), C.c_int()
        L.check(self.lib.pt_det_plan(h, w, flavour, C.byref(nh), C.byref(nw)), "pt_det_plan")
        return nh.value, nw.value

    def det_forward(self, pages: torch.Tensor, flavour: int = L.PT_DET_PRE_DB_PP, thresh: float = 0.3,
                    use_dilation: bool = False, want_bitmap: bool = True, out_prob=None, out_bitmap=None):
        """pages uint8 [n,h,w,3] RGB on the GPU -> (prob f32 [n,nh,nw], bitmap int32 [n,nh,nw/32] or None)."""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, c = pages.shape
        assert c == 3
        nh, nw = self.det_plan(h, w, flavour)
        prob = out_prob if out_prob is not None else torch.empty((n, nh, nw), dtype=torch.float32, device=self._tdev)
        bitmap = None
        if want_bitmap:
            bitmap = out_bitmap if out_bitmap is not None else torch.empty((n, nh, nw // 32), dtype=torch.int32,
                                                                             device=self._tdev)
        L.check(self.lib.pt_det_forward(self._h, _ptr(pages), n, h, w, flavour, float(thresh), int(use_dilation),
                                        _ptr(prob), _ptr(bitmap), self._stream()), "pt_det_forward")
        return prob, bitmap

    def det_preprocess(self, pages: torch.Tensor, flavour: int = L.PT_DET_PRE_DB_PP) -> torch.Tensor:
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        nh, nw = self.det_plan(h, w, flavour)
        out = torch.empty((n, nh, nw, 8 if self.split else 4), dtype=self.act_dtype,
                          device=self._tdev)
        L.check(self.lib.pt_det_preprocess(self._h, _ptr(pages), n, h, w, flavour, _ptr(out), self._stream()),
                "pt_det_preprocess")
        return out

    def det_forward_net(self, x: torch.Tensor, want_logits: bool = False):
        """x bf16 NHWC4 [n,H,W,4] (BF16X3 mode: [n,H,W,8] = hi rgb0 | lo rgb0) -> prob f32 [n,H,W] (and logits)."""
        self._chk(x, self.act_dtype, "x")
        n, H, W, c = x.shape
        assert c == (8 if self.split else 4)
        prob = torch.empty((n, H, W), dtype=torch.float32, device=self._tdev)
        logits = torch.empty((n, H, W), dtype=torch.float32, device=self._tdev) if want_logits else None
        L.check(self.lib.pt_det_forward_net(self._h, _ptr(x), n, H, W, _ptr(prob), _ptr(logits), self._stream()),
                "pt_det_forward_net")
        return (prob, logits) if want_logits else prob

    # ---- layout (PicoDet) ----------------------------------------------------------------------------------------
    def layout_plan(self, inp_h: int, inp_w: int):
        fh, fw = (C.c_int * 4)(), (C.c_int * 4)()
        L.check(self.lib.pt_layout_plan(inp_h, inp_w, fh, fw), "pt_layout_plan")
        return list(fh), list(fw)

    def layout_preprocess(self, pages: torch.Tensor, inp_h: int = 800, inp_w: int = 608) -> torch.Tensor:
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        out = torch.empty((n, inp_h, inp_w, 8 if self.split else 4), dtype=self.act_dtype,
                          device=self._tdev)
        L.check(self.lib.pt_layout_preprocess(self._h, _ptr(pages), n, h, w, inp_h, inp_w, _ptr(out), self._stream()),
                "pt_layout_preprocess")
        return out

    def layout_forward_net(self, x: torch.Tensor):
        """x bf16 NHWC4 [n,H,W,4|8] -> 4 head maps f32 [n, A_l, 40] (class logits, then box-distribution logits)"""
        self._chk(x, self.act_dtype, "x")
        n, H, W, _ = x.shape
        fh, fw = self.layout_plan(H, W)
        heads = [torch.empty((n, fh[l] * fw[l], L.PT_LAYOUT_HEAD_CS), dtype=torch.float32, device=self._tdev) for l in range(4)]
        L.check(self.lib.pt_layout_forward_net(self._h, _ptr(x), n, H, W, *[_ptr(t) for t in heads], self._stream()),
                "pt_layout_forward_net")
        return heads

    def layout_forward(self, pages: torch.Tensor, inp_h: int = 800, inp_w: int = 608, num_classes: int = 5,
                       thr_lo: float = 0.45, max_cands: int = 2048):
        """pages uint8 [n,h,w,3] -> (counts int32 [n] on the host, candidate records f32 [n, max_cands, 48] on the device)"""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        counts = torch.zeros((n,), dtype=torch.int32, device=self._tdev)
        cands = torch.empty((n, max_cands, L.PT_LAYOUT_CAND_FLOATS), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_layout_forward(self._h, _ptr(pages), n, h, w, inp_h, inp_w, num_classes, float(thr_lo), max_cands,
                                           _ptr(counts), _ptr(cands), self._stream()), "pt_layout_forward")
        return counts, cands

    def tsr_preprocess(self, pages: torch.Tensor, tables, inp_h: int = 1024, inp_w: int = 1024, bgr: bool = True):
        """pages uint8 [np,h,w,3] on the device, tables: numpy array of TSR_TABLE_DTYPE -> bf16 NHWC4 [n,inp_h,inp_w,4|8]."""
        self._chk(pages, torch.uint8, "pages")
        npg, ph, pw, _ = pages.shape
        n = len(tables)
        tb = _upload(tables.view(np.uint8).reshape(n, -1), self._tdev)
        out = torch.empty((n, inp_h, inp_w, 8 if self.split else 4), dtype=self.act_dtype,
                          device=self._tdev)
        L.check(self.lib.pt_tsr_preprocess(self._h, _ptr(pages), npg, ph, pw, _ptr(tb), n, inp_h, inp_w, int(bgr), _ptr(out),
                                           self._stream()), "pt_tsr_preprocess")
        return out

    def tsr_forward_net(self, x: torch.Tensor, wireless: bool = False):
        """Lore detector (DLA-34 + DCN, or the ResNet-18 'wireless' one): x bf16 NHWC4 [n,H,W,4] (BF16X3: 8 channels) ->
        dict of fp32 NHWC head maps at H/4 x W/4 ({'hm': [n,h,w,2], 'st': [.,8], 'wh': [.,8], 'ax': [.,256],
        'cr': [.,256], 'reg': [.,2]})."""
        self._chk(x, self.act_dtype, "x")
        n, H, W, c = x.shape
        assert c == (8 if self.split else 4)
        h, w = H // 4, W // 4
        bufs = {k: torch.empty((n, h, w, 256 if k in ("ax", "cr") else 8), dtype=torch.float32, device=self._tdev)
                for k in ("hm", "st", "wh", "ax", "cr", "reg")}
        fn = self.lib.pt_tsr_forward_net_wireless if wireless else self.lib.pt_tsr_forward_net
        L.check(fn(self._h, _ptr(x), n, H, W, _ptr(bufs["hm"]), _ptr(bufs["st"]), _ptr(bufs["wh"]), _ptr(bufs["ax"]),
                   _ptr(bufs["cr"]), _ptr(bufs["reg"]), self._stream()), "pt_tsr_forward_net")
        bufs["hm"] = bufs["hm"][..., :2]
        bufs["reg"] = bufs["reg"][..., :2]
        return bufs

    def tsr_decode(self, heads, wiz_rev: bool = True, vis_thresh: float = 0.2, sync: bool = True):
        """heads: dict of fp32 NHWC maps (hm/st/wh/reg with 8-channel stride or their [..., :k] views, ax/cr 256)
        -> (counts int32 [n] on the host -- or still on the device when sync=False --, dets f32 [n,3000,9],
        logi f32 [n,3000,256] on the device)."""
        def full(t, c):
            if t.shape[-1] != c or not t.is_contiguous():
                base = t._base if t._base is not None else t
                assert base.shape[-1] == c and base.is_contiguous(), "head map must come from tsr_forward_net"
                return base
            return t
        hm, st, wh, reg = (full(heads[k], 8) for k in ("hm", "st", "wh", "reg"))
        ax, cr = full(heads["ax"], 256), full(heads["cr"], 256)
        n, h, w, _ = ax.shape
        counts = torch.zeros((n,), dtype=torch.int32, device=self._tdev)
        dets = torch.empty((n, L.PT_TSR_MAX_CELLS, 9), dtype=torch.float32, device=self._tdev)
        logi = torch.empty((n, L.PT_TSR_MAX_CELLS, 256), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_tsr_decode(self._h, _ptr(hm), _ptr(st), _ptr(wh), _ptr(ax), _ptr(cr), _ptr(reg), n, h, w,
                                       int(wiz_rev), float(vis_thresh), _ptr(counts), _ptr(dets), _ptr(logi),
                                       self._stream()), "pt_tsr_decode")
        return (counts.cpu().numpy() if sync else counts), dets, logi

    def tsr_forward_decode(self, x: torch.Tensor, wiz_rev: bool = True, vis_thresh: float = 0.2, sync: bool = True, out=None):
        """DLA-34 forward + decode in one call (sparse ax / cr heads): x bf16 NHWC4 [n,H,W,4|8] -> the outputs of tsr_decode.
        out: (counts i32 [n] zeroed, dets f32 [n,3000,9], logi f32 [n,3000,256]) contiguous device tensors to write into
        (slices of a larger allocation: several micro-batches then feed ONE processor call)"""
        self._chk(x, self.act_dtype, "x")
        n, H, W, _ = x.shape
        if out is not None:
            counts, dets, logi = out
            assert counts.shape == (n,) and dets.shape == (n, L.PT_TSR_MAX_CELLS, 9) and logi.shape == (n, L.PT_TSR_MAX_CELLS, 256)
            assert counts.is_contiguous() and dets.is_contiguous() and logi.is_contiguous()
        else:
            counts = torch.zeros((n,), dtype=torch.int32, device=self._tdev)
            dets = torch.empty((n, L.PT_TSR_MAX_CELLS, 9), dtype=torch.float32, device=self._tdev)
            logi = torch.empty((n, L.PT_TSR_MAX_CELLS, 256), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_tsr_forward_decode(self._h, _ptr(x), n, H, W, int(wiz_rev), float(vis_thresh), _ptr(counts),
                                               _ptr(dets), _ptr(logi), self._stream()), "pt_tsr_forward_decode")
        return (counts.cpu().numpy() if sync else counts), dets, logi

    def tsr_band_radius(self) -> int:
        """receptive-field radius, in input rows, of the DLA-34 front segment (base_layer .. level2)"""
        return int(self.lib.pt_tsr_band_radius())

    def tsr_plan_bands(self, tables, inp_h: int = 1024, inp_w: int = 1024, max_stack_rows: int = 0):
        """pt_tsr_plan_bands (host arithmetic of the library): tables numpy TSR_TABLE_DTYPE -> (bands int32 [n, 8] = full, row0, row1,
        keep0, keep1, stack, stack_row, reserved; number of stacks; fraction of the n * inp_h rows planned)"""
        tb = np.ascontiguousarray(tables)
        n = len(tb)
        out = np.zeros((n, 8), np.int32)
        ns, frac = C.c_int(0), C.c_double(0.0)
        L.check(self.lib.pt_tsr_plan_bands(tb.ctypes.data, n, inp_h, inp_w, int(max_stack_rows), out.ctypes.data, C.byref(ns), C.byref(frac)),
                "pt_tsr_plan_bands")
        return out, int(ns.value), float(frac.value)

    def tsr_warp_forward_decode(self, pages: torch.Tensor, tables, inp_h: int = 1024, inp_w: int = 1024, bgr: bool = True, wiz_rev: bool = True,
                                vis_thresh: float = 0.2, sync: bool = True, out=None):
        """tsr_preprocess + tsr_forward_decode in one call (pt_tsr_warp_forward_decode): the detector's front segment runs on the row bands the
        letterboxed crops fill.  pages uint8 [np,h,w,3] on the device, tables numpy TSR_TABLE_DTYPE; out as for tsr_forward_decode."""
        self._chk(pages, torch.uint8, "pages")
        npg, ph, pw, _ = pages.shape
        tb_h = np.ascontiguousarray(tables)
        n = len(tb_h)
        tb = _upload(tb_h.view(np.uint8).reshape(n, -1), self._tdev)
        if out is not None:
            counts, dets, logi = out
            assert counts.shape == (n,) and dets.shape == (n, L.PT_TSR_MAX_CELLS, 9) and logi.shape == (n, L.PT_TSR_MAX_CELLS, 256)
            assert counts.is_contiguous() and dets.is_contiguous() and logi.is_contiguous()
        else:
            counts = torch.zeros((n,), dtype=torch.int32, device=self._tdev)
            dets = torch.empty((n, L.PT_TSR_MAX_CELLS, 9), dtype=torch.float32, device=self._tdev)
            logi = torch.empty((n, L.PT_TSR_MAX_CELLS, 256), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_tsr_warp_forward_decode(self._h, _ptr(pages), npg, ph, pw, tb_h.ctypes.data, _ptr(tb), n, inp_h, inp_w, int(bgr),
                                                    int(wiz_rev), float(vis_thresh), _ptr(counts), _ptr(dets), _ptr(logi), self._stream()),
                "pt_tsr_warp_forward_decode")
        return (counts.cpu().numpy() if sync else counts), dets, logi

    def op_tsr_level2(self, pages: torch.Tensor, tables, inp_h: int, inp_w: int, bgr: bool = True, bands: bool = True, margin: int = -1):
        """pt_op_tsr_level2 (test hook): `layers[2]` of the DLA-34 base for the table crops, [n, inp_h/4, inp_w/4, 64 | 128] in the activation format;
        bands=False: on whole maps; margin >= 0 plans the bands with that radius (wrong below tsr_band_radius())."""
        self._chk(pages, torch.uint8, "pages")
        npg, ph, pw, _ = pages.shape
        tb_h = np.ascontiguousarray(tables)
        n = len(tb_h)
        tb = _upload(tb_h.view(np.uint8).reshape(n, -1), self._tdev)
        out = torch.empty((n, inp_h // 4, inp_w // 4, 128 if self.split else 64), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_tsr_level2(self._h, _ptr(pages), npg, ph, pw, tb_h.ctypes.data, _ptr(tb), n, inp_h, inp_w, int(bgr), int(bands),
                                          int(margin), _ptr(out), self._stream()), "pt_op_tsr_level2")
        return out

    def centernet_forward_net(self, x: torch.Tensor):
        """CenterNet table-cell detector (DLA-34 + DLAUp, PT_MODEL_CENTERNET_DLA34): x bf16 NHWC4 [n,H,W,4] (BF16X3: 8 channels) -> dict of
        fp32 NHWC head maps at H/4 x W/4 ({'hm': [n,h,w,2] pre-sigmoid, 'v2c': [.,8], 'c2v': [.,8], 'reg': [.,2]}; hm / reg are views of
        8-channel-stride maps)."""
        self._chk(x, self.act_dtype, "x")
        n, H, W, c = x.shape
        assert c == (8 if self.split else 4)
        bufs = {k: torch.empty((n, H // 4, W // 4, 8), dtype=torch.float32, device=self._tdev) for k in ("hm", "v2c", "c2v", "reg")}
        L.check(self.lib.pt_centernet_forward_net(self._h, _ptr(x), n, H, W, _ptr(bufs["hm"]), _ptr(bufs["v2c"]), _ptr(bufs["c2v"]),
                                                  _ptr(bufs["reg"]), self._stream()), "pt_centernet_forward_net")
        bufs["hm"] = bufs["hm"][..., :2]
        bufs["reg"] = bufs["reg"][..., :2]
        return bufs

    def centernet_decode(self, heads, affines, sync: bool = True):
        """heads: the dict of centernet_forward_net (or fp32 NHWC maps of 8 channels: hm / reg may be their [..., :2] views); affines:
        float64 [n, 2, 3], per table the inverse map head-map pixels -> crop pixels -> (counts int32 [n] on the host -- or still on the
        device when sync=False --, cells f32 [n, 1000, 9] on the device: rows [0, counts[i]) = 8 crop-pixel coordinates + score, in
        top-K order, every cell with score >= 0.3)"""
        def full(t):
            if t.shape[-1] != 8 or not t.is_contiguous():
                base = t._base if t._base is not None else t
                assert base.shape[-1] == 8 and base.is_contiguous(), "head map must come from centernet_forward_net"
                return base
            return t
        hm, v2c, c2v, reg = (full(heads[k]) for k in ("hm", "v2c", "c2v", "reg"))
        for t in (hm, v2c, c2v, reg):
            self._chk(t, torch.float32, "head map")
        n, h, w, _ = hm.shape
        aff = np.ascontiguousarray(np.asarray(affines, np.float64).reshape(n, 6))
        d_aff = _upload(aff, self._tdev)
        counts = torch.zeros((n,), dtype=torch.int32, device=self._tdev)
        cells = torch.empty((n, L.PT_CENTERNET_MAX_CELLS, 9), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_centernet_decode(self._h, _ptr(hm), _ptr(v2c), _ptr(c2v), _ptr(reg), n, h, w, _ptr(d_aff), _ptr(counts),
                                             _ptr(cells), self._stream()), "pt_centernet_decode")
        return (counts.cpu().numpy() if sync else counts), cells

    DOCX_HEADS = {"cls": 4, "ftype": 3, "hm": 11, "hm_sub": 2, "reg": 2, "reg_sub": 2, "wh": 8, "wh_sub": 8}     # configuration_docxlayout.py:45-46

    def docx_preprocess(self, pages: torch.Tensor, tables, inp_h: int = 768, inp_w: int = 768, bgr: bool = True,
                        mean=(0.40789655, 0.44719303, 0.47026116), std=(0.2886383, 0.27408165, 0.27809834)):
        """tsr_preprocess's warp with ``((v / 255) - mean) / std`` for the constants given (float32, in the order of the output channels):
        pages uint8 [np,h,w,3] on the device, tables numpy TSR_TABLE_DTYPE -> 16-bit NHWC4 [n,inp_h,inp_w,4|8] (pt_docx_preprocess)."""
        self._chk(pages, torch.uint8, "pages")
        npg, ph, pw, _ = pages.shape
        n = len(tables)
        tb = _upload(tables.view(np.uint8).reshape(n, -1), self._tdev)
        out = torch.empty((n, inp_h, inp_w, 8 if self.split else 4), dtype=self.act_dtype, device=self._tdev)
        m3 = (C.c_float * 3)(*[float(v) for v in mean])
        s3 = (C.c_float * 3)(*[float(v) for v in std])
        L.check(self.lib.pt_docx_preprocess(self._h, _ptr(pages), npg, ph, pw, _ptr(tb), n, inp_h, inp_w, int(bgr), m3, s3, _ptr(out),
                                            self._stream()), "pt_docx_preprocess")
        return out

    def docx_forward_net(self, x: torch.Tensor, out=None):
        """DocXLayout layout detector (DLA-34 + DLAUp + eight heads, PT_MODEL_DOCX_DLA34): x 16-bit NHWC4 [n,H,W,4] (pair modes: 8 channels) ->
        dict of fp32 NHWC head maps at H/4 x W/4, pre-sigmoid: 'hm' [n,h,w,16] (11 valid), every other head [n,h,w,8] (DOCX_HEADS valid).
        out: such a dict to write into (slices of a larger allocation: several micro-batches then feed ONE decode launch)."""
        self._chk(x, self.act_dtype, "x")
        n, H, W, c = x.shape
        assert c == (8 if self.split else 4)
        if out is None:
            out = {k: torch.empty((n, H // 4, W // 4, 16 if k == "hm" else 8), dtype=torch.float32, device=self._tdev) for k in self.DOCX_HEADS}
        for k in self.DOCX_HEADS:
            self._chk(out[k], torch.float32, k)
            assert tuple(out[k].shape) == (n, H // 4, W // 4, 16 if k == "hm" else 8), (k, tuple(out[k].shape))
        L.check(self.lib.pt_docx_forward_net(self._h, _ptr(x), n, H, W, *[_ptr(out[k]) for k in ("cls", "ftype", "hm", "hm_sub", "reg", "reg_sub", "wh",
                                                                                                "wh_sub")], self._stream()), "pt_docx_forward_net")
        return out

    def docx_decode(self, heads, top_k: int = 100, thr_lo: float = 0.3 - 1e-3, ncls_main: int = 11, ncls_sub: int = 2, out=None, with_inds: bool = True):
        """heads: the dict of docx_forward_net -> (counts int32 [n,2], records f32 [n,2,K,12], flat indices int32 [n,2,K] or None, keep uint8 [n,2,K]),
        all on the device (pt_docx_decode: peaks, joint top-K, corners, arg-max columns and the polygon NMS of both branches in one launch).  Rows at
        and behind a count are not written.  out: the four tensors to write into."""
        n, h, w, _ = heads["hm"].shape
        for k in self.DOCX_HEADS:
            self._chk(heads[k], torch.float32, k)
            assert tuple(heads[k].shape) == (n, h, w, 16 if k == "hm" else 8), (k, tuple(heads[k].shape))
        K = int(top_k)
        if out is None:
            out = (torch.zeros((n, 2), dtype=torch.int32, device=self._tdev),
                   torch.zeros((n, 2, max(K, 1), L.PT_DOCX_REC_FLOATS), dtype=torch.float32, device=self._tdev),
                   torch.zeros((n, 2, max(K, 1)), dtype=torch.int32, device=self._tdev) if with_inds else None,
                   torch.zeros((n, 2, max(K, 1)), dtype=torch.uint8, device=self._tdev))
        counts, recs, inds, keep = out
        kb = max(K, 1)      # an out-of-range K is refused by the library; the buffers must hold whatever K it may accept
        assert tuple(counts.shape) == (n, 2) and counts.dtype == torch.int32 and counts.is_contiguous()
        assert tuple(recs.shape) == (n, 2, recs.shape[2], L.PT_DOCX_REC_FLOATS) and recs.dtype == torch.float32 and recs.is_contiguous()
        assert tuple(keep.shape) == (n, 2, recs.shape[2]) and keep.dtype == torch.uint8 and keep.is_contiguous()
        assert inds is None or (tuple(inds.shape) == (n, 2, recs.shape[2]) and inds.dtype == torch.int32 and inds.is_contiguous())
        assert recs.shape[2] == kb or not 1 <= K <= L.PT_DOCX_MAX_K, (recs.shape, K)
        L.check(self.lib.pt_docx_decode(_ptr(heads["hm"]), _ptr(heads["wh"]), _ptr(heads["reg"]), _ptr(heads["cls"]), _ptr(heads["ftype"]),
                                        _ptr(heads["hm_sub"]), _ptr(heads["wh_sub"]), _ptr(heads["reg_sub"]), n, h, w, int(ncls_main), int(ncls_sub), K,
                                        float(thr_lo), _ptr(counts), _ptr(recs), _ptr(inds), _ptr(keep), self._stream()), "pt_docx_decode")
        return counts, recs, inds, keep

    def op_docx_order(self, counts: torch.Tensor, recs: torch.Tensor, keep: torch.Tensor, affine, scores_thresh: float = 0.3, top_k: int = 100,
                      num_classes: int = 13, n_main: int = 11, use_nms: bool = True, out=None):
        """docx_page_result for every page of a batch in one launch (pt_op_docx_order, csrc/docx_order.hip).  counts int32 [B,2] / recs float32
        [B,2,K,12] / keep uint8 [B,2,K]: what docx_decode returns; affine: the float64 [2,3] of centernet_decode_affine(page_h, page_w, map_h, map_w)
        -> (n_out int32 [B], flag int32 [B], rows float32 [B,2K,6] = (x0, y0, x2, y2 of the rounded vertices, score, 0-based class) in reading
        order) on the device.  flag != 0: the page needs the host route (a list of 64 or more blocks in a sort, ...) and has no rows; rows at and
        behind n_out are left as they were.  out: (n_out, flag, rows) to write into.  Everything stays on the device; nothing synchronises."""
        import numpy as np
        self._chk(counts, torch.int32, "counts")
        self._chk(recs, torch.float32, "recs")
        self._chk(keep, torch.uint8, "keep")
        if recs.dim() != 4 or recs.shape[1] != 2 or recs.shape[3] != L.PT_DOCX_REC_FLOATS or tuple(counts.shape) != (recs.shape[0], 2) \
                or tuple(keep.shape) != tuple(recs.shape[:3]):
            raise ValueError(f"op_docx_order: counts [B,2], recs [B,2,K,{L.PT_DOCX_REC_FLOATS}] and keep [B,2,K] expected, got {tuple(counts.shape)}, "
                             f"{tuple(recs.shape)} and {tuple(keep.shape)}")
        B, K = int(recs.shape[0]), int(recs.shape[2])
        m = np.asarray(affine, np.float64).reshape(6)
        if out is None:
            out = (torch.zeros((B,), dtype=torch.int32, device=self._tdev), torch.zeros((B,), dtype=torch.int32, device=self._tdev),
                   torch.zeros((B, 2 * K, 6), dtype=torch.float32, device=self._tdev))
        n_out, flag, rows = out
        self._chk(n_out, torch.int32, "n_out")
        self._chk(flag, torch.int32, "flag")
        self._chk(rows, torch.float32, "rows")
        if n_out.numel() < B or flag.numel() < B or rows.numel() < B * 2 * K * 6:
            raise ValueError("op_docx_order: output buffers too small")
        L.check(self.lib.pt_op_docx_order(_ptr(counts), _ptr(recs), _ptr(keep), B, K, *[float(v) for v in m], float(scores_thresh), int(top_k),
                                          int(num_classes), int(n_main), int(bool(use_nms)), _ptr(n_out), _ptr(flag), _ptr(rows), self._stream()),
                "pt_op_docx_order")
        return n_out, flag, rows

    def tsr_process(self, logi: torch.Tensor, dets: torch.Tensor, counts, use_2dpe: bool = False):
        """logic features of pt_tsr_decode -> (logic_axis, stacked_axis) f32 [n,3000,4]; rows [0, counts[i]) valid."""
        import numpy as np
        self._chk(logi, torch.float32, "logi")
        n = logi.shape[0]
        hc = np.ascontiguousarray(counts, dtype=np.int32)
        assert hc.shape == (n,)
        logic = torch.zeros((n, L.PT_TSR_MAX_CELLS, 4), dtype=torch.float32, device=self._tdev)
        stacked = torch.zeros((n, L.PT_TSR_MAX_CELLS, 4), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_tsr_process(self._h, _ptr(logi), _ptr(dets), hc.ctypes.data, n, int(use_2dpe), _ptr(logic),
                                        _ptr(stacked), self._stream()), "pt_tsr_process")
        return logic, stacked

    def det_bitmap(self, prob: torch.Tensor, thresh: float, use_dilation: bool = False) -> torch.Tensor:
        self._chk(prob, torch.float32, "prob")
        n, H, W = prob.shape
        bm = torch.empty((n, H, W // 32), dtype=torch.int32, device=self._tdev)
        L.check(self.lib.pt_det_bitmap(self._h, _ptr(prob), n, H, W, float(thresh), int(use_dilation), _ptr(bm),
                                       self._stream()), "pt_det_bitmap")
        return bm

    def det_box_scores(self, prob: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
        """boxes f32 [nb, 9] = (page, x0,y0,...,x3,y3) -> scores f32 [nb]."""
        self._chk(prob, torch.float32, "prob")
        self._chk(boxes, torch.float32, "boxes")
        n, H, W = prob.shape
        nb = boxes.shape[0]
        scores = torch.empty((nb,), dtype=torch.float32, device=self._tdev)
        if nb:
            L.check(self.lib.pt_det_box_scores(self._h, _ptr(prob), n, H, W, _ptr(boxes), nb, _ptr(scores),
                                               self._stream()), "pt_det_box_scores")
        return scores

    def op_det_poly_scores(self, prob: torch.Tensor, points: torch.Tensor, offsets: torch.Tensor, pages: torch.Tensor, h_offsets, h_pages,
                           sums: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, scores: Optional[torch.Tensor] = None,
                           work: Optional[torch.Tensor] = None) -> torch.Tensor:
        """box_score_slow for nb contours in one call (pt_op_det_poly_scores, csrc/det_poly_score.hip): the mean of prob f32 [n, H, W] over the
        cv2.fillPoly mask of each contour inside its clipped bounding rectangle.  points int32 [np, 2] (x, y), offsets int32 [nb + 1], pages int32
        [nb] on the device; h_offsets / h_pages: their host copies (numpy), which every limit is checked on (PtError, nothing launched, nothing
        written).  -> scores f32 [nb] = float32(sum / count), 0 for an empty mask.  sums f64 [nb] / counts int32 [nb]: buffers that also receive the
        sum and the pixel count; scores / work (uint8, nb * PT_DET_POLY_WORK_BYTES): buffers to use instead of allocating."""
        self._chk(prob, torch.float32, "prob")
        for t, name in ((points, "points"), (offsets, "offsets"), (pages, "pages")):
            self._chk(t, torch.int32, name)
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.int32).reshape(-1)
        h_pages = np.ascontiguousarray(h_pages, dtype=np.int32).reshape(-1)
        n, H, W = prob.shape
        nb = h_pages.shape[0]
        if h_offsets.shape[0] != nb + 1 or offsets.numel() < nb + 1 or pages.numel() < nb or points.numel() % 2:
            raise ValueError(f"op_det_poly_scores: offsets {tuple(offsets.shape)} / host {h_offsets.shape} and pages {tuple(pages.shape)} / host "
                             f"{h_pages.shape} do not fit, or points {tuple(points.shape)} is not [np, 2]")
        if scores is None:
            scores = torch.empty((nb,), dtype=torch.float32, device=self._tdev)
        if work is None:
            work = torch.empty((max(nb, 1) * L.PT_DET_POLY_WORK_BYTES,), dtype=torch.uint8, device=self._tdev)
        self._chk(scores, torch.float32, "scores")
        self._chk(work, torch.uint8, "work")
        if sums is not None:
            self._chk(sums, torch.float64, "sums")
        if counts is not None:
            self._chk(counts, torch.int32, "counts")
        if scores.numel() < nb or (sums is not None and sums.numel() < nb) or (counts is not None and counts.numel() < nb):
            raise ValueError("op_det_poly_scores: output buffers too small")
        L.check(self.lib.pt_op_det_poly_scores(_ptr(prob), n, H, W, _ptr(points), points.numel() // 2, _ptr(offsets), h_offsets.ctypes.data_as(C.c_void_p),
                                               _ptr(pages), h_pages.ctypes.data_as(C.c_void_p), nb, _ptr(scores), _ptr(sums), _ptr(counts), _ptr(work),
                                               work.numel(), self._stream()), "pt_op_det_poly_scores")
        return scores[:nb]

    # ---- image-page straightening (csrc/page_pre.hip) ---------------------------------------------
    def page_line_mask(self, pages: torch.Tensor) -> torch.Tensor:
        """uint8 RGB [n, h, w, 3] -> the deskew's opened horizontal-line mask, bit-packed: int64 [n, h, (w + 63) // 64] (bit b of word q =
        column 64 q + b)"""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        bits = torch.empty((n, h, (w + 63) // 64), dtype=torch.int64, device=self._tdev)
        L.check(self.lib.pt_page_line_mask(_ptr(pages), n, h, w, _ptr(bits), self._stream()), "pt_page_line_mask")
        return bits

    def page_warp_cubic(self, pages: torch.Tensor, minv: np.ndarray, idx: Sequence[int]) -> torch.Tensor:
        """cv2.warpAffine(INTER_CUBIC, BORDER_REPLICATE) of pages[idx[j]] by the INVERSE map minv[j] (float64 [m, 6]) -> uint8 [m, h, w, 3]"""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        mi = np.ascontiguousarray(minv, dtype=np.float64).reshape(-1, 6)
        ix = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        assert len(mi) == len(ix) and len(ix) and ((ix >= 0) & (ix < n)).all(), "page_warp_cubic: bad page indices"
        out = torch.empty((len(ix), h, w, 3), dtype=torch.uint8, device=self._tdev)
        d_m, d_i = _upload(mi, self._tdev), _upload(ix, self._tdev)
        L.check(self.lib.pt_page_warp_cubic(_ptr(pages), n, h, w, _ptr(d_m), _ptr(d_i), len(ix), _ptr(out), self._stream()),
                "pt_page_warp_cubic")
        d_m.record_stream(torch.cuda.current_stream(self._tdev))
        d_i.record_stream(torch.cuda.current_stream(self._tdev))
        return out

    def page_quarter_turn(self, pages: torch.Tensor, code: int) -> torch.Tensor:
        """cv2.rotate(page, code) of every page: L.PT_ROTATE_90_CLOCKWISE / _180 / _90_COUNTERCLOCKWISE"""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        shape = (n, h, w, 3) if code == L.PT_ROTATE_180 else (n, w, h, 3)
        out = torch.empty(shape, dtype=torch.uint8, device=self._tdev)
        L.check(self.lib.pt_page_quarter_turn(_ptr(pages), n, h, w, int(code), _ptr(out), self._stream()), "pt_page_quarter_turn")
        return out

    # ---- image classification (PP-LCNet) ------------------------------------------------------------
    def _cls_batch(self, images: Sequence[np.ndarray]):
        """RGB uint8 images of any sizes -> (flat device bytes, device pt_cls_image records, max_h, max_w)"""
        desc = np.zeros(len(images), dtype=CLS_IMAGE_DTYPE)
        off = 0
        parts = []
        for k, im in enumerate(images):
            im = np.ascontiguousarray(im[:, :, :3], dtype=np.uint8)
            desc[k] = (off, im.shape[0], im.shape[1])
            off += im.size
            parts.append(im.reshape(-1))
        flat = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        return (_upload(flat, self._tdev), _upload(desc.view(np.uint8).reshape(-1), self._tdev),
                int(desc["h"].max()), int(desc["w"].max()))

    def cls_preprocess(self, images: Sequence[np.ndarray], out_hw) -> torch.Tensor:
        """-> bf16 NHWC4 [n, out_h, out_w, 4] (8 channels in BF16X3 mode)"""
        n = len(images)
        base, desc, mh, mw = self._cls_batch(images)
        ch = 8 if self.split else 4
        out = torch.empty((n, out_hw[0], out_hw[1], ch), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_cls_preprocess(self._h, _ptr(base), _ptr(desc), n, mh, mw, out_hw[0], out_hw[1], _ptr(out),
                                           self._stream()), "pt_cls_preprocess")
        return out

    def cls_forward_net(self, x: torch.Tensor, slot: int = 0, textline: bool = False) -> torch.Tensor:
        """x bf16 NHWC4 [n,H,W,4|8] -> logits f32 [n, class_num] (device)"""
        self._chk(x, self.act_dtype, "x")
        n, H, W, _ = x.shape
        logits = torch.empty((n, L.PT_CLS_MAX_CLASSES), dtype=torch.float32, device=self._tdev)
        nc = C.c_int(0)
        L.check(self.lib.pt_cls_forward_net(self._h, slot, _ptr(x), n, H, W, int(textline), _ptr(logits), C.byref(nc),
                                            self._stream()), "pt_cls_forward_net")
        return logits[:, :nc.value]

    def cls_forward(self, images: Sequence[np.ndarray], out_hw, slot: int = 0, textline: bool = False) -> torch.Tensor:
        """RGB uint8 images (any sizes, host) -> logits f32 [n, class_num] (device): resize + normalise + PP-LCNet"""
        n = len(images)
        base, desc, mh, mw = self._cls_batch(images)
        logits = torch.empty((n, L.PT_CLS_MAX_CLASSES), dtype=torch.float32, device=self._tdev)
        nc = C.c_int(0)
        L.check(self.lib.pt_cls_forward(self._h, slot, _ptr(base), _ptr(desc), n, mh, mw, out_hw[0], out_hw[1], int(textline),
                                        _ptr(logits), C.byref(nc), self._stream()), "pt_cls_forward")
        return logits[:, :nc.value]

    def cls_forward_pages(self, pages: torch.Tensor, out_hw, slot: int = 0, textline: bool = False) -> torch.Tensor:
        """pages uint8 [n,h,w,3] resident on the device -> logits f32 [n, class_num]"""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        desc = np.zeros(n, dtype=CLS_IMAGE_DTYPE)
        desc["offset"] = np.arange(n, dtype=np.int64) * (h * w * 3)
        desc["h"], desc["w"] = h, w
        d = _upload(desc.view(np.uint8).reshape(-1), self._tdev)
        logits = torch.empty((n, L.PT_CLS_MAX_CLASSES), dtype=torch.float32, device=self._tdev)
        nc = C.c_int(0)
        L.check(self.lib.pt_cls_forward(self._h, slot, _ptr(pages), _ptr(d), n, h, w, out_hw[0], out_hw[1], int(textline),
                                        _ptr(logits), C.byref(nc), self._stream()), "pt_cls_forward")
        return logits[:, :nc.value]

    def cls_forward_lines(self, pages: torch.Tensor, lines: np.ndarray, out_hw, slot: int = 0, textline: bool = True):
        """text lines (REC_LINE_DTYPE records) cut from resident pages -> logits f32 [n_lines, class_num]"""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        nl = len(lines)
        logits = torch.empty((nl, L.PT_CLS_MAX_CLASSES), dtype=torch.float32, device=self._tdev)
        nc = C.c_int(0)
        if nl:
            d, px = self._lines_to_device(lines)
            mh, mw = max(1, int(lines["crop_h"].max())), max(1, int(lines["crop_w"].max()))
            L.check(self.lib.pt_cls_forward_lines(self._h, slot, _ptr(pages), n, h, w, _ptr(d), px.ctypes.data_as(C.c_void_p), nl,
                                                  mh, mw, out_hw[0], out_hw[1], int(textline), _ptr(logits), C.byref(nc),
                                                  self._stream()), "pt_cls_forward_lines")
        return logits[:, :nc.value] if nl else logits[:, :0]

    def cls_forward_lines_direct(self, pages: torch.Tensor, lines: np.ndarray, out_hw, slot: int = 0, textline: bool = True):
        """cls_forward_lines() without the recogniser's crop buffers (pt_cls_forward_lines_direct): bit-identical logits, and the call may be in
        flight beside rec_forward*() and the layout net on other streams"""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        nl = len(lines)
        logits = torch.empty((nl, L.PT_CLS_MAX_CLASSES), dtype=torch.float32, device=self._tdev)
        nc = C.c_int(0)
        if nl:
            d, _ = self._lines_to_device(lines)
            mh, mw = max(1, int(lines["crop_h"].max())), max(1, int(lines["crop_w"].max()))
            L.check(self.lib.pt_cls_forward_lines_direct(self._h, slot, _ptr(pages), n, h, w, _ptr(d), nl, mh, mw, out_hw[0], out_hw[1],
                                                         int(textline), _ptr(logits), C.byref(nc), self._stream()),
                    "pt_cls_forward_lines_direct")
        return logits[:, :nc.value] if nl else logits[:, :0]

    # ---- recognition ------------------------------------------------------------------------------
    def _lines_to_device(self, lines: np.ndarray):
        """structured array (REC_LINE_DTYPE) -> (uint8 device tensor holding the pt_rec_line records, host crop px)."""
        lines = np.ascontiguousarray(lines)
        assert lines.dtype == REC_LINE_DTYPE
        px = (lines["crop_w"].astype(np.int64) * lines["crop_h"].astype(np.int64)).clip(min=0)
        d = _upload(lines.view(np.uint8).reshape(-1), self._tdev)
        return d, np.ascontiguousarray(px)

    def rec_forward(self, pages: torch.Tensor, lines: np.ndarray, want_maxlogit: bool = True):
        """pages uint8 [n,h,w,3] on the GPU, lines: REC_LINE_DTYPE records -> (ids int32 [L,160], maxlogit f32 [L,160])."""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        nl = len(lines)
        ids = torch.empty((nl, L.PT_REC_T), dtype=torch.int32, device=self._tdev)
        mx = torch.empty((nl, L.PT_REC_T), dtype=torch.float32, device=self._tdev) if want_maxlogit else None
        if nl:
            d, px = self._lines_to_device(lines)
            L.check(self.lib.pt_rec_forward(self._h, _ptr(pages), n, h, w, _ptr(d), px.ctypes.data_as(C.c_void_p), nl,
                                            _ptr(ids), _ptr(mx), self._stream()), "pt_rec_forward")
        return ids, mx

    def rec_forward_crops(self, crops: Sequence[np.ndarray]):
        """already-cropped RGB uint8 images (any sizes) -> (ids int32 [L,160], maxlogit f32 [L,160])."""
        nl = len(crops)
        lines = np.zeros(nl, dtype=REC_LINE_DTYPE)
        lines["crop_w"] = [c.shape[1] for c in crops]
        lines["crop_h"] = [c.shape[0] for c in crops]
        flat = np.concatenate([np.ascontiguousarray(c[:, :, :3], dtype=np.uint8).reshape(-1) for c in crops]) if nl else \
            np.zeros(0, np.uint8)
        ids = torch.empty((nl, L.PT_REC_T), dtype=torch.int32, device=self._tdev)
        mx = torch.empty((nl, L.PT_REC_T), dtype=torch.float32, device=self._tdev)
        if nl:
            d, px = self._lines_to_device(lines)
            dc = torch.from_numpy(flat).to(self._tdev)
            L.check(self.lib.pt_rec_forward_crops(self._h, _ptr(dc), _ptr(d), px.ctypes.data_as(C.c_void_p), nl, _ptr(ids),
                                                  _ptr(mx), self._stream()), "pt_rec_forward_crops")
        return ids, mx

    def rec_pp_preprocess(self, pages: Optional[torch.Tensor], lines: np.ndarray, items: np.ndarray, total_floats: int,
                          img_h: int = 48, crops_flat: Optional[np.ndarray] = None) -> torch.Tensor:
        """PPOcrRecPreProcessor on the device: ``items`` (REC_PP_ITEM_DTYPE, the host's width-sorted plan) -> one flat fp32
        buffer holding every mini-batch's [b, 3, img_h, img_w] array.  Lines are cut from resident ``pages`` or, with
        ``crops_flat`` (concatenated uint8 crops), are already cropped."""
        assert items.dtype == REC_PP_ITEM_DTYPE and len(items) and len(lines)
        out = torch.empty((int(total_floats),), dtype=torch.float32, device=self._tdev)
        d, px = self._lines_to_device(lines)
        di = _upload(np.ascontiguousarray(items).view(np.uint8).reshape(-1), self._tdev)
        max_w = int(items["img_w"].max())
        if crops_flat is None:
            self._chk(pages, torch.uint8, "pages")
            n, h, w, _ = pages.shape
            L.check(self.lib.pt_rec_pp_preprocess(self._h, _ptr(pages), n, h, w, _ptr(d), px.ctypes.data_as(C.c_void_p), len(lines),
                                                  _ptr(di), len(items), img_h, max_w, _ptr(out), self._stream()),
                    "pt_rec_pp_preprocess")
        else:
            dc = torch.from_numpy(np.ascontiguousarray(crops_flat)).to(self._tdev)
            L.check(self.lib.pt_rec_pp_preprocess_crops(self._h, _ptr(dc), _ptr(d), px.ctypes.data_as(C.c_void_p), len(lines),
                                                        _ptr(di), len(items), img_h, max_w, _ptr(out), self._stream()),
                    "pt_rec_pp_preprocess_crops")
        return out

    def rec_preprocess(self, pages: torch.Tensor, lines: np.ndarray) -> torch.Tensor:
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        nl = len(lines)
        shape = (nl, L.PT_REC_H, L.PT_REC_W, 2) if self.split else (nl, L.PT_REC_H, L.PT_REC_W)
        gray = torch.empty(shape, dtype=self.act_dtype, device=self._tdev)
        d, px = self._lines_to_device(lines)
        L.check(self.lib.pt_rec_preprocess(self._h, _ptr(pages), n, h, w, _ptr(d), px.ctypes.data_as(C.c_void_p), nl,
                                           _ptr(gray), self._stream()), "pt_rec_preprocess")
        return gray

    def rec_forward_net(self, gray: torch.Tensor):
        """gray bf16 [n,32,640] (BF16X3: [n,32,640,2]) -> (ids int32 [n,160], maxlogit f32 [n,160])."""
        self._chk(gray, self.act_dtype, "gray")
        n = gray.shape[0]
        ids = torch.empty((n, L.PT_REC_T), dtype=torch.int32, device=self._tdev)
        mx = torch.empty((n, L.PT_REC_T), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_rec_forward_net(self._h, _ptr(gray), n, _ptr(ids), _ptr(mx), self._stream()),
                "pt_rec_forward_net")
        return ids, mx

    # ---- ConvNextViT recogniser ---------------------------------------------------------------
    def _crops_to_device(self, crops: Sequence[np.ndarray]):
        nl = len(crops)
        lines = np.zeros(nl, dtype=REC_LINE_DTYPE)
        lines["crop_w"] = [c.shape[1] for c in crops]
        lines["crop_h"] = [c.shape[0] for c in crops]
        flat = np.concatenate([np.ascontiguousarray(c[:, :, :3], dtype=np.uint8).reshape(-1) for c in crops])
        d, px = self._lines_to_device(lines)
        return d, px, torch.from_numpy(flat).to(self._tdev), self._crop_wh(lines)

    @staticmethod
    def _crop_wh(lines: np.ndarray) -> np.ndarray:
        """host int32 [n, 2] = (crop_w, crop_h): lets the engine share the all-padding chunks of short lines"""
        return np.ascontiguousarray(np.stack([lines["crop_w"], lines["crop_h"]], 1).astype(np.int32))

    def rec_cvit_forward(self, pages: torch.Tensor, lines: np.ndarray):
        """pages uint8 [n,h,w,3] on the GPU, lines: REC_LINE_DTYPE records -> (ids int32 [L,201], maxlogit f32 [L,201])."""
        self._chk(pages, torch.uint8, "pages")
        n, h, w, _ = pages.shape
        nl = len(lines)
        ids = torch.empty((nl, L.PT_CVIT_T), dtype=torch.int32, device=self._tdev)
        mx = torch.empty((nl, L.PT_CVIT_T), dtype=torch.float32, device=self._tdev)
        if nl:
            d, px = self._lines_to_device(lines)
            wh = self._crop_wh(lines)
            L.check(self.lib.pt_rec_cvit_forward(self._h, _ptr(pages), n, h, w, _ptr(d), px.ctypes.data_as(C.c_void_p),
                                                 wh.ctypes.data_as(C.c_void_p), nl, _ptr(ids), _ptr(mx), self._stream()),
                    "pt_rec_cvit_forward")
        return ids, mx

    def rec_cvit_forward_crops(self, crops: Sequence[np.ndarray]):
        """already-cropped RGB uint8 images (any sizes) -> (ids int32 [L,201], maxlogit f32 [L,201])."""
        nl = len(crops)
        ids = torch.empty((nl, L.PT_CVIT_T), dtype=torch.int32, device=self._tdev)
        mx = torch.empty((nl, L.PT_CVIT_T), dtype=torch.float32, device=self._tdev)
        if nl:
            d, px, dc, wh = self._crops_to_device(crops)
            L.check(self.lib.pt_rec_cvit_forward_crops(self._h, _ptr(dc), _ptr(d), px.ctypes.data_as(C.c_void_p),
                                                       wh.ctypes.data_as(C.c_void_p), nl, _ptr(ids), _ptr(mx), self._stream()),
                    "pt_rec_cvit_forward_crops")
        return ids, mx

    def rec_cvit_preprocess_crops(self, crops: Sequence[np.ndarray]) -> torch.Tensor:
        """keep-ratio resize to 32 x 804 + gray of already-cropped lines -> fp32 [L,32,804]."""
        nl = len(crops)
        gray = torch.empty((nl, L.PT_REC_H, L.PT_CVIT_W), dtype=torch.float32, device=self._tdev)
        d, px, dc, _ = self._crops_to_device(crops)
        L.check(self.lib.pt_rec_cvit_preprocess_crops(self._h, _ptr(dc), _ptr(d), px.ctypes.data_as(C.c_void_p), nl, _ptr(gray),
                                                      self._stream()), "pt_rec_cvit_preprocess_crops")
        return gray

    def rec_cvit_forward_net(self, gray: torch.Tensor, text_w: Optional[Sequence[int]] = None):
        """gray fp32 [3n,32,300] (chunks) or [n,32,804] (lines) -> (ids int32 [n,201], maxlogit f32 [n,201]).
        ``text_w`` (per line): columns >= text_w[i] are zero padding -- all-padding chunks are then computed once and shared."""
        self._chk(gray, torch.float32, "gray")
        assert gray.dim() == 3 and gray.shape[1] == L.PT_REC_H and gray.shape[2] in (L.PT_CVIT_CHUNK_W, L.PT_CVIT_W)
        layout = 1 if gray.shape[2] == L.PT_CVIT_W else 0
        assert layout == 1 or gray.shape[0] % 3 == 0, "three chunks per line"
        n = gray.shape[0] if layout else gray.shape[0] // 3
        ids = torch.empty((n, L.PT_CVIT_T), dtype=torch.int32, device=self._tdev)
        mx = torch.empty((n, L.PT_CVIT_T), dtype=torch.float32, device=self._tdev)
        tw = None if text_w is None else np.ascontiguousarray(np.asarray(text_w, dtype=np.int32))
        assert tw is None or len(tw) == n
        L.check(self.lib.pt_rec_cvit_forward_net(self._h, _ptr(gray), layout, n, None if tw is None else tw.ctypes.data_as(C.c_void_p),
                                                 _ptr(ids), _ptr(mx), self._stream()), "pt_rec_cvit_forward_net")
        return ids, mx

    def mtl_backbone_forward(self, x: torch.Tensor) -> torch.Tensor:
        """MtlTabNet backbone (TableResNetExtra): x fp32 [n, 3, H, W] (normalised image, on the GPU) -> the last feature map
        fp32 [n, 512, H/8, W/8].  torch only moves data here (NCHW fp32 -> padded NHWC bf16, hi/lo in BF16X3)."""
        self._chk(x, torch.float32, "x")
        n, c, h, w = x.shape
        assert c == 3 and h % 8 == 0 and w % 8 == 0
        xp = torch.zeros((n, h, w, 32), dtype=torch.float32, device=self._tdev)
        xp[..., :3] = x.permute(0, 2, 3, 1)
        hi = xp.to(self.act_dtype)
        if self.split:
            hi = torch.cat([hi, (xp - hi.float()).to(self.act_dtype)], -1)
        hi = hi.contiguous()
        f3 = torch.empty((n, h // 8, w // 8, 512), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_tsr_mtl_backbone_net(self._h, _ptr(hi), n, h, w, _ptr(f3), self._stream()), "pt_tsr_mtl_backbone_net")
        return f3.permute(0, 3, 1, 2)

    def mtl_backbone_features(self, xin: torch.Tensor, size_hw: Tuple[int, int]) -> torch.Tensor:
        """pre-processed input bf16 [n, H, W, 32 (x 2 in BF16X3)] (mtl_preprocess) -> f3 fp32 [n, H/8 * W/8, 512] (NHWC, flattened)"""
        n = xin.shape[0]
        h, w = size_hw
        f3 = torch.empty((n, (h // 8) * (w // 8), 512), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_tsr_mtl_backbone_net(self._h, _ptr(xin), n, h, w, _ptr(f3), self._stream()), "pt_tsr_mtl_backbone_net")
        return f3

    def mtl_preprocess(self, pages: torch.Tensor, tables: np.ndarray, size: int = 480) -> torch.Tensor:
        """MtlTabNet test pipeline (TableResize keep-ratio long side `size`, TablePad, to_tensor, normalise) of table crops cut from
        resident pages.  pages uint8 [n_pages, h, w, 3]; tables: TSR_TABLE_DTYPE records (page, x0, y0, crop_w, crop_h).
        -> bf16 [n, size, size, 32] ([hi 32 | lo 32] in BF16X3), the backbone's input."""
        self._chk(pages, torch.uint8, "pages")
        assert tables.dtype == TSR_TABLE_DTYPE
        n = len(tables)
        d_tab = _upload(tables.view(np.uint8).reshape(-1), self._tdev)
        m = 2 if self.split else 1
        out = torch.empty((n, size, size, 32 * m), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_tsr_mtl_preprocess(self._h, _ptr(pages), pages.shape[0], pages.shape[1], pages.shape[2], _ptr(d_tab), n, size,
                                               _ptr(out), self._stream()), "pt_tsr_mtl_preprocess")
        return out

    def mtl_resized_size(self, crop_w: int, crop_h: int, size: int = 480) -> Tuple[int, int]:
        ow, oh = C.c_int(), C.c_int()
        self.lib.pt_tsr_mtl_resized_size(int(crop_w), int(crop_h), int(size), C.byref(ow), C.byref(oh))
        return ow.value, oh.value

    def mtl_decoder_config(self) -> dict:
        v = (C.c_int * 13)()
        L.check(self.lib.pt_tsr_mtl_decoder_config(self._h, v), "pt_tsr_mtl_decoder_config")
        k = ("num_classes", "num_classes_cell", "sos", "eos", "pad", "max_len", "sos_cell", "eos_cell", "pad_cell", "max_len_cell", "tag0", "tag1", "d_ff_pad")
        return dict(zip(k, [int(x) for x in v]))

    def mtl_decode(self, f3: torch.Tensor, want_cell_logits: bool = False, force_redecode: bool = False) -> dict:
        """The three MtlTabNet decoders for a batch of tables (pt_tsr_mtl_structure + pt_tsr_mtl_cells).  f3 fp32 [n, hw, 512].
        -> dict: tag_logits fp32 [n, T, classes], boxes fp32 [n, T, 4] (device), lens [n], cell_counts [n], cell_steps [n] (numpy),
        cell_ids int32 / cell_prob fp32 [total cells, Tc] (device; cells ordered by table, then position), cell_logits or None."""
        self._chk(f3, torch.float32, "f3")
        n, hw, d = f3.shape
        assert d == 512
        cfg = self.mtl_decoder_config()
        T, Tc = cfg["max_len"] + 1, cfg["max_len_cell"] + 1
        tag = torch.zeros((n, T, cfg["num_classes"]), dtype=torch.float32, device=self._tdev)
        box = torch.zeros((n, T, 4), dtype=torch.float32, device=self._tdev)
        lens = np.zeros(n, np.int32)
        counts = np.zeros(n, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        L.check(self.lib.pt_tsr_mtl_structure(self._h, _ptr(f3), n, hw, _ptr(tag), _ptr(box), ip(lens), ip(counts), 1 if force_redecode else 0,
                                              self._stream()), "pt_tsr_mtl_structure")
        total = int(counts.sum())
        steps = np.zeros(n, np.int32)
        ids = torch.zeros((max(total, 1), Tc), dtype=torch.int32, device=self._tdev)
        prob = torch.zeros((max(total, 1), Tc), dtype=torch.float32, device=self._tdev)
        logits = torch.zeros((max(total, 1), Tc, cfg["num_classes_cell"]), dtype=torch.float32, device=self._tdev) if want_cell_logits else None
        L.check(self.lib.pt_tsr_mtl_cells(self._h, total, _ptr(ids), _ptr(prob), _ptr(logits), ip(steps), 1 if force_redecode else 0, self._stream()),
                "pt_tsr_mtl_cells")
        return dict(tag_logits=tag, boxes=box, lens=lens, cell_counts=counts, cell_steps=steps, cell_ids=ids[:total], cell_prob=prob[:total],
                    cell_logits=None if logits is None else logits[:total], cfg=cfg)

    def op_conv2d(self, x: torch.Tensor, w_tiled: torch.Tensor, bias: torch.Tensor, ks: int, stride: int = 1,
                  relu: bool = False, res: Optional[torch.Tensor] = None, res_mode: int = 0, rep: int = 1,
                  shuffle_cout: int = 0, out: Optional[torch.Tensor] = None, out_coff: int = 0,
                  split: int = 0) -> torch.Tensor:
        """Single conv on the MFMA kernel.  x bf16 [B,H,W,Cin]; w_tiled int16/bf16 bits; bias f32 [N].  split: 0 plain bf16, 1 (hi | lo)
        tensors with the three-pass tiles, 2 the same tensors with the two-pass fp16 tiles (weights.tile_conv_weight_f16x2)."""
        self._chk(x, self.act_dtype, "x")
        self._chk(bias, torch.float32, "bias")
        B, H, W, Cin = x.shape
        m = 2 if split else 1
        Cin //= m
        N = bias.numel()
        pad = ks // 2
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        if out is None:
            if shuffle_cout:
                out = torch.empty((B, 2 * Ho, 2 * Wo, shuffle_cout * m), dtype=self.act_dtype, device=self._tdev)
            else:
                out = torch.empty((B, Ho * rep, Wo * rep, N * m), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_conv2d(self._h, _ptr(x), B, H, W, Cin, _ptr(w_tiled), _ptr(bias), N, ks, stride,
                                      _ptr(out), out.shape[-1], out_coff, rep, shuffle_cout, _ptr(res), res_mode,
                                      int(relu), int(split), out.shape[-1] // 2, self._stream()), "pt_op_conv2d")      # relu: bool, or the epilogue's activation code (0 none, 1 ReLU, 2 hardswish)
        return out

    def op_conv1x1_ex(self, x: torch.Tensor, w_tiled: torch.Tensor, bias: torch.Tensor, relu: int = 0, out_f32: bool = False,
                      n_valid: int = 0, res_f32: Optional[torch.Tensor] = None, ylimit: Optional[torch.Tensor] = None) -> torch.Tensor:
        """1x1 stride-1 conv with the network launchers' extra epilogues (pt_op_conv1x1_ex): fp32 output, n_valid stored channels, fp32
        residual, a device row limit (int32 [1]: output rows >= ylimit[0] are not computed and keep what `out` held, zeros here)."""
        self._chk(x, self.act_dtype, "x")
        self._chk(bias, torch.float32, "bias")
        B, H, W, Cin = x.shape
        N = bias.numel()
        cs = n_valid or N
        out = torch.zeros((B, H, W, cs), dtype=torch.float32 if out_f32 else self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_conv1x1_ex(self._h, _ptr(x), B, H, W, Cin, _ptr(w_tiled), _ptr(bias), N, None if out_f32 else _ptr(out),
                                          _ptr(out) if out_f32 else None, cs, n_valid, _ptr(res_f32), int(relu), _ptr(ylimit),
                                          self._stream()), "pt_op_conv1x1_ex")
        return out

    def op_dcn(self, x: torch.Tensor, om: torch.Tensor, w_tiled: torch.Tensor, bias: torch.Tensor, relu: bool = True, split: int = 0) -> torch.Tensor:
        """Fused modulated deformable 3x3 convolution (lore/dcnv2.py:71-86) as a single operator.  x bf16 [B,H,W,C] ([hi | lo] when split),
        om fp32 [B,H,W,32] (18 offsets, 9 mask logits, 5 unused), w_tiled = the [N, 9C, 1, 1] weight tiled as a 1x1 conv, bias fp32 [N]."""
        self._chk(x, self.act_dtype, "x")
        self._chk(om, torch.float32, "om")
        self._chk(bias, torch.float32, "bias")
        B, H, W, Cc = x.shape
        m = 2 if split else 1
        Cc //= m
        if tuple(om.shape) != (B, H, W, 32):
            raise ValueError(f"op_dcn: om must be [B,H,W,32], got {tuple(om.shape)}")
        N = bias.numel()
        out = torch.empty((B, H, W, N * m), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_dcn(self._h, _ptr(x), _ptr(om), B, H, W, Cc, _ptr(w_tiled), _ptr(bias), N, _ptr(out), int(relu), int(split),
                                   self._stream()), "pt_op_dcn")
        return out

    def op_dwconvt_up_add(self, x: torch.Tensor, w_taps: torch.Tensor, add: Optional[torch.Tensor], f: int, split: int = 0) -> torch.Tensor:
        """IDAUp's up-sampler (pt_op_dwconvt_up_add): depthwise ConvTranspose2d(C, C, 2f, stride f, padding f/2) of x [B,h,w,C] (+ add [B,hf,wf,C]);
        w_taps fp32 [(2f)^2, C]."""
        self._chk(x, self.act_dtype, "x")
        self._chk(w_taps, torch.float32, "w_taps")
        B, h, w, Cc = x.shape
        if add is not None:
            self._chk(add, self.act_dtype, "add")
            if tuple(add.shape) != (B, h * f, w * f, Cc):
                raise ValueError(f"op_dwconvt_up_add: add must be {(B, h * f, w * f, Cc)}, got {tuple(add.shape)}")
        out = torch.empty((B, h * f, w * f, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_dwconvt_up_add(self._h, _ptr(x), _ptr(w_taps), _ptr(add), _ptr(out), B, h, w, Cc // 2 if split else Cc, int(f),
                                              int(split), self._stream()), "pt_op_dwconvt_up_add")
        return out

    def op_dcn_up_add(self, x: torch.Tensor, om: torch.Tensor, w_tiled: torch.Tensor, bias: torch.Tensor, up_in: torch.Tensor, up_taps: torch.Tensor,
                      f: int, relu: bool = True, split: int = 0) -> torch.Tensor:
        """op_dcn followed by op_dwconvt_up_add(up_in, up_taps, add=that output, f) as one launch (pt_op_dcn_up_add), bit for bit."""
        self._chk(x, self.act_dtype, "x")
        self._chk(om, torch.float32, "om")
        self._chk(bias, torch.float32, "bias")
        self._chk(up_in, self.act_dtype, "up_in")
        self._chk(up_taps, torch.float32, "up_taps")
        B, H, W, Cc = x.shape
        if tuple(om.shape) != (B, H, W, 32):
            raise ValueError(f"op_dcn_up_add: om must be [B,H,W,32], got {tuple(om.shape)}")
        N = bias.numel()
        if up_in.dim() != 4 or up_in.shape[0] != B or up_in.shape[3] != N:
            raise ValueError(f"op_dcn_up_add: up_in must be [{B},h,w,{N}], got {tuple(up_in.shape)}")
        out = torch.empty((B, H, W, N), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_dcn_up_add(self._h, _ptr(x), _ptr(om), B, H, W, Cc // 2 if split else Cc, _ptr(w_tiled), _ptr(bias), N, _ptr(out), int(relu),
                                          int(split), _ptr(up_in), up_in.shape[1], up_in.shape[2], _ptr(up_taps), int(f), self._stream()),
                "pt_op_dcn_up_add")
        return out

    def op_lore_hm_head(self, feat: torch.Tensor, w1_tiled: torch.Tensor, b1: torch.Tensor, w2_tiled: torch.Tensor, b2: torch.Tensor,
                        fused: bool, want_sig: bool = False, want_sig_ref: bool = False, logits_fill: float = 0.0):
        """Lore's heat-map head (pt_op_lore_hm_head) on feat [B,H,W,64]: hm.0 3x3 64 -> 256 + ReLU, hm.2 1x1 256 -> 2 (64 GEMM columns, rows 2.. zero).
        Returns dict(logits fp32 [B,H,W,8] (pre-filled with logits_fill), hid [B,H,W,256] (two launches only), sig [B,H,W,2] (fused, want_sig),
        sig_ref [B,H,W,2] (want_sig_ref: the decode's sigmoid launch on `logits`))."""
        self._chk(feat, self.act_dtype, "feat")
        self._chk(b1, torch.float32, "b1")
        self._chk(b2, torch.float32, "b2")
        B, H, W, Cc = feat.shape
        if Cc != 64 or b1.numel() != 256 or b2.numel() != 64:
            raise ValueError(f"op_lore_hm_head: feat [B,H,W,64], b1 [256], b2 [64]; got {tuple(feat.shape)}, {b1.numel()}, {b2.numel()}")
        if want_sig and not fused:
            raise ValueError("op_lore_hm_head: the two launches have no score output of their own (want_sig_ref)")
        logits = torch.full((B, H, W, 8), float(logits_fill), dtype=torch.float32, device=self._tdev)
        hid = None if fused else torch.empty((B, H, W, 256), dtype=self.act_dtype, device=self._tdev)
        sig = torch.zeros((B, H, W, 2), dtype=torch.float32, device=self._tdev) if want_sig else None
        sig_ref = torch.zeros((B, H, W, 2), dtype=torch.float32, device=self._tdev) if want_sig_ref else None
        L.check(self.lib.pt_op_lore_hm_head(self._h, _ptr(feat), B, H, W, _ptr(w1_tiled), _ptr(b1), _ptr(w2_tiled), _ptr(b2), int(bool(fused)), _ptr(hid),
                                            _ptr(logits), _ptr(sig), _ptr(sig_ref), self._stream()), "pt_op_lore_hm_head")
        return dict(logits=logits, hid=hid, sig=sig, sig_ref=sig_ref)

    # ---- single operators of the generic ONNX executor (pdf_table_amd/onnx_exec.py); bf16 NHWC, C a multiple of 8 -------
    # (split=True: the tolerance mode's (hi | lo) tensors -- the last dimension holds [hi(C) | lo(C)], C = shape[-1] // 2)
    def op_dwconv(self, x: torch.Tensor, w_taps: torch.Tensor, bias: torch.Tensor, k: int, stride: int = 1, act: int = 0, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        self._chk(w_taps, torch.float32, "w_taps")
        self._chk(bias, torch.float32, "bias")
        B, H, W, Cc = x.shape
        pad = k // 2
        out = torch.empty((B, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_dwconv(self._h, _ptr(x), B, H, W, Cc // 2 if split else Cc, _ptr(w_taps), _ptr(bias), k, stride, act, _ptr(out), int(split),
                                      self._stream()), "pt_op_dwconv")
        return out

    def op_add(self, a: torch.Tensor, b: torch.Tensor, split: bool = False) -> torch.Tensor:
        self._chk(a, self.act_dtype, "a")
        self._chk(b, self.act_dtype, "b")
        if a.shape != b.shape:
            raise ValueError(f"op_add: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        out = torch.empty_like(a)
        L.check(self.lib.pt_op_add(self._h, _ptr(a), _ptr(b), _ptr(out), a.numel() // a.shape[-1], a.shape[-1] // 2 if split else a.shape[-1], int(split),
                                   self._stream()), "pt_op_add")
        return out

    def op_maxpool(self, x: torch.Tensor, k: int, stride: int, pad: int, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        B, H, W, Cc = x.shape
        out = torch.empty((B, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_maxpool(self._h, _ptr(x), B, H, W, Cc // 2 if split else Cc, k, stride, pad, _ptr(out), int(split), self._stream()), "pt_op_maxpool")
        return out

    def op_avgpool(self, x: torch.Tensor, k: int, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        B, H, W, Cc = x.shape
        out = torch.empty((B, H // k, W // k, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_avgpool(self._h, _ptr(x), B, H, W, Cc // 2 if split else Cc, k, _ptr(out), int(split), self._stream()), "pt_op_avgpool")
        return out

    # ---- per-axis strides, 1x3 / 3x1 kernels, rectangular pools (csrc/rect_ops.hip, ABI 18: the geometry of text-line recognisers) ----
    def op_conv2d_rect(self, x: torch.Tensor, w_tiled: torch.Tensor, bias: torch.Tensor, kh: int, kw: int, sh: int = 1, sw: int = 1, act: int = 0,
                       out: Optional[torch.Tensor] = None, out_coff: int = 0, split: int = 0) -> torch.Tensor:
        """Dense convolution with kh, kw in {1, 3} and sh, sw in {1, 2} chosen per axis, padding k // 2 per axis.  x [B,H,W,Cin] ([hi | lo] when
        split); w_tiled: weights.tile_conv_weight of [N, Cin, kh, kw] (tile_conv_weight_x3 when split); bias f32 [N]; act 0 none, 1 ReLU,
        2 hardswish.  out / out_coff: write channels [out_coff, out_coff + N) of a wider tensor (the lo half at out.shape[-1] // 2 further)."""
        self._chk(x, self.act_dtype, "x")
        self._chk(bias, torch.float32, "bias")
        B, H, W, Cin = x.shape
        m = 2 if split else 1
        Cin //= m
        N = bias.numel()
        Ho, Wo = (H + 2 * (kh // 2) - kh) // sh + 1, (W + 2 * (kw // 2) - kw) // sw + 1
        if out is None:
            out = torch.empty((B, Ho, Wo, N * m), dtype=self.act_dtype, device=self._tdev)
        else:
            self._chk(out, self.act_dtype, "out")
            if tuple(out.shape[:3]) != (B, Ho, Wo):
                raise ValueError(f"op_conv2d_rect: out must be [{B},{Ho},{Wo},C], got {tuple(out.shape)}")
        L.check(self.lib.pt_op_conv2d_rect(self._h, _ptr(x), B, H, W, Cin, _ptr(w_tiled), _ptr(bias), N, kh, kw, sh, sw, _ptr(out), out.shape[-1],
                                           out_coff, int(act), int(split), out.shape[-1] // 2, self._stream()), "pt_op_conv2d_rect")
        return out

    def op_conv2d_large(self, x: torch.Tensor, w_tiled: torch.Tensor, bias: torch.Tensor, kh: int, kw: int, act: int = 0,
                        out: Optional[torch.Tensor] = None, out_coff: int = 0, split: int = 0) -> torch.Tensor:
        """Dense stride-1 convolution with kh, kw in {1, 3, 5, 7, 9}, at least one of them >= 5, padding k // 2 per axis (csrc/large_conv.hip: the
        9x9 / 7x7 / 5x5 / 7x1 / 1x7 / 5x1 / 1x5 layers of the PP-OCRv4 server detector's neck).  Operands, act, out / out_coff and split as
        op_conv2d_rect."""
        self._chk(x, self.act_dtype, "x")
        self._chk(bias, torch.float32, "bias")
        B, H, W, Cin = x.shape
        m = 2 if split else 1
        Cin //= m
        N = bias.numel()
        if out is None:
            out = torch.empty((B, H, W, N * m), dtype=self.act_dtype, device=self._tdev)
        else:
            self._chk(out, self.act_dtype, "out")
            if tuple(out.shape[:3]) != (B, H, W):
                raise ValueError(f"op_conv2d_large: out must be [{B},{H},{W},C], got {tuple(out.shape)}")
        L.check(self.lib.pt_op_conv2d_large(self._h, _ptr(x), B, H, W, Cin, _ptr(w_tiled), _ptr(bias), N, kh, kw, _ptr(out), out.shape[-1],
                                            out_coff, int(act), int(split), out.shape[-1] // 2, self._stream()), "pt_op_conv2d_large")
        return out

    def op_dwconv_rect(self, x: torch.Tensor, w_taps: torch.Tensor, bias: torch.Tensor, k: int, sh: int, sw: int, act: int = 0, split: bool = False) -> torch.Tensor:
        """depthwise k x k (3 / 5, pad k // 2) with a stride per axis; operands as op_dwconv"""
        self._chk(x, self.act_dtype, "x")
        self._chk(w_taps, torch.float32, "w_taps")
        self._chk(bias, torch.float32, "bias")
        B, H, W, Cc = x.shape
        pad = k // 2
        out = torch.empty((B, (H + 2 * pad - k) // max(sh, 1) + 1, (W + 2 * pad - k) // max(sw, 1) + 1, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_dwconv_rect(self._h, _ptr(x), B, H, W, Cc // 2 if split else Cc, _ptr(w_taps), _ptr(bias), k, sh, sw, act, _ptr(out),
                                           int(split), self._stream()), "pt_op_dwconv_rect")
        return out

    def op_pool_rect(self, x: torch.Tensor, kind: int, kh: int, kw: int, split: bool = False) -> torch.Tensor:
        """kind 0 max / 1 average over kh x kw windows, stride = window, no padding, sizes rounded down: [B,H,W,C] -> [B,H//kh,W//kw,C]"""
        self._chk(x, self.act_dtype, "x")
        B, H, W, Cc = x.shape
        out = torch.empty((B, H // max(kh, 1), W // max(kw, 1), Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_pool_rect(self._h, _ptr(x), B, H, W, Cc // 2 if split else Cc, kind, kh, kw, _ptr(out), int(split), self._stream()),
                "pt_op_pool_rect")
        return out

    def op_affine_act(self, x: torch.Tensor, c: int, s1: Optional[torch.Tensor] = None, b1: Optional[torch.Tensor] = None, act: int = 0,
                      s2: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None, split: bool = False) -> torch.Tensor:
        """y = s2[c] act(s1[c] x + b1[c]) + b2[c] over a 16-bit NHWC map [.., Cpad] (csrc/det_ops.hip); act 0 none / 1 ReLU / 2 hardswish; the vectors are
        fp32 [Cpad] (None: identity); channels c .. Cpad of the result are zeros"""
        self._chk(x, self.act_dtype, "x")
        cp = x.shape[-1] // 2 if split else x.shape[-1]
        vec = []
        for name, v, fill in (("s1", s1, 1.0), ("b1", b1, 0.0), ("s2", s2, 1.0), ("b2", b2, 0.0)):
            if v is None:
                v = torch.full((cp,), fill, dtype=torch.float32, device=self._tdev)
            self._chk(v, torch.float32, name)
            if v.numel() != cp:
                raise ValueError(f"op_affine_act: {name} has {v.numel()} entries, the rows {cp} channels")
            vec.append(v)
        out = torch.empty_like(x)
        L.check(self.lib.pt_op_affine_act(self._h, _ptr(x), x.numel() // x.shape[-1], cp, int(c), _ptr(vec[0]), _ptr(vec[1]), _ptr(vec[2]), _ptr(vec[3]),
                                          int(act), _ptr(out), int(split), self._stream()), "pt_op_affine_act")
        return out

    def op_db_tail(self, x: torch.Tensor, c: int, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, split: bool = False) -> torch.Tensor:
        """the tail of a DB head in one launch (csrc/det_ops.hip): x 16-bit [B, H, W, Cpad] whose first c channels are real, w1 fp32 [c, C1, 2, 2],
        b1 [C1], w2 [C1, 1, 2, 2], b2 [1] -> sigmoid(convT(relu(convT(x)))) as fp32 [B, 4H, 4W, 1]"""
        self._chk(x, self.act_dtype, "x")
        for name, v in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
            self._chk(v, torch.float32, name)
        B, H, W, Cc = x.shape
        cp = Cc // 2 if split else Cc
        c1 = b1.numel()
        if tuple(w1.shape) != (int(c), c1, 2, 2) or tuple(w2.shape) != (c1, 1, 2, 2) or b2.numel() != 1:
            raise ValueError(f"op_db_tail: w1 {tuple(w1.shape)} / b1 [{c1}] / w2 {tuple(w2.shape)} / b2 [{b2.numel()}] for {c} input channels")
        out = torch.empty((B, 4 * H, 4 * W, 1), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_op_db_tail(self._h, _ptr(x), B, H, W, cp, int(c), c1, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(out), int(split),
                                       self._stream()), "pt_op_db_tail")
        return out

    def op_chan_mean(self, x: torch.Tensor, split: bool = False) -> torch.Tensor:
        """GlobalAveragePool: [B, H, W, C] -> [B, 1, 1, C]"""
        self._chk(x, self.act_dtype, "x")
        B, H, W, Cc = x.shape
        ch = Cc // 2 if split else Cc
        scratch = torch.empty((self.lib.pt_op_chan_mean_scratch_floats(B, ch),), dtype=torch.float32, device=self._tdev)
        out = torch.empty((B, 1, 1, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_chan_mean(self._h, _ptr(x), B, H * W, ch, _ptr(scratch), _ptr(out), int(split), self._stream()), "pt_op_chan_mean")
        return out

    def op_scale_channels(self, x: torch.Tensor, gate: torch.Tensor, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        self._chk(gate, self.act_dtype, "gate")
        B, H, W, Cc = x.shape
        if gate.numel() != B * Cc:
            raise ValueError(f"op_scale_channels: gate {tuple(gate.shape)} does not match [{B}, {Cc}]")
        out = torch.empty_like(x)
        L.check(self.lib.pt_op_scale_channels(self._h, _ptr(x), _ptr(gate), B, H * W, Cc // 2 if split else Cc, _ptr(out), int(split), self._stream()),
                "pt_op_scale_channels")
        return out

    def op_act(self, x: torch.Tensor, kind: int, alpha: float = 0.0, beta: float = 0.0, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        out = torch.empty_like(x)
        ch = x.shape[-1] // 2 if split else x.shape[-1]
        L.check(self.lib.pt_op_act(self._h, _ptr(x), x.numel() // (2 if split else 1), kind, float(alpha), float(beta), _ptr(out), ch, int(split),
                                   self._stream()), "pt_op_act")
        return out

    def op_copy_channels(self, src: torch.Tensor, dst: torch.Tensor, n: int, src_coff: int = 0, dst_coff: int = 0):
        """dst[..., dst_coff : dst_coff + n] = src[..., src_coff : src_coff + n] (same pixel count; Concat / Slice / Split over channels)"""
        self._chk(src, self.act_dtype, "src")
        self._chk(dst, self.act_dtype, "dst")
        npix = src.numel() // src.shape[-1]
        assert npix == dst.numel() // dst.shape[-1]
        L.check(self.lib.pt_op_copy_channels(self._h, _ptr(src), npix, src.shape[-1], src_coff, _ptr(dst), dst.shape[-1], dst_coff, n, self._stream()),
                "pt_op_copy_channels")

    def copy_bytes(self, src: torch.Tensor, dst: torch.Tensor):
        """dst <- src (same byte count, contiguous) by a kernel on the current stream; either tensor may live in pinned host memory"""
        nb = src.numel() * src.element_size()
        assert nb == dst.numel() * dst.element_size() and src.is_contiguous() and dst.is_contiguous()
        L.check(self.lib.pt_copy_bytes(self._h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), nb, self._stream()), "pt_copy_bytes")

    def op_upsample(self, x: torch.Tensor, f: int) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        B, H, W, Cc = x.shape
        out = torch.empty((B, H * f, W * f, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_upsample_nearest(self._h, _ptr(x), B, H, W, Cc, int(f), _ptr(out), self._stream()), "pt_op_upsample_nearest")
        return out

    def op_mul(self, a: torch.Tensor, b: torch.Tensor, split: bool = False) -> torch.Tensor:
        self._chk(a, self.act_dtype, "a")
        self._chk(b, self.act_dtype, "b")
        if a.shape != b.shape:
            raise ValueError(f"op_mul: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        out = torch.empty_like(a)
        L.check(self.lib.pt_op_mul(self._h, _ptr(a), _ptr(b), _ptr(out), a.numel() // (2 if split else 1), a.shape[-1] // 2 if split else a.shape[-1], int(split),
                                   self._stream()), "pt_op_mul")
        return out

    def op_layernorm(self, x: torch.Tensor, c: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        self._chk(gamma, torch.float32, "gamma")
        self._chk(beta, torch.float32, "beta")
        out = torch.empty_like(x)
        cp = x.shape[-1] // 2 if split else x.shape[-1]
        L.check(self.lib.pt_op_layernorm(self._h, _ptr(x), x.numel() // x.shape[-1], cp, int(c), _ptr(gamma), _ptr(beta), float(eps), _ptr(out), int(split),
                                         self._stream()), "pt_op_layernorm")
        return out

    def op_softmax(self, x: torch.Tensor, c: int, f32: bool = False, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        rows = x.numel() // x.shape[-1]
        cp = x.shape[-1] // 2 if split else x.shape[-1]
        if f32:
            out = torch.empty(x.shape[:-1] + (int(c),), dtype=torch.float32, device=self._tdev)
            L.check(self.lib.pt_op_softmax(self._h, _ptr(x), rows, cp, int(c), _ptr(out), None, int(split), self._stream()), "pt_op_softmax")
        else:
            out = torch.empty_like(x)
            L.check(self.lib.pt_op_softmax(self._h, _ptr(x), rows, cp, int(c), None, _ptr(out), int(split), self._stream()), "pt_op_softmax")
        return out

    def op_ctc_greedy(self, x: torch.Tensor, c: int, split: bool = False):
        """token rows of 16-bit logits [.., Cp] ([hi | lo] when split), the first c channels real -> (ids int32 [rows], conf float32 [rows]): per
        row the lowest index of the largest logit and its soft-max probability (csrc/ctc_ops.hip: one pass, channels c .. Cp - 1 never read)"""
        self._chk(x, self.act_dtype, "x")
        rows = x.numel() // x.shape[-1]
        cp = x.shape[-1] // 2 if split else x.shape[-1]
        ids = torch.empty((rows,), dtype=torch.int32, device=self._tdev)
        conf = torch.empty((rows,), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_op_ctc_greedy(self._h, _ptr(x), rows, cp, int(c), _ptr(ids), _ptr(conf), int(split), self._stream()), "pt_op_ctc_greedy")
        return ids, conf

    def op_pico_candidates(self, scores, dists, ncls: int, thr_lo: float, max_cands: int = 2048, split: bool = False, out=None):
        """The 2 L outputs of a PicoDet export -> candidate records (pt_op_pico_candidates, csrc/layout_ops.hip).  scores / dists: per level the
        16-bit token rows [B, 1, A_l, Cp] ([hi | lo] when split) of class probabilities (ncls real channels) and distribution logits (32 real
        channels) -> (counts int32 [B], cands float32 [B, max_cands, 48]) on the device: the anchors whose largest class value is > thr_lo as
        (int32 level, int32 anchor, ncls probabilities, 32 logits, zeros), values converted (hi + lo in fp32 when split) and copied only.
        counts reports every candidate, cands holds the first max_cands arrivals; a page's slab past its records is left as it was.
        out: (counts, cands) to write into instead of new tensors."""
        scores, dists = list(scores), list(dists)
        if len(scores) != len(dists) or not scores:
            raise ValueError(f"op_pico_candidates: {len(scores)} score tensors and {len(dists)} distribution tensors")
        m = 2 if split else 1
        B = int(scores[0].shape[0])
        anchors = []
        for sc, bd in zip(scores, dists):
            self._chk(sc, self.act_dtype, "scores")
            self._chk(bd, self.act_dtype, "dists")
            a = sc.numel() // (B * sc.shape[-1])
            if sc.shape[0] != B or bd.shape[0] != B or bd.numel() // (B * bd.shape[-1]) != a or sc.shape[-1] != scores[0].shape[-1] \
                    or bd.shape[-1] != dists[0].shape[-1]:
                raise ValueError(f"op_pico_candidates: level shapes {tuple(sc.shape)} / {tuple(bd.shape)} do not pair up, or differ in width from level 0")
            anchors.append(a)
        n = len(scores)
        if out is None:
            counts = torch.empty((B,), dtype=torch.int32, device=self._tdev)
            cands = torch.empty((B, int(max_cands), L.PT_LAYOUT_CAND_FLOATS), dtype=torch.float32, device=self._tdev)
        else:
            counts, cands = out
            self._chk(counts, torch.int32, "counts")
            self._chk(cands, torch.float32, "cands")
            if counts.numel() < B or cands.numel() < B * int(max_cands) * L.PT_LAYOUT_CAND_FLOATS:
                raise ValueError("op_pico_candidates: output buffers too small")
        h_s = (C.c_void_p * n)(*[t.data_ptr() for t in scores])
        h_d = (C.c_void_p * n)(*[t.data_ptr() for t in dists])
        h_a = (C.c_int * n)(*anchors)
        L.check(self.lib.pt_op_pico_candidates(self._h, h_s, h_d, h_a, n, B, scores[0].shape[-1] // m, dists[0].shape[-1] // m, int(ncls), float(thr_lo),
                                               int(max_cands), _ptr(counts), _ptr(cands), int(split), self._stream()), "pt_op_pico_candidates")
        return counts, cands

    def op_layout_decode(self, counts: torch.Tensor, cands: torch.Tensor, ncls: int, strides, inp_h: int, inp_w: int, org_h: int, org_w: int,
                         probs: bool, score_threshold: float, nms_threshold: float, nms_top_k: int = 1000, candidate_size: int = 200,
                         keep_top_k: int = 100, max_dets: Optional[int] = None, out=None):
        """LayoutStage.decode_page for every page of a batch in one launch (pt_op_layout_decode, csrc/layout_decode.hip).  counts int32 [B] / cands
        float32 [B, max_cands, 48]: the candidate records of layout_forward / op_pico_candidates, in any order; probs: the class columns are
        probabilities (an ONNX export) rather than logits -> (ndet int32 [B], dets float64 [B, max_dets, 6] = (x0, y0, x1, y1, score, class)) on the
        device: per page classes ascending, within a class the greedy pick order; ndet counts every detection, dets holds the first max_dets
        (default ncls * min(keep_top_k, candidate_size)); rows past a page's count are left as they were.  Equal scores: (level, anchor)
        ascending.  out: (ndet, dets) to write into instead of new tensors.  Everything stays on the device; nothing synchronises."""
        self._chk(counts, torch.int32, "counts")
        self._chk(cands, torch.float32, "cands")
        if cands.dim() != 3 or cands.shape[2] != L.PT_LAYOUT_CAND_FLOATS or counts.numel() != cands.shape[0]:
            raise ValueError(f"op_layout_decode: counts [B] and cands [B, max_cands, {L.PT_LAYOUT_CAND_FLOATS}] expected, got {tuple(counts.shape)} "
                             f"and {tuple(cands.shape)}")
        B, max_cands = int(cands.shape[0]), int(cands.shape[1])
        strides = [int(s) for s in strides]
        if max_dets is None:
            max_dets = int(ncls) * (min(int(keep_top_k), int(candidate_size)) if keep_top_k > 0 else int(candidate_size))
        if out is None:
            ndet = torch.empty((B,), dtype=torch.int32, device=self._tdev)
            dets = torch.empty((B, max(int(max_dets), 1), 6), dtype=torch.float64, device=self._tdev)
        else:
            ndet, dets = out
            self._chk(ndet, torch.int32, "ndet")
            self._chk(dets, torch.float64, "dets")
            if ndet.numel() < B or dets.numel() < B * int(max_dets) * 6:
                raise ValueError("op_layout_decode: output buffers too small")
        h_st = (C.c_int * max(len(strides), 1))(*strides)
        L.check(self.lib.pt_op_layout_decode(_ptr(counts), _ptr(cands), B, max_cands, int(ncls), len(strides), h_st, int(inp_h), int(inp_w), int(org_h),
                                             int(org_w), int(bool(probs)), float(score_threshold), float(nms_threshold), int(nms_top_k),
                                             int(candidate_size), int(keep_top_k), int(max_dets), _ptr(ndet), _ptr(dets), self._stream()),
                "pt_op_layout_decode")
        return ndet, dets

    def slanet_preprocess(self, pages: torch.Tensor, tables: np.ndarray, size: int = 488) -> torch.Tensor:
        """SLANetPreprocessor on resident pages (pt_slanet_preprocess): pages uint8 [n_pages, h, w, 3], tables TSR_TABLE_DTYPE records (page, x0, y0,
        crop_w, crop_h) -> float32 NHWC [n, size, size, 3] in B, G, R order, zero-padded at the bottom and the right"""
        self._chk(pages, torch.uint8, "pages")
        assert tables.dtype == TSR_TABLE_DTYPE
        n = len(tables)
        host = np.ascontiguousarray(tables)
        d_tab = _upload(host.view(np.uint8).reshape(-1), self._tdev)
        out = torch.empty((n, int(size), int(size), 3), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_slanet_preprocess(self._h, _ptr(pages), pages.shape[0], pages.shape[1], pages.shape[2], _ptr(d_tab), C.c_void_p(host.ctypes.data), n,
                                              int(size), _ptr(out), self._stream()), "pt_slanet_preprocess")
        return out

    def op_sla_scratch_bytes(self, B: int, N: int, hidden: int) -> int:
        n = C.c_longlong(0)
        L.check(self.lib.pt_op_sla_scratch_bytes(int(B), int(N), int(hidden), C.byref(n)), "pt_op_sla_scratch_bytes")
        return int(n.value)

    def op_sla_decode(self, fea: torch.Tensor, c: int, w16: torch.Tensor, f32: torch.Tensor, hidden: int, n_cls: int, n_loc: int, steps: int,
                      eos_id: int = -1, force_ids: Optional[torch.Tensor] = None, split: bool = False, scratch: Optional[torch.Tensor] = None):
        """The whole greedy walk of SLANet's head in one launch (pt_op_sla_decode, csrc/sla_head.hip).  fea: token rows [B, N, c_pad] ([hi | lo] of
        that width when split), the first c channels real; w16 / f32: the images of weights.pack_sla_head on the device (w16 any 2-byte dtype,
        [halves, n16]); scratch: a uint8 tensor of op_sla_scratch_bytes(B, N, hidden) bytes (allocated here when None) ->
        (probs float32 [B, T, V], loc float32 [B, T, L], ids int32 [B, T], steps int32 [B]).  eos_id >= 0: a table stops after the first step
        t > 0 whose id is eos_id, the rows after it are zeros; force_ids int32 [B, T]: the id fed to step t + 1 (ids still report the arg-max)."""
        self._chk(fea, self.act_dtype, "fea")
        self._chk(f32, torch.float32, "f32")
        if fea.dim() != 3:
            raise ValueError(f"op_sla_decode: fea must be [B, N, c_pad], got {tuple(fea.shape)}")
        B, N = fea.shape[0], fea.shape[1]
        m = 2 if split else 1
        cp = fea.shape[2] // m
        n16, n32 = C.c_longlong(0), C.c_longlong(0)
        L.check(self.lib.pt_op_sla_packed_elems(int(hidden), int(c), int(n_cls), int(n_loc), C.byref(n16), C.byref(n32)), "pt_op_sla_packed_elems")
        if not (w16.is_cuda and w16.is_contiguous() and w16.element_size() == 2 and w16.numel() == m * n16.value and f32.numel() == n32.value):
            raise ValueError(f"op_sla_decode: packed images of {w16.numel()} / {f32.numel()} values, {m * n16.value} / {n32.value} expected "
                             f"(weights.pack_sla_head, split={bool(split)})")
        T = int(steps)
        if force_ids is not None:
            self._chk(force_ids, torch.int32, "force_ids")
            if tuple(force_ids.shape) != (B, T):
                raise ValueError(f"op_sla_decode: force_ids must be [{B}, {T}], got {tuple(force_ids.shape)}")
        need = self.op_sla_scratch_bytes(B, N, hidden)
        if scratch is None:
            scratch = torch.empty((need,), dtype=torch.uint8, device=self._tdev)
        self._chk(scratch, torch.uint8, "scratch")
        probs = torch.empty((B, T, int(n_cls)), dtype=torch.float32, device=self._tdev)
        loc = torch.empty((B, T, int(n_loc)), dtype=torch.float32, device=self._tdev)
        ids = torch.empty((B, T), dtype=torch.int32, device=self._tdev)
        nsteps = torch.empty((B,), dtype=torch.int32, device=self._tdev)
        L.check(self.lib.pt_op_sla_decode(self._h, _ptr(fea), B, N, cp, int(c), int(hidden), int(n_cls), int(n_loc), T, _ptr(w16), _ptr(f32), _ptr(scratch),
                                          scratch.numel(), int(eos_id), _ptr(force_ids), _ptr(probs), _ptr(loc), _ptr(ids), _ptr(nsteps), int(split),
                                          self._stream()), "pt_op_sla_decode")
        return probs, loc, ids, nsteps

    def op_table_match(self, loc: torch.Tensor, ids: torch.Tensor, steps: Optional[torch.Tensor], cell_flags: torch.Tensor, frames: torch.Tensor,
                       lines: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        """Text lines -> cell rows of the tables op_sla_decode walked, in one launch (pt_op_table_match, csrc/table_match.hip): TableMatch's
        _filter_ocr_result + match_result on the device.  loc float32 [B, T, L] / ids int32 [B, T] / steps int32 [B] or None (all T rows): the head's
        outputs; cell_flags uint8 [V], 1 at the cell tokens; frames float32 [B, 4] = (w, h, x0, y0) per table; lines float32 [M, 4] grouped by table
        and offsets int32 [B + 1] (0 .. M, non-decreasing) -> int32 [M]: per line the step index t of its cell row, -1 for a line the y filter drops
        or a table without a cell row.  Everything stays on the device; nothing synchronises."""
        self._chk(loc, torch.float32, "loc")
        self._chk(ids, torch.int32, "ids")
        self._chk(cell_flags, torch.uint8, "cell_flags")
        self._chk(frames, torch.float32, "frames")
        self._chk(lines, torch.float32, "lines")
        self._chk(offsets, torch.int32, "offsets")
        if steps is not None:
            self._chk(steps, torch.int32, "steps")
        if loc.dim() != 3 or tuple(ids.shape) != tuple(loc.shape[:2]):
            raise ValueError(f"op_table_match: loc must be [B, T, L] and ids [B, T], got {tuple(loc.shape)} and {tuple(ids.shape)}")
        B, T, L_ = loc.shape
        M = lines.numel() // 4
        if lines.numel() != 4 * M or frames.numel() != 4 * B or offsets.numel() != B + 1 or (steps is not None and steps.numel() != B):
            raise ValueError(f"op_table_match: {B} tables need frames [B, 4], offsets [B + 1], steps [B] and lines [M, 4]; got {tuple(frames.shape)}, "
                             f"{tuple(offsets.shape)}, {None if steps is None else tuple(steps.shape)}, {tuple(lines.shape)}")
        out = torch.empty((M,), dtype=torch.int32, device=self._tdev)
        L.check(self.lib.pt_op_table_match(_ptr(loc), _ptr(ids), _ptr(steps), B, T, L_, _ptr(cell_flags), cell_flags.numel(), _ptr(frames), _ptr(lines),
                                           _ptr(offsets), M, _ptr(out), self._stream()), "pt_op_table_match")
        return out

    def op_lore_match(self, dets: torch.Tensor, axes: torch.Tensor, counts: torch.Tensor, affine: torch.Tensor, offset: torch.Tensor,
                      lines: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        """Text lines -> cell rows of Lore tables, in one launch (pt_op_lore_match, csrc/lore_match.hip): table_text_match.find_top1_match over the
        cells table_cells_from_logits would build, on the device.  dets float32 [B, PT_TSR_MAX_CELLS, 9] (tsr_decode) / axes float32
        [B, PT_TSR_MAX_CELLS, 4] (tsr_process: ``stacked`` or ``logic``, unrounded) / counts int32 [B]; affine float64 [B, 6]: the inverse map
        transform_quads builds, per table; offset float64 [B, 2]: the crop's (x0, y0); lines float32 [M, 4] grouped by table and offsets int32
        [B + 1] (0 .. M, non-decreasing) -> int32 [M]: per line the INPUT row index of its cell, -1 in a table without cells.  Everything stays
        on the device; nothing synchronises."""
        self._chk(dets, torch.float32, "dets")
        self._chk(axes, torch.float32, "axes")
        self._chk(counts, torch.int32, "counts")
        self._chk(affine, torch.float64, "affine")
        self._chk(offset, torch.float64, "offset")
        self._chk(lines, torch.float32, "lines")
        self._chk(offsets, torch.int32, "offsets")
        if dets.dim() != 3 or tuple(dets.shape[1:]) != (L.PT_TSR_MAX_CELLS, 9) or tuple(axes.shape) != (dets.shape[0], L.PT_TSR_MAX_CELLS, 4):
            raise ValueError(f"op_lore_match: dets must be [B, {L.PT_TSR_MAX_CELLS}, 9] and axes [B, {L.PT_TSR_MAX_CELLS}, 4], got {tuple(dets.shape)} "
                             f"and {tuple(axes.shape)}")
        B = dets.shape[0]
        M = lines.numel() // 4
        if lines.numel() != 4 * M or counts.numel() != B or affine.numel() != 6 * B or offset.numel() != 2 * B or offsets.numel() != B + 1:
            raise ValueError(f"op_lore_match: {B} tables need counts [B], affine [B, 6], offset [B, 2], offsets [B + 1] and lines [M, 4]; got "
                             f"{tuple(counts.shape)}, {tuple(affine.shape)}, {tuple(offset.shape)}, {tuple(offsets.shape)}, {tuple(lines.shape)}")
        out = torch.empty((M,), dtype=torch.int32, device=self._tdev)
        L.check(self.lib.pt_op_lore_match(_ptr(dets), _ptr(axes), _ptr(counts), B, _ptr(affine), _ptr(offset), _ptr(lines), _ptr(offsets), M,
                                          _ptr(out), self._stream()), "pt_op_lore_match")
        return out

    # ---- the TEDS table metric's kernels (csrc/teds.hip, engine-free; pdf_table_amd/table_metric.py packs their arrays) ----
    def op_teds_cost(self, tok: torch.Tensor, coff: torch.Tensor, pairs: torch.Tensor, h_coff, h_pairs, out: Optional[torch.Tensor] = None,
                     c_elems: Optional[int] = None) -> torch.Tensor:
        """Cell contents -> rename costs, in one launch (pt_op_teds_cost): levenshtein / max(len) in float64 for every (row content, column content)
        of every table pair.  tok int32 [n_tok] token ids; coff int32 [n_cont + 1] CSR offsets of the contents (at most 1024 tokens each); pairs int64
        [P, 5] = (first row content, rows, first column content, columns, offset in `out`); h_coff / h_pairs: the same two arrays as numpy arrays on
        the host, which every limit is checked on (PtError, nothing launched, where one is broken).  out float64 [>= c_elems] (default: allocated to
        fit) receives each pair's rows x columns matrix; c_elems: how much of `out` the call may write (default: all of it)."""
        import numpy as np
        self._chk(tok, torch.int32, "tok")
        self._chk(coff, torch.int32, "coff")
        self._chk(pairs, torch.int64, "pairs")
        h_coff = np.ascontiguousarray(h_coff, dtype=np.int32)
        h_pairs = np.ascontiguousarray(h_pairs, dtype=np.int64).reshape(-1, 5)
        P = h_pairs.shape[0]
        if pairs.numel() != 5 * P or coff.numel() != h_coff.size or h_coff.size < 1:
            raise ValueError(f"op_teds_cost: the host copies do not fit the device arrays: pairs {tuple(pairs.shape)} / {h_pairs.shape}, coff "
                             f"{tuple(coff.shape)} / {h_coff.shape}")
        if out is None:
            need = int((h_pairs[:, 4] + h_pairs[:, 1] * h_pairs[:, 3]).max()) if P else 0
            out = torch.empty((max(need, 1),), dtype=torch.float64, device=self._tdev)
        self._chk(out, torch.float64, "out")
        c_elems = out.numel() if c_elems is None else int(c_elems)
        if c_elems > out.numel():
            raise ValueError(f"op_teds_cost: c_elems {c_elems} above the {out.numel()} elements of out")
        L.check(self.lib.pt_op_teds_cost(_ptr(tok), tok.numel(), _ptr(coff), C.c_void_p(h_coff.ctypes.data), h_coff.size - 1, _ptr(pairs),
                                         C.c_void_p(h_pairs.ctypes.data), P, _ptr(out), c_elems, self._stream()), "pt_op_teds_cost")
        return out

    def op_teds_dist(self, pairs: torch.Tensor, h_pairs, node: torch.Tensor, lml: torch.Tensor, kr: torch.Tensor, grp: torch.Tensor,
                     costs: torch.Tensor, scratch: torch.Tensor, out: Optional[torch.Tensor] = None, c_elems: Optional[int] = None,
                     scratch_bytes: Optional[int] = None) -> torch.Tensor:
        """Flattened table trees -> ordered tree edit distances (insert = delete = 1), one workgroup per table pair in one launch (pt_op_teds_dist).
        pairs int64 [P, 16] and its host copy h_pairs (numpy), node int32 [n_nodes, 4], lml int32 [n_nodes], kr int32 [n_kr], grp int32 [n_grp],
        costs float64 (op_teds_cost's output): see include/pdftable_hip.h.  scratch: uint8 or float64 device buffer, table_metric.scratch_bytes(n1, n2)
        bytes per pair at the pairs' own offsets.  -> float64 [>= P] (`out`, or a new tensor): the distances.  A tree above 4096 nodes or a scratch too
        small is refused (PtError) and nothing is launched."""
        import numpy as np
        self._chk(pairs, torch.int64, "pairs")
        for t, n in ((node, "node"), (lml, "lml"), (kr, "kr"), (grp, "grp")):
            self._chk(t, torch.int32, n)
        self._chk(costs, torch.float64, "costs")
        self._chk(scratch, torch.float64 if scratch.dtype == torch.float64 else torch.uint8, "scratch")
        h_pairs = np.ascontiguousarray(h_pairs, dtype=np.int64).reshape(-1, 16)
        P = h_pairs.shape[0]
        if pairs.numel() != 16 * P or node.numel() != 4 * lml.numel():
            raise ValueError(f"op_teds_dist: pairs {tuple(pairs.shape)} / host {h_pairs.shape}, node {tuple(node.shape)}, lml {tuple(lml.shape)} do not fit")
        if out is None:
            out = torch.empty((max(P, 1),), dtype=torch.float64, device=self._tdev)
        self._chk(out, torch.float64, "out")
        if out.numel() < P:
            raise ValueError(f"op_teds_dist: out holds {out.numel()} distances, {P} pairs")
        c_elems = costs.numel() if c_elems is None else int(c_elems)
        have = scratch.numel() * scratch.element_size()
        scratch_bytes = have if scratch_bytes is None else int(scratch_bytes)
        if c_elems > costs.numel() or scratch_bytes > have:
            raise ValueError("op_teds_dist: c_elems / scratch_bytes above the buffers' sizes")
        L.check(self.lib.pt_op_teds_dist(_ptr(pairs), C.c_void_p(h_pairs.ctypes.data), P, _ptr(node), _ptr(lml), lml.numel(), _ptr(kr), kr.numel(),
                                         _ptr(grp), grp.numel(), _ptr(costs), c_elems, _ptr(scratch), scratch_bytes, _ptr(out), self._stream()),
                "pt_op_teds_dist")
        return out

    # ---- the WTW cell metric's matching (csrc/cell_metric.hip, engine-free; pdf_table_amd/cell_metric.py packs its arrays) ----
    def op_cell_metric(self, boxes: torch.Tensor, axes: torch.Tensor, pairs: torch.Tensor, h_pairs, iou_threshold: float = 0.5,
                       moff: Optional[torch.Tensor] = None, h_moff=None, match: Optional[torch.Tensor] = None,
                       counts: Optional[torch.Tensor] = None, match_elems: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Cells of (prediction, truth) table pairs -> per truth cell the first prediction cell at iou >= iou_threshold, one workgroup per pair in
        one launch (pt_op_cell_metric).  boxes float64 [N, 4] = (x1, y1, x3, y3), axes int32 [N, 4], pairs int64 [P, 4] = (first prediction cell,
        prediction cells, first truth cell, truth cells) and its host copy h_pairs (numpy), which every limit is checked on (PtError, nothing
        launched, where one is broken: more than 4096 cells, a range outside N).  moff int64 [P] / h_moff: where each pair's matches start in
        `match` (default: the prefix sum of the truth counts, uploaded here; pass both to stay free of allocation and upload).  -> (match int32
        [>= match_elems]: input index of the prediction cell inside its table or -1, truth cells in input order; counts int32 [P, 2] = (matches,
        matches with four equal axes)); `match` / `counts`: buffers to write into, match_elems: how much of `match` the call may write."""
        import numpy as np
        self._chk(boxes, torch.float64, "boxes")
        self._chk(axes, torch.int32, "axes")
        self._chk(pairs, torch.int64, "pairs")
        h_pairs = np.ascontiguousarray(h_pairs, dtype=np.int64).reshape(-1, 4)
        P = h_pairs.shape[0]
        N = boxes.numel() // 4
        if pairs.numel() != 4 * P or boxes.numel() != 4 * N or axes.numel() != 4 * N:
            raise ValueError(f"op_cell_metric: pairs {tuple(pairs.shape)} / host {h_pairs.shape}, boxes {tuple(boxes.shape)}, axes {tuple(axes.shape)} do not fit")
        if (moff is None) != (h_moff is None):
            raise ValueError("op_cell_metric: moff and h_moff go together")
        if h_moff is None:
            h_moff = np.concatenate([[0], np.cumsum(np.clip(h_pairs[:, 3], 0, None))[:-1]]).astype(np.int64) if P else np.zeros(0, np.int64)
            moff = torch.from_numpy(h_moff).to(self._tdev)
        h_moff = np.ascontiguousarray(h_moff, dtype=np.int64).reshape(-1)
        self._chk(moff, torch.int64, "moff")
        if moff.numel() != P or h_moff.size != P:
            raise ValueError(f"op_cell_metric: {P} pairs, moff {tuple(moff.shape)} / host {h_moff.shape}")
        if match is None:
            need = int((h_moff + np.clip(h_pairs[:, 3], 0, None)).max()) if P else 0
            match = torch.empty((max(need, 1),), dtype=torch.int32, device=self._tdev)
        if counts is None:
            counts = torch.empty((max(P, 1), 2), dtype=torch.int32, device=self._tdev)
        self._chk(match, torch.int32, "match")
        self._chk(counts, torch.int32, "counts")
        match_elems = match.numel() if match_elems is None else int(match_elems)
        if match_elems > match.numel() or counts.numel() < 2 * P:
            raise ValueError(f"op_cell_metric: match_elems {match_elems} above the {match.numel()} elements of match, or counts {tuple(counts.shape)} "
                             f"below {P} pairs")
        L.check(self.lib.pt_op_cell_metric(_ptr(boxes), _ptr(axes), N, _ptr(pairs), C.c_void_p(h_pairs.ctypes.data), P, _ptr(moff),
                                           C.c_void_p(h_moff.ctypes.data), float(iou_threshold), _ptr(match), match_elems, _ptr(counts),
                                           self._stream()), "pt_op_cell_metric")
        return match, counts

    def op_attention(self, qkv: torch.Tensor, heads: int, d: int, scale: float, out_c: int, split: bool = False) -> torch.Tensor:
        """qkv bf16 [B, 1, T, >= 3 heads d] rows of [q | k | v] -> bf16 [B, 1, T, out_c] (channels heads * d .. out_c are zero); split: both tensors
        carry [hi | lo] halves of that width"""
        self._chk(qkv, self.act_dtype, "qkv")
        B, T = qkv.shape[0], qkv.shape[-2]
        m = 2 if split else 1
        out = torch.zeros((B, 1, T, int(out_c) * m), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_attention(self._h, _ptr(qkv), B, T, int(heads), int(d), qkv.shape[-1] // m, float(scale), _ptr(out), int(out_c), int(split),
                                         self._stream()), "pt_op_attention")
        return out

    # ---- the ConvNextViT recogniser's kernels one at a time (csrc/cvit_model.hip; no model loaded) ---------------------
    def op_cvit_mlp(self, xb: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor, b2: torch.Tensor, x: torch.Tensor,
                    rows: Optional[int] = None) -> torch.Tensor:
        """x [>= rows, C] fp32 += W2 GELU(W1 xb + b1) + b2 IN PLACE over the first `rows` rows (default: all of xb's); w1 / w2p: the 16-bit
        patterns of weights.pack_cvit_mlp on the device (any 2-byte dtype)."""
        self._chk(xb, self.act_dtype, "xb")
        for t, n in ((b1, "b1"), (b2, "b2"), (x, "x")):
            self._chk(t, torch.float32, n)
        Cc = xb.shape[-1]
        rows = xb.shape[0] if rows is None else int(rows)
        if (w1.element_size() != 2 or w2p.element_size() != 2 or w1.numel() != 4 * Cc * Cc or w2p.numel() != 4 * Cc * Cc or not w1.is_contiguous()
                or not w2p.is_contiguous() or b1.numel() != 4 * Cc or b2.numel() != Cc or x.shape[-1] != Cc or rows > min(xb.shape[0], x.shape[0])):
            raise ValueError(f"op_cvit_mlp: operands do not fit C = {Cc}, rows = {rows}")
        L.check(self.lib.pt_op_cvit_mlp(self._h, _ptr(xb), rows, Cc, _ptr(w1), _ptr(b1), _ptr(w2p), _ptr(b2), _ptr(x), self._stream()), "pt_op_cvit_mlp")
        return x

    def op_cvit_attention(self, qkv: torch.Tensor, split: bool = False) -> torch.Tensor:
        """qkv [nchunks * 75, 576] rows of [q | k | v], 3 heads of 64, q already scaled -> [nchunks * 75, 192]; split: [hi | lo] rows of twice the width"""
        self._chk(qkv, self.act_dtype, "qkv")
        m = 2 if split else 1
        if qkv.dim() != 2 or qkv.shape[1] != 576 * m or qkv.shape[0] % 75:
            raise ValueError(f"op_cvit_attention: qkv must be [nchunks * 75, {576 * m}], got {tuple(qkv.shape)}")
        out = torch.zeros((qkv.shape[0], 192 * m), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_cvit_attention(self._h, _ptr(qkv), qkv.shape[0] // 75, _ptr(out), int(split), self._stream()), "pt_op_cvit_attention")
        return out

    def op_cvit_dwconv_ln(self, x: torch.Tensor, w49: torch.Tensor, bias: torch.Tensor, g: torch.Tensor, beta: torch.Tensor, split: bool = False) -> torch.Tensor:
        """depthwise 7x7 (padding 3) + LayerNorm(C, 1e-6) of the fp32 map x [B, H, W, C] -> 16-bit [B, H, W, C] ([hi | lo] when split); w49 [49, C]"""
        for t, n in ((x, "x"), (w49, "w49"), (bias, "bias"), (g, "g"), (beta, "beta")):
            self._chk(t, torch.float32, n)
        B, H, W, Cc = x.shape
        if tuple(w49.shape) != (49, Cc) or bias.numel() != Cc or g.numel() != Cc or beta.numel() != Cc:
            raise ValueError(f"op_cvit_dwconv_ln: parameters do not fit C = {Cc}")
        out = torch.zeros((B, H, W, Cc * (2 if split else 1)), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_cvit_dwconv_ln(self._h, _ptr(x), B, H, W, Cc, _ptr(w49), _ptr(bias), _ptr(g), _ptr(beta), _ptr(out), int(split),
                                              self._stream()), "pt_op_cvit_dwconv_ln")
        return out

    def op_cvit_ln(self, x: torch.Tensor, out: torch.Tensor, rows: int, g: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float, mode: int = 0,
                   H: int = 1, W: int = 1, cmap: Optional[torch.Tensor] = None, split: bool = False) -> torch.Tensor:
        """cvit_ln_kernel over `rows` rows (mode 2: OUTPUT rows) of the fp32 rows x [.., C] into the caller's `out` (the caller sizes it for the mode:
        pt_op_cvit_ln in include/pdftable_hip.h); g = beta = None: conversion only; cmap: int32 device tensor (mode 2)"""
        self._chk(x, torch.float32, "x")
        self._chk(out, self.act_dtype, "out")
        for t, n in ((g, "g"), (beta, "beta")):
            if t is not None:
                self._chk(t, torch.float32, n)
        if cmap is not None:
            self._chk(cmap, torch.int32, "cmap")
        L.check(self.lib.pt_op_cvit_ln(self._h, _ptr(x), int(rows), x.shape[-1], _ptr(g), _ptr(beta), float(eps), _ptr(out), int(split), int(mode), int(H),
                                       int(W), _ptr(cmap), self._stream()), "pt_op_cvit_ln")
        return out

    # ---- the MtlTabNet decoders' attention kernels one at a time (csrc/mtl_decoder.hip; no model loaded) ------------------
    def mtl_pick_split(self, ntiles: int, hw: int):
        """(nsplit, keys_per_split) the decoding loops use for `ntiles` query tiles over hw keys (host arithmetic)"""
        return mtl_pick_split(ntiles, hw)

    def op_mtl_cross_attention(self, kernel: int, q: torch.Tensor, kv: torch.Tensor, n_tables: int, hw: int, slot: int, tiles, keys_per_split: int, nsplit: int,
                               npos: int, M: int, Mp: int, att: torch.Tensor, opart: Optional[torch.Tensor] = None, mlpart: Optional[torch.Tensor] = None,
                               split: bool = False, nb: int = 1, row_bs: int = 0, opart_bs: int = 0, ml_bs: int = 0) -> torch.Tensor:
        """pt_op_mtl_cross_attention (include/pdftable_hip.h) into the caller's `att`.  kernel: L.PT_MTL_ATTN_*; tiles: host rows of (table, first query
        row, queries, row stride); kv: the 16-bit [n_tables * hw, 5120] keys / values (x 2: [hi | lo] when split) or their uint8 e4m3 copy (STREAM8)."""
        m = 2 if split else 1
        self._chk(q, self.act_dtype, "q")
        self._chk(att, self.act_dtype, "att")
        self._chk(kv, torch.uint8 if kernel == L.PT_MTL_ATTN_STREAM8 else self.act_dtype, "kv")
        tl = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 4))
        R = int(npos) * int(Mp)
        rows_need = (int(nb) - 1) * int(row_bs) + R * 512 * m
        if q.numel() < rows_need or att.numel() < rows_need or kv.numel() < int(n_tables) * int(hw) * 5120 * (1 if kernel == L.PT_MTL_ATTN_STREAM8 else m):
            raise ValueError("op_mtl_cross_attention: q / att / kv are smaller than the shapes announce")
        if nsplit > 1:
            self._chk(opart, torch.float32, "opart")
            self._chk(mlpart, torch.float32, "mlpart")
            if opart.numel() < (int(nb) - 1) * int(opart_bs) + nsplit * R * 512 or mlpart.numel() < (int(nb) - 1) * int(ml_bs) + nsplit * R * 16:
                raise ValueError("op_mtl_cross_attention: partial buffers are smaller than nsplit slices announce")
        d_tiles = torch.empty((max(len(tl), 1), 4), dtype=torch.int32, device=self._tdev)
        self._mtl_tiles = (tl, d_tiles)          # the host list is read by a copy on the stream: keep it until the next call
        L.check(self.lib.pt_op_mtl_cross_attention(self._h, int(kernel), _ptr(q), _ptr(kv), int(n_tables), int(hw), int(slot), C.c_void_p(tl.ctypes.data), len(tl),
                                                   _ptr(d_tiles), int(keys_per_split), int(nsplit), int(npos), int(M), int(Mp), _ptr(opart), _ptr(mlpart), _ptr(att),
                                                   int(split), int(nb), int(row_bs), int(opart_bs), int(ml_bs), self._stream()), "pt_op_mtl_cross_attention")
        return att

    def op_mtl_self_attention(self, cache: torch.Tensor, tok: torch.Tensor, pad: int, p0: int, p1: int, Mp: int, M: int, att: torch.Tensor, split: bool = False,
                              nb: int = 1, cache_bs: int = 0, att_bs: int = 0) -> torch.Tensor:
        """pt_op_mtl_self_attention into the caller's `att`: cache [p1 + 1, Mp, 1536] rows of [q | k | v] (x 2 when split), tok int32 [>= p1 + 1, Mp]"""
        m = 2 if split else 1
        self._chk(cache, self.act_dtype, "cache")
        self._chk(att, self.act_dtype, "att")
        self._chk(tok, torch.int32, "tok")
        if (cache.numel() < (int(nb) - 1) * int(cache_bs) + (int(p1) + 1) * int(Mp) * 1536 * m or tok.numel() < (int(p1) + 1) * int(Mp)
                or att.numel() < (int(nb) - 1) * int(att_bs) + (int(p1) - int(p0) + 1) * int(Mp) * 512 * m):
            raise ValueError("op_mtl_self_attention: cache / tok / att are smaller than the shapes announce")
        L.check(self.lib.pt_op_mtl_self_attention(self._h, _ptr(cache), _ptr(tok), int(pad), int(p0), int(p1), int(Mp), int(M), _ptr(att), int(split), int(nb),
                                                  int(cache_bs), int(att_bs), self._stream()), "pt_op_mtl_self_attention")
        return att

    def op_mtl_kv_fp8(self, kv: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the e4m3 copy (x 8, saturating) of a 16-bit tensor whose element count is a multiple of 8 -> uint8 of the same shape (or the first
        kv.numel() bytes of the caller's `out`)"""
        self._chk(kv, self.act_dtype, "kv")
        if out is None:
            out = torch.zeros(kv.shape, dtype=torch.uint8, device=self._tdev)
        self._chk(out, torch.uint8, "out")
        if out.numel() < kv.numel():
            raise ValueError("op_mtl_kv_fp8: out is smaller than kv")
        L.check(self.lib.pt_op_mtl_kv_fp8(self._h, _ptr(kv), kv.numel(), _ptr(out), self._stream()), "pt_op_mtl_kv_fp8")
        return out

    # ---- the Lore processor's kernels one at a time (pt_op_lore_* in include/pdftable_hip.h): outputs are the caller's, so that a test can pre-fill them
    @staticmethod
    def _lore_counts(counts):
        import numpy as np
        hc = np.ascontiguousarray(counts, dtype=np.int32)
        return hc, int(hc.clip(0, L.PT_TSR_MAX_CELLS).sum()), int(((hc.clip(0, L.PT_TSR_MAX_CELLS) + 31) // 32).sum())

    def op_lore_tok_prepare(self, logi: torch.Tensor, dets: Optional[torch.Tensor], counts, x_pe: Optional[torch.Tensor], y_pe: Optional[torch.Tensor],
                            x0: torch.Tensor, cat: torch.Tensor, use_pe: bool, split: bool = False) -> torch.Tensor:
        """pt_op_lore_tok_prepare into the caller's x0 [Npad, 256] and cat [Npad, 512] (x 2 when split) -> the device token map int32 [N, 2]"""
        hc, N, _ = self._lore_counts(counts)
        m = 2 if split else 1
        self._chk(logi, torch.float32, "logi")
        self._chk(x0, self.act_dtype, "x0")
        self._chk(cat, self.act_dtype, "cat")
        for t, name in ((dets, "dets"), (x_pe, "x_pe"), (y_pe, "y_pe")):
            if t is not None:
                self._chk(t, torch.float32, name)
        Npad = x0.shape[0]
        if (logi.shape != (len(hc), L.PT_TSR_MAX_CELLS, 256) or (dets is not None and dets.shape != (len(hc), L.PT_TSR_MAX_CELLS, 9)) or x0.shape != (Npad, 256 * m)
                or cat.shape != (Npad, 512 * m) or any(t is not None and t.shape != (256, 256) for t in (x_pe, y_pe))):
            raise ValueError("op_lore_tok_prepare: operands do not fit the counts")
        tok = torch.full((max(N, 1), 2), -1, dtype=torch.int32, device=self._tdev)
        L.check(self.lib.pt_op_lore_tok_prepare(self._h, _ptr(logi), _ptr(dets), hc.ctypes.data, len(hc), int(use_pe), _ptr(x_pe), _ptr(y_pe), Npad, _ptr(tok),
                                                _ptr(x0), _ptr(cat), int(split), self._stream()), "pt_op_lore_tok_prepare")
        return tok[:N]

    def op_lore_norm(self, x: torch.Tensor, alpha: Optional[torch.Tensor], bias: Optional[torch.Tensor], out: torch.Tensor, split: bool = False) -> torch.Tensor:
        """pt_op_lore_norm of fp32 rows [rows, 256] into the caller's `out` (at least rows x 256, x 2 when split); alpha = bias = None: conversion only"""
        self._chk(x, torch.float32, "x")
        self._chk(out, self.act_dtype, "out")
        for t in (alpha, bias):
            if t is not None:
                self._chk(t, torch.float32, "alpha / bias")
        if x.dim() != 2 or x.shape[1] != 256 or out.numel() < x.numel() * (2 if split else 1) or any(t is not None and t.numel() != 256 for t in (alpha, bias)):
            raise ValueError("op_lore_norm: x must be [rows, 256], out at least as large, alpha / bias [256]")
        L.check(self.lib.pt_op_lore_norm(self._h, _ptr(x), x.shape[0], _ptr(alpha), _ptr(bias), _ptr(out), int(split), self._stream()), "pt_op_lore_norm")
        return out

    def op_lore_cvt_logic(self, x: torch.Tensor, out: torch.Tensor, split: bool = False) -> torch.Tensor:
        """pt_op_lore_cvt_logic: fp32 [Npad, 8] into the caller's `out` [Npad, 32] (x 2 when split)"""
        self._chk(x, torch.float32, "x")
        self._chk(out, self.act_dtype, "out")
        if x.dim() != 2 or x.shape[1] != 8 or out.numel() < x.shape[0] * 32 * (2 if split else 1):
            raise ValueError("op_lore_cvt_logic: x must be [Npad, 8], out at least [Npad, 32]")
        L.check(self.lib.pt_op_lore_cvt_logic(self._h, _ptr(x), _ptr(out), x.shape[0], int(split), self._stream()), "pt_op_lore_cvt_logic")
        return out

    def op_lore_attention(self, qkv: torch.Tensor, counts, out: torch.Tensor, split: bool = False) -> torch.Tensor:
        """pt_op_lore_attention: qkv [Npad, 768] (x 2 when split) into the caller's `out` [Npad, 256] (x 2 when split) -> the device tile list int32 [tiles, 3]"""
        hc, _, ntiles = self._lore_counts(counts)
        m = 2 if split else 1
        self._chk(qkv, self.act_dtype, "qkv")
        self._chk(out, self.act_dtype, "out")
        Npad = qkv.shape[0]
        if qkv.dim() != 2 or qkv.shape[1] != 768 * m or out.shape != (Npad, 256 * m):
            raise ValueError(f"op_lore_attention: qkv must be [Npad, {768 * m}] and out [Npad, {256 * m}]")
        tiles = torch.full((max(ntiles, 1), 3), -1, dtype=torch.int32, device=self._tdev)
        L.check(self.lib.pt_op_lore_attention(self._h, _ptr(qkv), hc.ctypes.data, len(hc), Npad, _ptr(tiles), _ptr(out), int(split), self._stream()),
                "pt_op_lore_attention")
        return tiles[:ntiles]

    def op_lore_scatter4(self, x: torch.Tensor, tok: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """pt_op_lore_scatter4: fp32 token rows [>= N, 8] -> the caller's `out` [n_tables, PT_TSR_MAX_CELLS, 4] at the (table, row) pairs of tok int32 [N, 2]"""
        self._chk(x, torch.float32, "x")
        self._chk(tok, torch.int32, "tok")
        self._chk(out, torch.float32, "out")
        N = tok.shape[0]
        if x.dim() != 2 or x.shape[1] != 8 or x.shape[0] < N or out.dim() != 3 or out.shape[1:] != (L.PT_TSR_MAX_CELLS, 4):
            raise ValueError("op_lore_scatter4: x must be [>= N, 8], out [n_tables, PT_TSR_MAX_CELLS, 4]")
        L.check(self.lib.pt_op_lore_scatter4(self._h, _ptr(x), _ptr(tok), N, _ptr(out), self._stream()), "pt_op_lore_scatter4")
        return out

    def op_lstm(self, pregates: torch.Tensor, r_packed: torch.Tensor, hidden: int, dirs: int, reverse: bool, out_c: int, split: bool = False) -> torch.Tensor:
        """The recurrence of an ONNX LSTM layer (pt_op_lstm; hidden <= 128, zero initial states).  pregates [B, 1, T, dirs * 4 * Hp] (x m halves
        when split) = X W^T + Wb + Rb, gates i, o, f, c per direction; r_packed: weights.pack_lstm_r(R) on the device -> token rows
        [B, 1, T, out_c] (x m): h_t at channel d * hidden + unit, forward units first, the channels from dirs * hidden on zero."""
        self._chk(pregates, self.act_dtype, "pregates")
        B, T = pregates.shape[0], pregates.shape[-2]
        m = 2 if split else 1
        need = self.lib.pt_op_lstm_packed_elems(int(hidden), int(dirs), int(split))
        if need == 0 or r_packed.numel() != need or not r_packed.is_contiguous() or r_packed.element_size() != 2:
            raise ValueError(f"op_lstm: packed R of {r_packed.numel()} values for hidden {hidden}, dirs {dirs}, split {int(split)} ({need} expected)")
        out = torch.zeros((B, 1, T, int(out_c) * m), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_lstm(self._h, _ptr(pregates), pregates.shape[-1], _ptr(r_packed), T, B, int(hidden), int(dirs), int(bool(reverse)), _ptr(out),
                                    out.shape[-1], int(split), self._stream()), "pt_op_lstm")
        return out

    def op_stem7x7(self, x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        B, H, W, _ = x.shape
        out = torch.empty((B, H // 2, W // 2, 128 if split else 64), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_stem7x7(self._h, _ptr(x), B, H, W, _ptr(w), _ptr(bias), _ptr(out), int(split), self._stream()),
                "pt_op_stem7x7")
        return out

    def op_maxpool3x3s2(self, x: torch.Tensor, split: bool = False) -> torch.Tensor:
        self._chk(x, self.act_dtype, "x")
        B, H, W, Cc = x.shape
        out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), dtype=self.act_dtype, device=self._tdev)
        L.check(self.lib.pt_op_maxpool3x3s2(self._h, _ptr(x), B, H, W, Cc // 2 if split else Cc, _ptr(out), int(split),
                                            self._stream()),
                "pt_op_maxpool3x3s2")
        return out

    def op_db_head_final(self, x: torch.Tensor, w4x64: torch.Tensor, bias: torch.Tensor, split: bool = False):
        self._chk(x, self.act_dtype, "x")
        B, H, W, _ = x.shape
        prob = torch.empty((B, 2 * H, 2 * W), dtype=torch.float32, device=self._tdev)
        logits = torch.empty((B, 2 * H, 2 * W), dtype=torch.float32, device=self._tdev)
        L.check(self.lib.pt_op_db_head_final(self._h, _ptr(x), B, H, W, _ptr(w4x64), _ptr(bias), _ptr(prob),
                                             _ptr(logits), int(split), self._stream()), "pt_op_db_head_final")
        return prob, logits

    # ---- profiling ---------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        """True / 1: HIP events around every launch; 2 + L.PT_PROF_CLASSES.index(name): only that kernel class; False: off"""
        L.check(self.lib.pt_profile_enable(self._h, int(on)), "pt_profile_enable")

    def profile_read_labels(self):
        """-> {label: {"launches", "ms", "flop", "bytes"}} of the launches recorded since the last read (profile_enable(1))"""
        buf = C.create_string_buffer(1 << 18)
        L.check(self.lib.pt_profile_read_labels(self._h, buf, len(buf)), "pt_profile_read_labels")
        out = {}
        for ln in buf.value.decode().splitlines():
            lab, n, ms, fl, by = ln.split("\t")
            out[lab] = {"launches": int(n), "ms": float(ms), "flop": float(fl), "bytes": float(by)}
        return out

    def profile_read(self):
        ms = (C.c_double * 4)()
        nl = (C.c_longlong * 4)()
        fl = (C.c_double * 4)()
        L.check(self.lib.pt_profile_read(self._h, ms, nl, fl), "pt_profile_read")
        return {k: {"ms": ms[i], "launches": nl[i], "flop": fl[i]} for i, k in enumerate(L.PT_PROF_CLASSES)}



def _serialised(fn):
    @functools.wraps(fn)
    def call(self, *a, **kw):
        with self._lock:
            return fn(self, *a, **kw)
    return call


# every public method of the handle queues its pt_* calls under the engine's lock (see HipEngine.__init__); close() / __del__ stay free of it
for _name, _fn in list(vars(HipEngine).items()):
    if callable(_fn) and not _name.startswith("_") and _name not in ("close", "precision_scope") and not isinstance(_fn, (property, staticmethod, classmethod)):
        setattr(HipEngine, _name, _serialised(_fn))


# ---- host-side halves of the DB post-process (no GPU needed) -------------------------------------------
def db_candidates(bitmap_words: np.ndarray, max_candidates: int = 1000, min_size: float = 3.0):
    """bitmap uint32/int32 [H, W/32] of one page -> (boxes f32 [k,8] TL,TR,BR,BL ; sside f32 [k])."""
    lib = L.load()
    bm = np.ascontiguousarray(bitmap_words).view(np.uint32)
    H, wpr = bm.shape
    cap = max_candidates
    boxes = np.empty((cap, 8), dtype=np.float32)
    sside = np.empty((cap,), dtype=np.float32)
    n = C.c_int()
    L.check(lib.pt_db_candidates(bm.ctypes.data_as(C.c_void_p), H, wpr * 32, max_candidates, float(min_size),
                                 boxes.ctypes.data_as(C.c_void_p), sside.ctypes.data_as(C.c_void_p), cap,
                                 C.byref(n)), "pt_db_candidates")
    return boxes[:n.value].copy(), sside[:n.value].copy()


def db_candidates_batch(bitmaps: np.ndarray, max_candidates: int = 1000, min_size: float = 3.0, n_threads: int = 0):
    """bitmaps uint32/int32 [n, H, W/32] -> (boxes f32 [n, cap, 8], counts int32 [n]); pages run on threads inside the library"""
    lib = L.load()
    bm = np.ascontiguousarray(bitmaps).view(np.uint32)
    n, H, wpr = bm.shape
    cap = max_candidates
    boxes = np.empty((n, cap, 8), dtype=np.float32)
    counts = np.zeros((n,), dtype=np.int32)
    L.check(lib.pt_db_candidates_batch(bm.ctypes.data_as(C.c_void_p), n, H, wpr * 32, max_candidates, float(min_size), int(n_threads),
                                       boxes.ctypes.data_as(C.c_void_p), None, cap, counts.ctypes.data_as(C.c_void_p)),
            "pt_db_candidates_batch")
    return boxes, counts


def db_contour_candidates_batch(bitmaps: np.ndarray, max_candidates: int = 1000, min_size: float = 3.0, n_threads: int = 0,
                                points: Optional[np.ndarray] = None, alloc=None):
    """db_candidates_batch that also returns the traced contour of every kept candidate (pt_db_contour_candidates_batch; what score_mode "slow"
    scores).  -> (boxes f32 [n, cap, 8], counts int32 [n], points int32 [np, 2] (x, y), offsets int32 [sum(counts) + 1]): candidate j, counted over
    the pages in order, owns points[offsets[j]:offsets[j + 1]].  points: a C-contiguous int32 [cap, 2] array to write into (DetStage passes a view
    of pinned memory); alloc(np) -> such an array of at least np rows (default: numpy).  A buffer that is too small loses nothing but the call: the
    library reports how many points there are, alloc gives a buffer that holds them and the call is made again; the result is a view of the buffer."""
    lib = L.load()
    bm = np.ascontiguousarray(bitmaps).view(np.uint32)
    n, H, wpr = bm.shape
    cap = max_candidates
    boxes = np.empty((n, cap, 8), dtype=np.float32)
    counts = np.zeros((n,), dtype=np.int32)
    offsets = np.zeros((n * cap + 1,), dtype=np.int32)
    alloc = alloc or (lambda k: np.empty((k, 2), dtype=np.int32))
    if points is None:
        points = alloc(max(1024, 64 * n))
    need = C.c_longlong()
    for _ in range(2):
        if points.dtype != np.int32 or points.ndim != 2 or points.shape[1] != 2 or not points.flags.c_contiguous:
            raise ValueError("db_contour_candidates_batch: points must be a C-contiguous int32 [cap, 2] array")
        L.check(lib.pt_db_contour_candidates_batch(bm.ctypes.data_as(C.c_void_p), n, H, wpr * 32, max_candidates, float(min_size), int(n_threads),
                                                   boxes.ctypes.data_as(C.c_void_p), None, cap, counts.ctypes.data_as(C.c_void_p),
                                                   points.ctypes.data_as(C.c_void_p), points.shape[0], offsets.ctypes.data_as(C.c_void_p),
                                                   C.byref(need)), "pt_db_contour_candidates_batch")
        if need.value <= points.shape[0]:
            break
        points = alloc(int(need.value))
    else:
        raise L.PtError(f"pt_db_contour_candidates_batch: alloc returned {points.shape[0]} rows for {need.value} points")
    return boxes, counts, points[:need.value], offsets[:int(counts.sum()) + 1]


def db_finalize_batch(boxes: np.ndarray, scores: np.ndarray, counts: np.ndarray, net_hw, dest_hw, box_thresh: float = 0.6,
                      unclip_ratio: float = 1.5, min_size: float = 3.0, post_flavour: int = L.PT_DET_POST_DB_PP,
                      filter_tag: bool = False, n_threads: int = 0):
    """boxes f32 [n, cap, 8], scores f32 [n, cap], counts int32 [n] -> per page: int32 [k, 8] boxes, or, with filter_tag
    (the db_pp flavour's filter_tag_det_res), float32 [k, 8]"""
    lib = L.load()
    n, cap, _ = boxes.shape
    out = np.empty((n, cap, 8), dtype=np.int32)
    outf = np.empty((n, cap, 8), dtype=np.float32) if filter_tag else None
    nout = np.zeros((n,), dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    L.check(lib.pt_db_finalize_batch(boxes.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p),
                                     counts.ctypes.data_as(C.c_void_p), n, cap, float(box_thresh), float(unclip_ratio), float(min_size),
                                     int(net_hw[0]), int(net_hw[1]), int(dest_hw[0]), int(dest_hw[1]), int(post_flavour),
                                     1 if filter_tag else 0, int(n_threads), out.ctypes.data_as(C.c_void_p),
                                     outf.ctypes.data_as(C.c_void_p) if filter_tag else None, None, nout.ctypes.data_as(C.c_void_p)),
            "pt_db_finalize_batch")
    src = outf if filter_tag else out
    return [src[i, :nout[i]].copy() for i in range(n)]


def db_finalize(boxes: np.ndarray, scores: np.ndarray, net_hw, dest_hw, box_thresh: float = 0.6,
                unclip_ratio: float = 1.5, min_size: float = 3.0, post_flavour: int = L.PT_DET_POST_DB_PP):
    lib = L.load()
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 8)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    nb = boxes.shape[0]
    out = np.empty((max(nb, 1), 8), dtype=np.int32)
    osc = np.empty((max(nb, 1),), dtype=np.float32)
    n = C.c_int()
    L.check(lib.pt_db_finalize(boxes.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), nb,
                               float(box_thresh), float(unclip_ratio), float(min_size), int(net_hw[0]), int(net_hw[1]),
                               int(dest_hw[0]), int(dest_hw[1]), int(post_flavour), out.ctypes.data_as(C.c_void_p),
                               osc.ctypes.data_as(C.c_void_p), max(nb, 1), C.byref(n)), "pt_db_finalize")
    return out[:n.value].copy(), osc[:n.value].copy()


def page_line_angles(bits: np.ndarray, w: int, min_width: int = 400, n_threads: int = 16) -> list:
    """bit-packed line masks int64 / uint64 [n, h, (w + 63) // 64] (HipEngine.page_line_mask) -> per page a float64 array of the
    get_line_angle values of every RETR_EXTERNAL contour wider than min_width, in cv2's contour order; pages run on n_threads (<= 16)"""
    lib = L.load()
    b = np.ascontiguousarray(bits).view(np.uint64)
    n, h, nw = b.shape
    assert nw == (w + 63) // 64
    # external contours are disjoint: at most one per two rows in every 401-column span wider than min_width
    cap = ((h + 1) // 2) * (w // (min_width + 1) + 1) + 1
    angles = np.empty((n, cap), dtype=np.float64)
    counts = np.zeros((n,), dtype=np.int32)
    L.check(lib.pt_page_line_angles(b.ctypes.data_as(C.c_void_p), n, h, w, int(min_width), max(1, min(16, int(n_threads))),
                                    angles.ctypes.data_as(C.c_void_p), cap, counts.ctypes.data_as(C.c_void_p)), "pt_page_line_angles")
    return [angles[i, :counts[i]].copy() for i in range(n)]


def page_pre_tables():
    """(the 15 fixed-point blur taps int32, the bicubic weight table int16 [1024, 16]) the page kernels use"""
    lib = L.load()
    taps = np.zeros((15,), dtype=np.int32)
    cub = np.zeros((1024, 16), dtype=np.int16)
    L.check(lib.pt_page_pre_tables(taps.ctypes.data_as(C.c_void_p), cub.ctypes.data_as(C.c_void_p)), "pt_page_pre_tables")
    return taps, cub
