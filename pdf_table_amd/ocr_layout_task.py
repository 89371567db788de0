"""``OcrLayoutTask`` on the HIP engine -- drop-in for the reference's stage-1 plug-in (model="picodet").

Reference: src/pdftable/model/ocr_pdf/ocr_layout_task.py:30-157.  Same constructor (``task, model, task_type``), same
result: one list per input image of ``{"bbox": ndarray [4] (x1, y1, x2, y2 in source pixels; float64 holding float32-rounded corners divided by the scale, as in the reference), "label", "score",
"category_id"}`` (:125-141, picodet/processor_picodet.py:286-296).  The reference runs an ONNX export of PaddleDetection's
picodet_lcnet_x1_0 layout model; here the in-tree LCNet + CSP-PAN + PicoHead graph (assumed hyper-parameters, see
pdf_table_amd.synth_weights.picodet_state_dict) runs on the engine.

``model="DocXLayout"`` (the reference's only torch layout model, ocr_layout_task.py:45-68) serves a checkpoint given as ``task_path=<file or
directory>`` (docxlayout_stage.load_checkpoint) through ``DocXLayoutStage``: same result shape, labels of ``DocXLayoutConfig``.  There are no
seeded in-tree weights for it: without a checkpoint the constructor raises ``RuntimeError``, also when ``synthetic_seed`` is set.  ``device_decode``
is PicoDet's decode and raises ``ValueError`` for this model (its decode always runs on the device).  ``device_order=True`` is this model's own
knob (``DocXLayoutStage(device_order=True)``: region list and reading order on the device) and raises ``ValueError`` for any other model.

ONNX door (the reference's layout stage is ONNX-only: "pytorch model not support yet!", ocr_layout_task.py:82-123): a ``model.onnx`` /
``inference.onnx`` under ``task_path`` (or ``task_path`` = the file) is parsed by ``pdf_table_amd.onnx_import`` and run layer by layer by
``HipGraphExecutor`` behind the engine's own pre-processing kernel; its 2 L outputs are split like ``get_onnx_output_dict`` (:159-175: first
half per-level scores [B, A_l, classes], second half box distributions [B, A_l, 32]) and decoded by the same host post-processor.  The stage
around the graph is ``OnnxLayoutStage`` (layout_stage.py): the anchors that can pass the score threshold are compacted on the device
(``pt_op_pico_candidates``) and one pinned copy brings them to the host, with the ``forward`` / ``finish`` halves ``OcrTablePipeline``
pipelines; ``_detect_pages_host`` keeps the synchronous route (every anchor copied, numpy filters) for comparison.
"""
from __future__ import annotations

import os
import time
from typing import Dict, List

import numpy as np
import torch

from . import lib as L
from .base_infer_task import BaseInferTask
from .engine import HipEngine
from .layout_stage import LayoutStage, OnnxLayoutStage, PicodetConfig
from .ocr_detection_task import _read_image
from .weights import pack_picodet

__all__ = ["OcrLayoutTask"]


class OcrLayoutTask(BaseInferTask):
    def __init__(self, task="ocr_layout", model="picodet", engine: HipEngine = None, device_decode: bool = False, device_order: bool = False, **kwargs):
        # device_decode=True: the stage decodes, cuts and suppresses on the device (LayoutStage(device_decode=True), pt_op_layout_decode)
        self._device_decode = bool(device_decode)
        # device_order=True (DocXLayout only): the region list and the reading order on the device (DocXLayoutStage(device_order=True), pt_op_docx_order)
        self._device_order = bool(device_order)
        if self._device_order and model != "DocXLayout":
            raise ValueError(f"device_order=True puts DocXLayout's region list and reading order on the device (pt_op_docx_order); model={model!r} has "
                             "no such route")
        super().__init__(task=task, model=model, **kwargs)
        if model not in ["picodet", "DocXLayout"]:
            raise RuntimeError(f"current model is not supported: {model}")
        if model == "DocXLayout":
            if self._device_decode:
                raise ValueError("device_decode=True selects PicoDet's device decode; DocXLayout's decode (pt_docx_decode) always runs on the device")
            from .docxlayout_stage import DocXLayoutConfig
            self._config = DocXLayoutConfig()
            self.model_provider = "model_scope"
            self._engine = engine
            tp = kwargs.get("task_path")
            if not tp or not os.path.exists(str(tp)):
                raise RuntimeError("layout model 'DocXLayout' has no in-tree (seeded) weights: pass task_path=<checkpoint file (.pth / .bin / .pt) or "
                                   "directory holding pytorch_model.bin> (synthetic_seed= does not apply)")
            self._config.model_path = str(tp)
            if "resolution" in kwargs:      # the network input; the reference's is fixed at 768 x 768 (tests use smaller ones)
                self._config.resolution = tuple(int(v) for v in kwargs["resolution"])
            self._get_inference_model()
            return
        tt = kwargs.get("task_type", "en")
        self._config = PicodetConfig(task_type="ch" if tt == "zh" else tt)
        self.model_provider = "PaddleOCR"
        self._engine = engine
        try:
            self._config.model_path = self.get_model_name_or_path()
        except Exception:                       # registry lookups for unknown task types: keep the local path
            self._config.model_path = self._task_path
        self._get_inference_model()

    def _construct_docxlayout(self):
        from .docxlayout_stage import load_checkpoint
        from .weights import pack_docxlayout_dla34
        sd = load_checkpoint(self._config.model_path)
        sp = str(self.kwargs.get("stage_precision") or "").lower()
        self._stage_precision = L.PT_PRECISION_BF16X3 if sp in ("fp32", "bf16x3", "float32") else None
        if sp and self._stage_precision is None:
            raise ValueError(f"stage_precision={sp!r}: only 'fp32' (the pair mode for this stage alone) is supported")
        fmt = "bf16" if self._stage_precision is not None else self._engine.weight_fmt
        self._engine.load_weights(L.PT_MODEL_DOCX_DLA34, pack_docxlayout_dla34(sd, x3=True, fmt=fmt))
        self._exec = None
        self._model = self._predict

    def _construct_model(self, model):
        if self._engine is None:
            self._engine = self._new_engine()
        if model == "DocXLayout":
            return self._construct_docxlayout()
        ncls = len(self._config.labels)
        self._exec = None
        onnx_path = self._onnx_file()
        if onnx_path is not None:
            from .onnx_exec import HipGraphExecutor
            from .onnx_import import UnsupportedOnnxGraph
            self._exec = HipGraphExecutor(onnx_path, engine=self._engine, precision=self._exec_precision)      # raises UnsupportedOnnxGraph naming an operator without a kernel
            if len(self._exec.outputs) % 2 or not self._exec.outputs:
                raise UnsupportedOnnxGraph(f"{onnx_path}: a PicoDet export returns 2 L tensors (L score maps, then L box distributions), "
                                           f"this graph returns {self._exec.outputs}")
            self._model = self._predict_onnx
            return
        if self.synthetic_seed is not None:
            from .synth_weights import picodet_state_dict
            sd = picodet_state_dict(seed=int(self.synthetic_seed), num_classes=ncls)
        else:
            path = os.path.join(str(self._config.model_path), "pytorch_model.bin")
            if not os.path.exists(path):
                raise RuntimeError(f"no PicoDet checkpoint under {self._config.model_path}: the reference would download an ONNX "
                                   "export from the hub (no network here, and the ONNX importer is SURVEY.md section 8f-3); pass "
                                   "task_path=<dir with a PicoDet state_dict> or synthetic_seed=<int>")
            sd = torch.load(path, map_location="cpu", weights_only=True)
        # stage_precision="fp32": this stage alone in the pair mode (LayoutStage.precision) -- its blob is then a bf16 blob with the pair tiles whatever
        # the engine's own precision is
        sp = str(self.kwargs.get("stage_precision") or "").lower()
        self._stage_precision = L.PT_PRECISION_BF16X3 if sp in ("fp32", "bf16x3", "float32") else None
        if sp and self._stage_precision is None:
            raise ValueError(f"stage_precision={sp!r}: only 'fp32' (the pair mode for this stage alone) is supported")
        if self._stage_precision is not None:
            self._engine.load_weights(L.PT_MODEL_PICODET, pack_picodet(sd, ncls, x3=True, fmt="bf16"))
        else:
            self._engine.load_weights(L.PT_MODEL_PICODET, pack_picodet(sd, ncls, fmt=self._engine.weight_fmt))
        self._model = self._predict

    def _build_processor(self):
        if self.model == "DocXLayout":
            from .docxlayout_stage import DocXLayoutStage
            # images reach the stage as RGB (files are read as RGB, arrays are taken as RGB: the CenterNet task's convention); the network eats BGR
            self._stage = DocXLayoutStage(self._engine, self._config, bgr=True, precision=getattr(self, "_stage_precision", None),
                                          device_order=self._device_order)
            return
        if getattr(self, "_exec", None) is not None:
            # the graph file behind LayoutStage's contract: forward() / finish() halves, candidate compaction on the device (pt_op_pico_candidates)
            self._stage = OnnxLayoutStage(self._engine, self._exec, self._config, device_decode=self._device_decode)
            return
        self._stage = LayoutStage(self._engine, self._config, precision=getattr(self, "_stage_precision", None), device_decode=self._device_decode)

    def _predict(self, images: List[np.ndarray]) -> List[List[Dict]]:
        out = []
        for img in images:            # images of a call may differ in size: one batch per image, like the reference
            out.append(self._stage(torch.from_numpy(np.ascontiguousarray(img)[None]).to(self._engine._tdev))[0])
        return out

    def get_onnx_output_dict(self, outputs):
        """ocr_layout_task.py:159-175: the first half of the graph outputs are the per-level scores, the second half the box distributions
        (the reference's dict keys are kept: ``boxes`` holds the scores, ``boxes_num`` the distributions)"""
        if self._exec is None:
            return None
        half = len(outputs) // 2
        return dict(boxes=list(outputs[:half]), boxes_num=list(outputs[half:half * 2]))

    def _predict_onnx(self, images: List[np.ndarray]) -> List[List[Dict]]:
        out = []
        for img in images:
            out.extend(self.detect_pages(torch.from_numpy(np.ascontiguousarray(img)[None]).to(self._engine._tdev)))
        return out

    def detect_pages(self, pages: torch.Tensor) -> List[List[Dict]]:
        """batched door: equally sized pages resident on the device.  With an ONNX file: OnnxLayoutStage -- the graph replay, one candidate
        compaction launch, one pinned copy of the records; the result lists equal _detect_pages_host()'s element for element"""
        return self._stage(pages)

    def _detect_pages_host(self, pages: torch.Tensor) -> List[List[Dict]]:
        """the synchronous ONNX route: every anchor of the 2 L graph outputs copied to the host and filtered by numpy (get_onnx_output_dict's
        split, then LayoutStage.decode_outputs).  What detect_pages() is compared against, and what the stage falls back to for graph outputs
        its device tail cannot read"""
        if getattr(self, "_exec", None) is None:
            return self._stage(pages)
        return self._stage.detect_host(pages)

    def _preprocess(self, inputs, **kwargs):
        if not isinstance(inputs, list):
            inputs = [inputs]
        return {"inputs": [{"image": _read_image(it), "image_file": it if isinstance(it, str) else ""} for it in inputs]}

    def _run_model(self, inputs, **kwargs):
        begin = time.time()
        res, elapse = self.infer({"images": [it["image"] for it in inputs["inputs"]]})
        inputs["results"] = [{"results": r, "elapse": elapse} for r in res]
        inputs["use_time"] = time.time() - begin
        return inputs

    def _postprocess(self, inputs, **kwargs):
        return [r["results"] for r in inputs["results"]]
