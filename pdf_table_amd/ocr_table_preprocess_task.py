"""OcrTablePreprocessTask -- the reference's image-page pre-process plug-in (model/ocr_pdf/ocr_table_preprocess_task.py:24-206) on the
HIP engine: the small-angle deskew (pre_rotate_image, :85-114) then the four-way page orientation (rotate_image_v2, :116-163) with the
table_attribute classifier on the same pass (get_image_cls_result, :165-183), through PagePreStage.

Same constructor (config, task_list, ...) and the same ``__call__`` result: ``(image_full, metric)`` with metric keys ``use_time``,
``angle_metric`` ({"angle", "score"[, "angle2", "score2"], "rotate_small"}), ``angle2`` (the deskew angle, as the reference names it)
and ``image_name``.  Deviation: the corrected page is returned, not written back to its file and re-read.  PDF
inputs are out of scope (the reference does not pre-process them either; here they are refused)."""
from __future__ import annotations

import time
from typing import Dict, Optional

from .cls_image_pulc_task import ClsImagePulcTask
from .engine import HipEngine
from .ocr_detection_task import _read_image
from .page_pre_stage import PagePreStage

__all__ = ["OcrTablePreprocessTask"]

# engine slots of the two page classifiers (slot 0 is the text-line orientation classifier's)
TASK_SLOTS = {"text_image_orientation": 1, "table_attribute": 2}


class OcrTablePreprocessTask(object):
    def __init__(self, config=None, task_list=None, debug=True, output_dir=None, predictor_type="pytorch",
                 task="ocr_table_preprocess", engine: Optional[HipEngine] = None, synthetic_seed: Optional[int] = None,
                 task_paths: Optional[Dict[str, str]] = None, **kwargs):
        self.config, self.debug, self.output_dir, self.predictor_type, self.task = config, debug, output_dir, predictor_type, task
        self.task_list = task_list if task_list is not None and isinstance(task_list, list) else ["text_image_orientation",
                                                                                                "table_attribute"]
        unknown = [t for t in self.task_list if t not in TASK_SLOTS]
        if unknown:
            raise KeyError(f"unsupported pre-process classifier task(s) {unknown} (one of {sorted(TASK_SLOTS)})")
        if "table_attribute" in self.task_list and "text_image_orientation" not in self.task_list:
            raise ValueError("table_attribute runs on the page-orientation pass: task_list needs text_image_orientation")
        self._engine = engine if engine is not None else HipEngine(0)
        self.inner_task = {}
        for k, t in enumerate(self.task_list):
            ck = dict(kwargs)
            if synthetic_seed is not None:
                ck["synthetic_seed"] = synthetic_seed + k
            if task_paths and t in task_paths:
                ck["task_path"] = task_paths[t]
            self.inner_task[t] = ClsImagePulcTask(task_type=t, engine=self._engine, slot=TASK_SLOTS[t], **ck)
        self._stage = PagePreStage(self._engine)
        self.table_attribute = None          # the last call's table_attribute result (the reference only logs it)

    def set_output_dir(self, output_dir):
        self.output_dir = output_dir

    def __call__(self, inputs, src_id=None):
        begin = time.time()
        if isinstance(inputs, str) and inputs.lower().endswith(".pdf"):
            raise ValueError("OcrTablePreprocessTask: PDF pages are not pre-processed (the reference skips them too)")
        image_name = inputs if isinstance(inputs, str) else None
        img = _read_image(inputs)
        ori = self.inner_task.get("text_image_orientation")
        att = self.inner_task.get("table_attribute")
        dev, angles, metrics, attrs = self._stage.straighten([img], deskew=True, orientation=None if ori is None else ori._stage,
                                                             attribute=None if att is None else att._stage)
        angle_metric = dict(metrics[0]) if metrics[0] is not None else {}
        angle_metric["rotate_small"] = angles[0]
        self.table_attribute = attrs[0]
        metric = {"use_time": time.time() - begin, "angle_metric": angle_metric, "angle2": angles[0], "image_name": image_name}
        return dev[0].cpu().numpy(), metric
