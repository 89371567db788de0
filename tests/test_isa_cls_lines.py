"""The fused text-line pre-process of the orientation classifier (cls_line_resize_norm_kernel) and the crop kernel it shares its sampler with
(rec_warp_kernel) compile without FLAT-encoded memory instructions: the crop reads stay global loads, the row stage stays in LDS (no GPU)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_cls_line_kernel_has_no_flat_instructions():
    spec = importlib.util.spec_from_file_location("isa_wait_audit", os.path.join(ROOT, "tools", "isa_wait_audit.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    csrc = os.path.join(ROOT, "pdf_table_amd", "csrc")
    res = t.audit([os.path.join(csrc, "cls_kernels.hip")])
    hits = {k: v for k, v in res.items() if "cls_line_resize_norm_kernel" in k}
    assert hits, sorted(res)
    flat = {k: v[2] for k, v in res.items() if v[2]}
    assert not flat, flat
