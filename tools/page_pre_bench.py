"""tools/page_pre_bench.py [--kernels-only] [--reps N]: what image-page straightening costs (page_pre.hip, PagePreStage, predict()).

64 generator pages of 1024 x 1024, half of them skewed by 0.5 .. 1.5 degrees (warped on the device by pt_page_warp_cubic itself), one batch.
Times, each the median of N repetitions after a warm-up:
  * the three kernels on the batch (HIP events): the line mask over 64 pages, the cubic warp of the 32 skewed pages, a quarter turn of 64
    pages; beside them a plain device copy of the same page bytes in the same process (torch clone: read + write), and each kernel's rate
    in bytes moved per second as a fraction of that copy's rate;
  * the host copy of the mask bits and the host angle pass (pt_page_line_angles, 16 threads);
  * PagePreStage.deskew on the batch (mask + copy + angles + warp, wall);
  * the page classifiers (text_image_orientation, table_attribute) on the batch, seeded weights;
  * predict() pages/s on the 64 pages, with page_preprocess=True (+ table_attribute) against every switch off (detection + recognition).
--kernels-only runs only the kernel loop: the run to put under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdf_table_amd import engine as E                                      # noqa: E402
from pdf_table_amd import lib as L                                         # noqa: E402
from pdf_table_amd.page_pre_stage import PagePreStage, rotation_minv      # noqa: E402
from pdf_table_amd.synth_pages import make_pages                          # noqa: E402

N = 64


def ev_time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    eng = E.HipEngine(0)
    h = w = 1024
    up = torch.from_numpy(make_pages(0, N, 1024)).cuda()
    idx = list(range(0, N, 2))
    rng = np.random.default_rng(0)
    thetas = rng.uniform(0.5, 1.5, len(idx)) * rng.choice([-1, 1], len(idx))
    minv = np.stack([rotation_minv(h, w, t) for t in thetas])
    pages = up.clone()
    pages[torch.tensor(idx, device="cuda")] = eng.page_warp_cubic(up, minv, idx)
    torch.cuda.synchronize()
    page_bytes = pages.numel()
    out = {"pages": N, "page": [h, w], "skewed": len(idx)}
    reps = a.reps
    for _ in range(2):     # warm-up: code objects, the bicubic table upload
        eng.page_line_mask(pages), eng.page_warp_cubic(pages, minv, idx), eng.page_quarter_turn(pages, L.PT_ROTATE_90_CLOCKWISE)
        pages.clone()
    torch.cuda.synchronize()
    t_mask = ev_time(lambda: eng.page_line_mask(pages), reps)
    t_warp = ev_time(lambda: eng.page_warp_cubic(pages, minv, idx), reps)
    t_turn = ev_time(lambda: eng.page_quarter_turn(pages, L.PT_ROTATE_90_CLOCKWISE), reps)
    t_copy = ev_time(lambda: pages.clone(), reps)
    nw = (w + 63) // 64
    copy_rate = 2 * page_bytes / (t_copy * 1e-3)
    mask_bytes = page_bytes + N * h * nw * 8                       # pages once + bits out
    warp_bytes = 2 * len(idx) * h * w * 3                          # the warped pages in and out
    turn_bytes = 2 * page_bytes
    out["kernels_ms"] = {"page_line_mask (64 pages)": t_mask, "page_warp_cubic (32 pages)": t_warp,
                         "page_quarter_turn (64 pages)": t_turn, "device copy of the 64 pages (clone)": t_copy}
    out["rate_GBps"] = {"copy": copy_rate / 1e9, "mask": mask_bytes / (t_mask * 1e-3) / 1e9,
                        "warp": warp_bytes / (t_warp * 1e-3) / 1e9, "turn": turn_bytes / (t_turn * 1e-3) / 1e9}
    out["rate_vs_copy"] = {k: out["rate_GBps"][k] / out["rate_GBps"]["copy"] for k in ("mask", "warp", "turn")}
    out["device_ms_per_batch_mask_plus_warp"] = t_mask + t_warp
    if a.kernels_only:
        print(json.dumps(out))
        return
    bits_d = eng.page_line_mask(pages)
    torch.cuda.synchronize()
    out["host_ms"] = {"mask bits to host": wall(lambda: bits_d.cpu(), reps)}
    bits = bits_d.cpu().numpy()
    out["host_ms"]["line angles (16 threads)"] = wall(lambda: E.page_line_angles(bits, w, 400, 16), reps)
    st = PagePreStage(eng)
    out["host_ms"]["PagePreStage.deskew (wall)"] = wall(lambda: st.deskew(pages), reps)
    _, ang = st.deskew(pages)
    out["deskew_angles_undo_theta_max_err"] = float(max(abs(t + ang[i]) for t, i in zip(thetas, idx)))
    out["deskew_unskewed_pages_warped"] = int(sum(abs(ang[i]) >= 0.2 for i in range(1, N, 2)))
    from pdf_table_amd.cls_stage import ClsStage
    from pdf_table_amd.synth_weights import pplcnet_state_dict
    from pdf_table_amd.weights import pack_pplcnet
    eng.load_weights(L.PT_MODEL_PPLCNET + 1, pack_pplcnet(pplcnet_state_dict(seed=6, class_num=4)))
    eng.load_weights(L.PT_MODEL_PPLCNET + 2, pack_pplcnet(pplcnet_state_dict(seed=7, class_num=6)))
    co, ca = ClsStage(eng, "text_image_orientation", 1), ClsStage(eng, "table_attribute", 2)
    co.pages(pages), ca.pages(pages)
    out["host_ms"]["text_image_orientation on 64 pages (wall, incl. post)"] = wall(lambda: co.pages(pages), reps)
    out["host_ms"]["table_attribute on 64 pages (wall, incl. post)"] = wall(lambda: ca.pages(pages), reps)
    out["host_ms"]["PagePreStage.orient (wall, both classifiers, turns, second pass)"] = wall(lambda: st.orient(pages, co, ca), reps)
    eng.close()
    del eng
    from pdf_table_amd.pipeline import OcrTablePipeline
    host_pages = list(pages.cpu().numpy())
    res = {}
    for name, kw in (("off", {}), ("page_preprocess=True, table_attribute=True", {"page_preprocess": True, "table_attribute": True})):
        p = OcrTablePipeline(device=0, synthetic_seed=0, **kw)
        p.predict(host_pages[:8])
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            p.predict(host_pages)
            ts.append(time.perf_counter() - t)
        res[name] = N / float(np.median(ts))
        p.engine.close()
        del p
    out["predict_pages_per_s"] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
