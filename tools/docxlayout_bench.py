"""DocXLayout on the engine, measured (profiles/r21/docxlayout.txt): one process, warm-up first, medians with ranges of 7 windows.

  kernel  pt_docx_decode per call at 64 pages of 192 x 192 maps: a seeded net's peak counts, and the full case (every value a peak: 100 + 100
          records a page through the radix-select path).  Device events around 10 back-to-back calls; ms per call.
  stage   DocXLayoutStage forward + finish per 64 pages of 1024 x 1024 (bf16), split into pre-process, net, decode (device events) and the
          host half (host clock).  Context lines, no pass / fail ratio: the in-tree LayoutStage (PicoDet, another model) on the same pages,
          alternating in the same process, and the CPU restatement's module run by torch in fp16 on the same GPU.
  stream  predict_stream() with detection, recognition and this layout on seeded pages (8 batches of 16).  pages/s.

    python tools/docxlayout_bench.py [out.txt]
"""
from __future__ import annotations

import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.docxlayout_stage import DOCX_MEAN, DOCX_STD, DocXLayoutConfig, DocXLayoutStage, docx_page_result  # noqa: E402
from pdf_table_amd.engine import HipEngine  # noqa: E402
from pdf_table_amd.synth_weights import docxlayout_dla34_state_dict  # noqa: E402
from pdf_table_amd.weights import pack_docxlayout_dla34  # noqa: E402

B, RUNS = 64, 7


def stats(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def stage_and_kernel_bench(out):
    from pdf_table_amd.synth_pages import make_page
    eng = HipEngine(0)
    sd = docxlayout_dla34_state_dict(seed=0)
    eng.load_weights(L.PT_MODEL_DOCX_DLA34, pack_docxlayout_dla34(sd, fmt=eng.weight_fmt))
    st = DocXLayoutStage(eng, DocXLayoutConfig())
    pages = torch.from_numpy(np.stack([make_page(i % 8, 1024)[0] for i in range(B)])).to(eng._tdev)
    org = tuple(pages.shape[1:3])
    tb = st._tables(B, *org)
    mb = st.micro_batch
    heads = {k: torch.empty((B, 192, 192, 16 if k == "hm" else 8), dtype=torch.float32, device=eng._tdev) for k in HipEngine.DOCX_HEADS}
    xs = [None]

    def pre():
        xs[0] = [eng.docx_preprocess(pages, tb[i:i + mb], 768, 768, mean=DOCX_MEAN, std=DOCX_STD) for i in range(0, B, mb)]

    def net():
        for k, x in enumerate(xs[0]):
            eng.docx_forward_net(x, out={h: v[k * mb:(k + 1) * mb] for h, v in heads.items()})

    outs = [None]

    def dec():
        outs[0] = eng.docx_decode(heads, with_inds=False)

    for f in (pre, net, dec):
        f()
    torch.cuda.synchronize()
    counts = outs[0][0].cpu().numpy()
    t_pre = [_events(pre, 2) for _ in range(RUNS)]
    t_net = [_events(net, 1) for _ in range(RUNS)]
    t_dec = [_events(dec, 10) for _ in range(RUNS)]
    flat = {k: torch.zeros_like(v) for k, v in heads.items()}
    full = lambda: eng.docx_decode(flat, with_inds=False)
    full()
    torch.cuda.synchronize()
    t_full = [_events(full, 10) for _ in range(RUNS)]
    out.append(f"== kernel: pt_docx_decode, {B} pages of 192 x 192 maps per call; ms per call, median (min .. max) of {RUNS} windows of 10 calls ==")
    out.append(f"seeded net (records per page: main {counts[:, 0].min()} .. {counts[:, 0].max()}, sub {counts[:, 1].min()} .. {counts[:, 1].max()}): {stats(t_dec)}")
    out.append(f"every value a peak (100 + 100 records a page, radix select):        {stats(t_full)}")
    # the host half alone, on the landed arrays
    c, r, _, k = (None if t is None else t.cpu().numpy() for t in outs[0])
    t_host = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        res = [docx_page_result(r[i, 0, :c[i, 0]][k[i, 0, :c[i, 0]] != 0], r[i, 1, :c[i, 1]][k[i, 1, :c[i, 1]] != 0], org, (192, 192)) for i in range(B)]
        t_host.append((time.perf_counter() - t0) * 1e3)
    t_all = []
    for _ in range(RUNS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, ticket = st.forward(pages)
        st.finish(n, ticket, org)
        t_all.append((time.perf_counter() - t0) * 1e3)
    nreg = [len(x) for x in res]
    out.append(f"== stage: DocXLayoutStage (seeded checkpoint, bf16), per {B} pages of 1024 x 1024 at 768 x 768, micro-batches of {mb}; regions per page "
               f"{min(nreg)} .. {max(nreg)}; ms, median (min .. max) of {RUNS} ==")
    out.append(f"pre-process (device events): {stats(t_pre)}")
    out.append(f"net         (device events): {stats(t_net)}")
    out.append(f"decode      (device events): {stats(t_dec)}")
    out.append(f"host half   (host clock)   : {stats(t_host)}")
    out.append(f"forward + finish (host clock, the first call dropped): {stats(t_all[1:])}")
    # context: the in-tree PicoDet stage on the same pages, alternating
    from pdf_table_amd.ocr_layout_task import OcrLayoutTask
    pico = OcrLayoutTask(model="picodet", task_type="en", synthetic_seed=4, engine=eng)._stage
    both = {"DocXLayoutStage": (st, []), "LayoutStage (PicoDet)": (pico, [])}
    for rep in range(RUNS + 1):
        for name, (s, ms) in both.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n, ticket = s.forward(pages)
            s.finish(n, ticket, org)
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3)
    out.append("-- context (another model, no ratio asserted): forward + finish on the same pages, alternating in this process --")
    for name, (_, ms) in both.items():
        out.append(f"{name:24s}: {stats(ms)}")
    # context: the restatement's module by torch in fp16 on the same GPU (a context line: a torch build without half convolutions only loses the line)
    try:
        import docxlayout_ref as R
        sd16 = {k: (v.cuda().half() if v.is_floating_point() else v.cuda()) for k, v in sd.items()}
        x16 = torch.randn(mb, 3, 768, 768, device="cuda").half()
        with torch.no_grad():
            R.docx_forward(sd16, x16)
            torch.cuda.synchronize()
            t_ref = [_events(lambda: R.docx_forward(sd16, x16), 1) * (B / mb) for _ in range(RUNS)]
        out.append(f"-- context: the restatement's network by torch in fp16 on this GPU, {mb} pages per call, scaled to {B} pages: {stats(t_ref)} ms --")
    except Exception as e:      # noqa: BLE001
        out.append(f"-- context: the restatement's network by torch in fp16 on this GPU: not measured ({type(e).__name__}: {e}) --")
    if statistics.median(t_host) > 0.5 * statistics.median(t_all[1:]):
        out.append("the host half (the comparator sort, in Python) is more than half of forward + finish: the next step, not taken here")
    eng.close()


def stream_bench(out, ckpt):
    from pdf_table_amd.pipeline import OcrTablePipeline
    from pdf_table_amd.synth_pages import make_page
    pipe = OcrTablePipeline(device=0, synthetic_seed=0, layout=True, layout_model="DocXLayout", layout_task_path=ckpt)
    pages = torch.from_numpy(np.stack([make_page(i % 8)[0] for i in range(16)])).to(pipe.engine._tdev)
    batches = [pages] * 8

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(len(r) for r in pipe.predict_stream(batches))
        return n / (time.perf_counter() - t0)

    run()
    pps = [run() for _ in range(RUNS)]
    out.append(f"== stream: predict_stream(), detection + recognition + DocXLayout, seeded, bf16, 8 batches of 16 pages of 1024 x 1024 per run; "
               f"median (min .. max) of {RUNS} ==")
    out.append(f"{stats(pps)} pages/s")
    pipe.engine.close()


if __name__ == "__main__":
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        torch.save(docxlayout_dla34_state_dict(seed=0), os.path.join(tmp, "pytorch_model.bin"))
        stage_and_kernel_bench(lines)
        stream_bench(lines, tmp)
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)
