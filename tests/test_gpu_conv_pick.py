"""The kernel pt_launch_conv takes is the kernel tools/conv_pick.cpp says it takes: both read pdf_table_amd/csrc/conv_pick.h, the library on the
device's CU count and the process's environment, the tool on what it is given.  (The rule itself is tests/test_conv_pick_host.py's.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pdf_table_amd.weights import tile_conv_weight

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_pick") / "conv_pick")
    subprocess.run([shutil.which("c++") or "c++", "-std=c++17", "-O1", "-o", exe, os.path.join(REPO, "tools", "conv_pick.cpp")], check=True)
    return exe


CASES = [
    # B, H, W, Cin, N, ks, stride, residual, switches
    (1, 16, 64, 64, 64, 3, 1, False, {}),
    (2, 37, 45, 64, 128, 3, 1, True, {}),
    (1, 30, 30, 512, 512, 3, 1, False, {}),
    (2, 40, 40, 256, 192, 3, 1, False, {}),
    (2, 33, 47, 256, 512, 3, 2, False, {}),
    (1, 4, 96, 128, 128, 3, 1, False, {}),
    (1, 8, 64, 256, 256, 3, 1, False, {}),
    (1, 3, 64, 64, 64, 3, 1, False, {}),
    (1, 8, 32, 512, 128, 1, 1, False, {}),
    (1, 9, 33, 64, 64, 1, 1, False, {}),
    (1, 8, 32, 32, 64, 1, 1, False, {}),
    (1, 30, 30, 512, 512, 3, 1, False, {"PT_CONV_PIPE": "0"}),
    (1, 9, 33, 64, 64, 1, 1, False, {"PT_CONV1_WIDE": "0"}),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[5]}x{c[5]}s{c[6]}-{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}" + "".join(f"-{k}={v}" for k, v in c[8].items()))
def test_library_takes_what_the_tool_says(eng, tool, case, monkeypatch):
    B, H, W, Cin, N, ks, stride, with_res, sw = case
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(Cin + N + H)
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, Cin, ks, ks, generator=g) * (2.0 / (Cin * ks * ks)) ** 0.5).to(torch.bfloat16).float()
    wt = torch.from_numpy(tile_conv_weight(w).view(np.int16)).to(dev)
    bias = (torch.randn(N, generator=g) * 0.1).to(dev)
    Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    res = torch.randn(B, Ho, Wo, N, generator=g).to(torch.bfloat16).to(dev) if with_res else None
    for k, v in sw.items():
        monkeypatch.setenv(k, v)
    eng.profile_enable(1)
    if ks == 1:
        out = eng.op_conv1x1_ex(x, wt, bias)
    else:
        out = eng.op_conv2d(x, wt, bias, ks, stride, res=res, res_mode=1 if with_res else 0)
    torch.cuda.synchronize()
    labels = list(eng.profile_read_labels())
    eng.profile_enable(False)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    said = subprocess.run([tool, "--num-cu", str(num_cu)] + (["has_res=1", "res_mode=1"] if with_res else []) + [str(v) for v in (B, H, W, Cin, N, ks, stride)],
                          check=True, capture_output=True, text=True).stdout.split("\t")
    assert labels == [said[0]], (labels, said)
    assert torch.isfinite(out.float()).all() and out.float().abs().max() > 0      # the launch happened
