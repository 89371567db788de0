"""The dense-conv kernel choice (pdf_table_amd/csrc/conv_pick.h) on the host: tools/conv_pick.cpp, built with the system compiler, against the
labels and kernel names recorded on an MI355X from the commit BEFORE the choice became a function of its own (tools/conv_pick_record.py ->
tests/golden/conv_pick/grid.json: a row on each side of every threshold of the rule at 256 CUs, every switch)."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "conv_pick", "grid.json")
CXX = shutil.which("c++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no c++ compiler")

DEFAULTS = {"PT_CONV1_DIRECT": "1", "PT_CONV_DMA": "1", "PT_CONV_VARIANT": "3", "PT_CONV_S2_DMA": "1", "PT_CONV_HALF": "-1", "PT_N_GROUP": "-1",
            "PT_CONV1_WIDE": "1", "PT_CONV_PIPE": "4", "PT_CONV_PIPE_BLOCKS": "1", "PT_CONV_WS64": "1", "PT_CONV_WS64_GRID": "0", "PT_CONV_PERSIST_GRID": "0",
            "PT_CONV_BLOCK_LIST": "1", "PT_CONV_XP": "unset", "PT_GEMM_PIPE": "1", "PT_GEMM_XP": "1", "PT_LORE_HM_FUSE": "1"}


def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PT_")}


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_pick") / "conv_pick")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-o", exe, os.path.join(REPO, "tools", "conv_pick.cpp")], check=True)
    return exe


def test_header_compiles_alone():
    """plain C++17 with nothing from HIP or common.h"""
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include", os.path.join(REPO, "pdf_table_amd", "csrc", "conv_pick.h"),
                    os.devnull], check=True)


def _switches(tool, *settings, env=None):
    e = _env()
    e.update(env or {})
    out = subprocess.run([tool, "--switches", *settings], check=True, capture_output=True, text=True, env=e).stdout
    return dict(ln.split(" ") for ln in out.splitlines())


def test_switch_defaults(tool):
    assert _switches(tool) == DEFAULTS


@pytest.mark.parametrize("v", range(6))
def test_conv_pipe_values(tool, v):
    """PT_CONV_PIPE decides what it decided when it was tested four ways (atoi < 4, first character, atoi < 3, atoi): from the environment and as a setting"""
    assert _switches(tool, env={"PT_CONV_PIPE": str(v)})["PT_CONV_PIPE"] == str(v)
    assert _switches(tool, f"PT_CONV_PIPE={v}")["PT_CONV_PIPE"] == str(v)
    # an 8-wave 3x3 layer, a stride-2 layer and a block-tile layer at every value: v3 at 0, v4 from 1, v5 (persistent, whatever the tile count) at 5
    rows = [subprocess.run([tool, f"PT_CONV_PIPE={v}", *shape.split()], check=True, capture_output=True, text=True, env=_env()).stdout.split("\t")
            for shape in ("16 64 64 256 256 3 1", "2 33 47 64 128 3 2", "1 4 64 128 128 3 1")]      # (256 tiles of 16 x 32 x 128: one whole round of 256 CUs)
    assert rows[0][0] == f"conv3x3 {'v3' if v == 0 else 'v5' if v == 5 else 'v4'} 256->256 @64x64"
    assert rows[0][1] == {0: "conv3x3_dma16_kernel<2, 8, 1>", 1: "conv3x3_pipe_kernel<2, 8, false, 0, false, 1, false>", 2: "conv3x3_pipe_kernel<2, 8, true, 0, false, 1, false>",
                          3: "conv3x3_pipe_kernel<2, 8, true, 0, true, 1, false>", 4: "conv3x3_pipe_kernel<2, 8, true, 0, true, 1, false>",
                          5: "conv3x3_pipe_persist_kernel<2, 8, 1>"}[v]
    assert rows[1][0] == f"conv3x3 s2 {'v3' if v == 0 else 'v4'} 64->128 @17x24"
    assert rows[2][1] == ("conv_igemm_kernel<3, 1, 1, 2, false, false>" if v == 0 else f"conv3x3_pipe_kernel<2, 8, true, 4, {'true' if v >= 3 else 'false'}, 1, false>")


def test_switch_text_is_atoi(tool):
    """decimal integers: where the first character and atoi disagreed ("01", "abc") atoi decides"""
    assert _switches(tool, "PT_CONV1_WIDE=01", "PT_GEMM_PIPE=abc", "PT_CONV_XP=0", "PT_CONV_HALF=1")["PT_CONV1_WIDE"] == "1"
    got = _switches(tool, "PT_GEMM_PIPE=abc", "PT_CONV_XP=0", "PT_CONV_HALF=1", "PT_CONV_WS64=2")
    assert (got["PT_GEMM_PIPE"], got["PT_CONV_XP"], got["PT_CONV_HALF"], got["PT_CONV_WS64"]) == ("0", "0", "1", "2")


def test_grid_against_recorded_choice(tool):
    with open(GOLDEN) as f:
        lines = [ln for ln in f if ln.strip()]
    rows = [json.loads(ln) for ln in lines]
    assert len(rows) >= 200
    out = subprocess.run([tool], input="".join(lines), check=True, capture_output=True, text=True, env=_env()).stdout.splitlines()
    assert len(out) == len(rows)
    named = 0
    bad = []
    for r, o in zip(rows, out):
        label, name = o.split("\t")[:2]
        if label != r["label"] or ("kernel" in r and name != r["kernel"]):
            bad.append((r, label, name))
        named += "kernel" in r
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, the first: {bad[0]}"
    assert named == len(rows), f"only {named} of {len(rows)} rows carry a kernel name"
