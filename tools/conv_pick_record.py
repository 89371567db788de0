"""Record which kernel pt_launch_conv takes for a grid of layers, on the GPU: the golden of tests/test_conv_pick_host.py.

    python tools/conv_pick_record.py groups                        the read-once switch settings of the grid, one per line ("-" = none)
    python tools/conv_pick_record.py run GROUP OUT.json            launch every row of that group once with profiling on; one JSON row per line:
                                                                   {"shape": {...}, "switches": {...}, "num_cu": n, "label": "..."}
    python tools/conv_pick_record.py names OUT.json TRACE.csv      add "kernel" to the rows from a rocprofv3 --kernel-trace of the same `run`: the i-th
                                                                   kernel of namespace pt_bf16 in the trace belongs to the i-th row (counts must match)

Read-once switches (PT_CONV_VARIANT, PT_CONV_DMA, ...) need a process each: `run` sets its group's before the library loads.  The per-call ones are
flipped row by row.  Uses only op_conv2d, op_conv1x1_ex and the launch profile, so it runs unchanged against any commit of the library.
The grid has a row on each side of every threshold of the selection rule on a 256-CU device (pdf_table_amd/csrc/conv_pick.h)."""
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PER_CALL = ("PT_CONV1_WIDE", "PT_CONV_PIPE", "PT_CONV_PIPE_BLOCKS", "PT_CONV_WS64", "PT_CONV_WS64_GRID", "PT_CONV_PERSIST_GRID", "PT_CONV_BLOCK_LIST",
            "PT_CONV_XP", "PT_GEMM_PIPE", "PT_GEMM_XP", "PT_LORE_HM_FUSE")
ONCE = ("PT_CONV1_DIRECT", "PT_CONV_DMA", "PT_CONV_VARIANT", "PT_CONV_S2_DMA", "PT_CONV_HALF", "PT_N_GROUP")


def row(B, H, W, Cin, N, ks=3, stride=1, sw=None, **extra):
    """extra: res (bool), relu, split, rep, shuffle_cout (op_conv2d); ex (op_conv1x1_ex) with out_f32, n_valid, ylimit (rows)"""
    shape = dict(B=B, H=H, W=W, Cin=Cin, N=N, ks=ks, stride=stride)
    return dict(shape=shape, switches=dict(sw or {}), extra=extra)


def grid(group):
    """rows of one read-once setting ({} = the defaults)"""
    R = []
    if not group:
        # weight-stationary 64 -> 64: 16 x 32 tiles >= 4 CU (9 x 240 x 240 = 1080 takes it, 8 x 240 x 240 = 960 does not)
        for B in (9, 8):
            R += [row(B, 240, 240, 64, 64), row(B, 240, 240, 64, 64, res=True, relu=1), row(B, 240, 240, 64, 64, sw={"PT_CONV_WS64": "0"})]
        R += [row(8, 240, 240, 64, 64, sw={"PT_CONV_WS64": "2"}), row(1, 16, 64, 64, 64, sw={"PT_CONV_WS64": "2"}), row(1, 16, 64, 64, 64, sw={"PT_CONV_WS64": "1"}),
              row(1, 16, 64, 64, 64, sw={"PT_CONV_WS64": "2", "PT_CONV_WS64_GRID": "1"}), row(1, 16, 64, 64, 64, rep=2, sw={"PT_CONV_WS64": "2"}),
              row(1, 16, 64, 64, 64, relu=2, sw={"PT_CONV_WS64": "2"})]
        # output rows: 11 / 12 with N % 128 == 0, 23 / 24 otherwise
        R += [row(2, 11, 64, 256, 256), row(2, 12, 64, 256, 256), row(2, 23, 40, 256, 192), row(2, 24, 40, 256, 192), row(2, 23, 40, 256, 64), row(2, 24, 40, 256, 64)]
        # 4-wave against 8-wave tile: Cin 128 / 160 on 64 x 32 x 64 maps (256 tiles of 16 x 32 x 128: one whole round of 256 CUs, so only Cin decides);
        # the other two pairs are ragged grids (128 and 24 tiles), where the 4-wave tile is taken at either Cin
        R += [row(64, 32, 64, 128, 128), row(64, 32, 64, 160, 128), row(32, 32, 64, 128, 128), row(32, 32, 64, 160, 128), row(2, 40, 40, 128, 128), row(2, 40, 40, 160, 128)]
        # ragged last round: 512 -> 512 @32x32, B = 44 (352 tiles) and B = 32 (256); persistent form from 2 CU tiles up (B = 64: 512; B = 63: 504)
        R += [row(B, 32, 32, 512, 512) for B in (44, 32, 63, 64)]
        R += [row(B, 64, 64, 256, 256) for B in (16, 31, 32)] + [row(32, 64, 64, 256, 256, res=True, relu=1), row(32, 64, 64, 256, 256, relu=2)]
        # 64 -> 256: the 8-wave persistent tile from 2 CU tiles up without a residual, the 4-wave tile with one
        R += [row(2, 256, 256, 64, 256), row(2, 256, 256, 64, 256, res=True), row(1, 256, 256, 64, 256), row(2, 256, 256, 64, 256, sw={"PT_CONV_PIPE": "3"})]
        # N % 128 != 0: the 32 x 32 x 64 8-wave tile (N = 64: 256 tiles, one whole round) under every PT_CONV_PIPE
        R += [row(2, 40, 40, 256, 192), row(64, 64, 64, 256, 192), row(2, 40, 40, 64, 192, res=True)]
        R += [row(64, 64, 64, 256, 64)] + [row(64, 64, 64, 256, 64, sw={"PT_CONV_PIPE": pv}) for pv in "0125"]
        # PT_CONV_PIPE 0 .. 5 on an 8-wave layer, a 4-wave layer, a residual layer, a replicated-output layer and a (hi | lo) layer
        for pv in "012345":
            sw = {"PT_CONV_PIPE": pv}
            R += [row(2, 40, 40, 256, 256, sw=sw), row(2, 40, 40, 128, 128, sw=sw), row(2, 37, 45, 64, 128, res=True, relu=1, sw=sw), row(1, 30, 30, 512, 512, sw=sw),
                  row(1, 16, 32, 256, 64, rep=2, sw=sw), row(2, 40, 40, 128, 128, split=1, sw=sw), row(2, 40, 40, 256, 192, sw=sw)]
        R += [row(1, 30, 30, 512, 512, sw={"PT_CONV_PIPE": "5", "PT_CONV_PERSIST_GRID": "3"})]
        # split = 1 / 2
        R += [row(2, 40, 40, 128, 128, split=1), row(2, 40, 40, 256, 256, split=1, res=True), row(1, 16, 32, 64, 64, split=1), row(2, 40, 40, 128, 128, split=2),
              row(1, 16, 32, 64, 64, split=2), row(9, 240, 240, 64, 64, split=1)]
        # pixel-shuffle and hardswish 3x3 layers
        R += [row(1, 16, 32, 64, 256, shuffle_cout=64), row(2, 40, 40, 256, 256, relu=2)]
        # stride 2: N 64 / 128, Cin 32 / 64, output rows 7 / 8
        R += [row(2, 33, 47, 64, 64, stride=2), row(2, 33, 47, 64, 128, stride=2), row(2, 33, 47, 32, 128, stride=2), row(2, 33, 47, 256, 512, stride=2, relu=1),
              row(2, 14, 64, 64, 128, stride=2), row(2, 16, 64, 64, 128, stride=2), row(2, 33, 47, 256, 512, stride=2, sw={"PT_CONV_PIPE": "0"}),
              row(2, 33, 47, 256, 512, stride=2, sw={"PT_CONV_PIPE": "1"}), row(2, 32, 48, 64, 128, stride=2, res=True), row(2, 33, 47, 64, 128, stride=2, relu=2),
              row(2, 33, 47, 64, 128, stride=2, split=1), row(2, 33, 47, 64, 64, stride=2, split=2)]
        # block tiles: maps of exactly 4 / 8 rows, W 32 / 64 / 96, Cin 96 / 128
        for H in (4, 8):
            for W in (32, 64, 96):
                R += [row(1, H, W, 96, 128), row(1, H, W, 128, 128)]
            R += [row(2, H, 64, 128, 128, sw={"PT_CONV_PIPE_BLOCKS": "0"}), row(2, H, 64, 128, 128, sw={"PT_CONV_PIPE": "0"}), row(2, H, 64, 128, 128, sw={"PT_CONV_PIPE": "2"}),
                  row(2, H, 64, 128, 64), row(2, H, 64, 256, 256, res=True), row(2, H, 64, 128, 128, split=1), row(2, H, 160, 256, 256, relu=1)]
        # the 4-row 4 x 64 patch of the chunk kernel (H <= 4, W > 32) and its neighbours
        R += [row(1, 4, 64, 64, 64), row(1, 3, 64, 64, 64), row(1, 4, 32, 64, 64), row(1, 5, 64, 64, 64), row(1, 3, 96, 64, 64, split=2), row(1, 3, 96, 64, 64, split=1)]
        # small 3x3 maps below every DMA threshold
        R += [row(1, 8, 32, 64, 64), row(1, 10, 40, 256, 256, relu=1), row(1, 10, 40, 256, 256, res=True, relu=1)]
        # 1x1 as a pipelined GEMM: Cin 480 / 512, N 64 / 128, rows % 32
        R += [row(1, 8, 32, 512, 128, ks=1), row(1, 8, 32, 480, 128, ks=1), row(1, 8, 32, 512, 64, ks=1), row(1, 9, 33, 512, 128, ks=1), row(1, 8, 32, 1024, 256, ks=1, relu=1),
              row(1, 8, 32, 512, 128, ks=1, sw={"PT_GEMM_PIPE": "0"}), row(1, 8, 32, 512, 128, ks=1, sw={"PT_GEMM_XP": "0"}), row(1, 8, 32, 512, 128, ks=1, res=True),
              row(1, 8, 32, 512, 128, ks=1, split=1), row(1, 8, 32, 512, 128, ks=1, ex=True, out_f32=True), row(1, 8, 32, 512, 128, ks=1, ex=True, ylimit=4),
              row(1, 8, 32, 512, 128, ks=1, ex=True, n_valid=72), row(1, 8, 32, 512, 256, ks=1, shuffle_cout=64)]
        # 1x1 wide: Cin 32 / 64 / 96 / 128 (KG and GEN), staged epilogues
        for Cin in (32, 64, 96, 128):
            R += [row(1, 9, 33, Cin, 64, ks=1), row(1, 9, 33, Cin, 64, ks=1, sw={"PT_CONV1_WIDE": "0"}), row(1, 9, 33, Cin, 64, ks=1, ex=True, ylimit=5),
                  row(1, 9, 33, Cin, 64, ks=1, ex=True, out_f32=True), row(1, 9, 33, Cin, 64, ks=1, ex=True, n_valid=8), row(1, 9, 33, Cin, 256, ks=1, shuffle_cout=64)]
        R += [row(1, 9, 33, 64, 64, ks=1, split=1), row(1, 9, 33, 64, 64, ks=1, split=2), row(1, 9, 33, 128, 128, ks=1, res=True, relu=1),
              row(1, 9, 33, 64, 64, ks=1, ex=True, out_f32=True, res_f32=True), row(1, 9, 33, 64, 64, ks=1, ex=True, ylimit=5, sw={"PT_CONV1_WIDE": "0"}),
              row(1, 9, 33, 64, 64, ks=1, sw={"PT_CONV_XP": "1"}), row(1, 9, 33, 128, 64, ks=1, ex=True, out_f32=True, res_f32=True, ylimit=5)]
        # 1x1 stride 2
        R += [row(2, 16, 32, 64, 64, ks=1, stride=2), row(2, 17, 33, 128, 256, ks=1, stride=2, relu=1), row(2, 16, 32, 64, 64, ks=1, stride=2, split=1),
              row(2, 16, 32, 64, 64, ks=1, stride=2, split=2)]
        return R
    # read-once settings: the layers whose choice they change
    conv3 = [row(2, 40, 40, 256, 256), row(2, 40, 40, 128, 128), row(9, 240, 240, 64, 64), row(1, 120, 64, 128, 128), row(1, 119, 64, 128, 128), row(1, 120, 64, 96, 128),
             row(2, 256, 256, 64, 256), row(32, 32, 32, 512, 512), row(2, 40, 40, 128, 128, split=1)]
    s2 = [row(2, 33, 47, 64, 128, stride=2), row(2, 33, 47, 256, 512, stride=2, relu=1)]
    blocks = [row(1, 4, 64, 128, 128), row(1, 8, 96, 128, 128)]
    one = [row(1, 8, 32, 512, 128, ks=1), row(1, 9, 33, 64, 64, ks=1), row(1, 9, 33, 128, 64, ks=1), row(1, 9, 33, 32, 64, ks=1), row(2, 16, 32, 64, 64, ks=1, stride=2)]
    small3 = [row(1, 8, 32, 64, 64), row(1, 4, 64, 64, 64), row(2, 33, 47, 64, 64, stride=2)]
    name = next(iter(group))
    if name == "PT_CONV_VARIANT":
        return conv3 + s2 + blocks
    if name == "PT_CONV_DMA":
        return conv3 + s2 + blocks + one
    if name == "PT_CONV_HALF":
        return conv3 + [row(2, 40, 40, 128, 128, sw={"PT_CONV_PIPE": pv}) for pv in "0135"] + [row(2, 40, 40, 256, 256, sw={"PT_CONV_PIPE": pv}) for pv in "0135"]
    if name == "PT_CONV_S2_DMA":
        return s2 + [row(2, 33, 47, 64, 128, stride=2, sw={"PT_CONV_PIPE": "0"})]
    if name == "PT_CONV1_DIRECT":
        return one + small3 + [row(1, 9, 33, 64, 64, ks=1, sw={"PT_CONV1_WIDE": "0"})]
    if name == "PT_N_GROUP":
        return one
    raise SystemExit(f"no rows for {group}")


GROUPS = [{}, {"PT_CONV_VARIANT": "0"}, {"PT_CONV_VARIANT": "1"}, {"PT_CONV_VARIANT": "2"}, {"PT_CONV_DMA": "0"}, {"PT_CONV_HALF": "0"}, {"PT_CONV_HALF": "1"},
          {"PT_CONV_S2_DMA": "0"}, {"PT_CONV1_DIRECT": "0"}, {"PT_N_GROUP": "0"}]


def group_name(g):
    return ",".join(f"{k}={v}" for k, v in g.items()) or "-"


def run(group, out_path):
    for k in PER_CALL + ONCE:
        os.environ.pop(k, None)
    os.environ.update(group)
    import torch
    from pdf_table_amd.engine import HipEngine
    eng = HipEngine(0)
    dev = torch.device("cuda", 0)
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = grid(group)
    with open(out_path, "w") as f:
        for r in rows:
            s, ex = r["shape"], r["extra"]
            split = int(ex.get("split", 0))
            m = 2 if split else 1
            taps = s["ks"] ** 2
            Ho = (s["H"] + 2 * (s["ks"] // 2) - s["ks"]) // s["stride"] + 1
            Wo = (s["W"] + 2 * (s["ks"] // 2) - s["ks"]) // s["stride"] + 1
            # the values do not matter to the choice: small random activations, zero weight tiles of the mode's size
            x = (torch.randn(s["B"], s["H"], s["W"], s["Cin"] * m, device=dev) * 0.1).to(eng.act_dtype)
            wt = torch.zeros(s["N"] * s["Cin"] * taps * (3 if split == 1 else 2 if split == 2 else 1), dtype=torch.int16, device=dev)
            bias = torch.zeros(s["N"], device=dev)
            for k in PER_CALL:
                os.environ.pop(k, None)
            os.environ.update(r["switches"])
            shape = dict(s)
            eng.profile_enable(1)
            if ex.get("ex"):
                yl = torch.tensor([ex["ylimit"]], dtype=torch.int32, device=dev) if "ylimit" in ex else None
                rf = torch.zeros(s["B"], s["H"], s["W"], ex.get("n_valid") or s["N"], device=dev) if ex.get("res_f32") else None
                eng.op_conv1x1_ex(x, wt, bias, relu=int(ex.get("relu", 0)), out_f32=bool(ex.get("out_f32")), n_valid=int(ex.get("n_valid", 0)), res_f32=rf, ylimit=yl)
                shape.update(relu=int(ex.get("relu", 0)), n_valid=int(ex.get("n_valid", 0)), has_out_f32=bool(ex.get("out_f32")), has_res_f32=rf is not None,
                             has_ylimit=yl is not None)
            else:
                rep, sh = int(ex.get("rep", 1)), int(ex.get("shuffle_cout", 0))
                res = torch.zeros(s["B"], Ho, Wo, s["N"] * m, dtype=eng.act_dtype, device=dev) if ex.get("res") else None
                eng.op_conv2d(x, wt, bias, s["ks"], s["stride"], relu=int(ex.get("relu", 0)), res=res, res_mode=1 if res is not None else 0, rep=rep, shuffle_cout=sh,
                              split=split)
                shape.update(relu=int(ex.get("relu", 0)), has_res=res is not None, res_mode=1 if res is not None else 0, rep=rep, shuffle_cout=sh, split=split)
            torch.cuda.synchronize()
            labels = eng.profile_read_labels()
            eng.profile_enable(False)
            assert len(labels) == 1 and next(iter(labels.values()))["launches"] == 1, (r, labels)
            sw = dict(group)
            sw.update(r["switches"])
            f.write(json.dumps(dict(shape=shape, switches=sw, num_cu=num_cu, label=next(iter(labels)))) + "\n")
    eng.close()
    print(f"{group_name(group)}: {len(rows)} rows -> {out_path}")


def names(out_path, trace_csv):
    with open(out_path) as f:
        rows = [json.loads(ln) for ln in f if ln.strip()]
    with open(trace_csv, newline="") as f:
        recs = sorted((r for r in csv.DictReader(f)), key=lambda r: int(r["Start_Timestamp"]))
    ks = []
    for r in recs:
        m = re.match(r"(?:void )?pt_bf16::(.+?)\(", r["Kernel_Name"])
        if m:
            ks.append(m.group(1))
    if len(ks) != len(rows):
        raise SystemExit(f"{trace_csv}: {len(ks)} pt_bf16 kernels in the trace, {len(rows)} rows in {out_path}: not pairing them")
    with open(out_path, "w") as f:
        for r, k in zip(rows, ks):
            r["kernel"] = k
            f.write(json.dumps(r) + "\n")
    print(f"{out_path}: {len(rows)} kernel names")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "groups":
        print("\n".join(group_name(g) for g in GROUPS))
    elif len(sys.argv) == 4 and sys.argv[1] == "run":
        run({} if sys.argv[2] == "-" else dict(kv.split("=") for kv in sys.argv[2].split(",")), sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "names":
        names(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
