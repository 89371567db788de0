"""Row bands of the DLA-34 detector's front segment (pt_tsr_plan_bands, csrc/lore_model.hip): the planner on hand-made tables, and the receptive-field
radius it plans with against the fp32/fp64 oracle net.

A crop wider than high fills only the middle rows of the detector's input.  The planner gives, per table, the input rows [row0, row1) the front
segment (base_layer .. level2) has to see -- content +- 2, widened by twice the radius R, aligned outwards to 64 -- and the rows [keep0, keep1) of
the stride-4 level-2 map that are taken from the band; every other row of that map comes from the map of an all-padding table."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.engine import TSR_TABLE_DTYPE
from pdf_table_amd.tsr_stage import lore_geometry

ALIGN, SLACK = 64, 2


def _lib():
    return L.load()


def _radius():
    return int(_lib().pt_tsr_band_radius())


def _table(crop_w, crop_h, inp_h, inp_w, upper_left=False, page=0, x0=0, y0=0):
    minv, _ = lore_geometry(crop_h, crop_w, inp_h, inp_w, upper_left)
    r = np.zeros((), dtype=TSR_TABLE_DTYPE)
    r["minv"], r["page"], r["x0"], r["y0"], r["crop_w"], r["crop_h"] = minv.reshape(6), page, x0, y0, crop_w, crop_h
    return r


def _plan(tables, inp_h, inp_w, cap=0):
    import ctypes as C
    tb = np.ascontiguousarray(np.array(tables, dtype=TSR_TABLE_DTYPE))
    out = np.zeros((len(tb), 8), np.int32)
    ns, frac = C.c_int(-1), C.c_double(-1.0)
    L.check(_lib().pt_tsr_plan_bands(tb.ctypes.data, len(tb), inp_h, inp_w, cap, out.ctypes.data, C.byref(ns), C.byref(frac)), "pt_tsr_plan_bands")
    keys = ("full", "row0", "row1", "keep0", "keep1", "stack", "stack_row")
    return [dict(zip(keys, (int(v) for v in row[:7]))) for row in out], ns.value, frac.value


def _content_rows(t, inp_h):
    """first and last destination row with a source row inside the crop: tsr_preprocess_kernel's fixed-point arithmetic in Python integers"""
    def sat(v):
        return int(min(max(np.rint(v), -2147483648.0), 2147483647.0))
    rows = []
    for y in range(inp_h):
        Y = (sat((t["minv"][4] * y + t["minv"][5]) * 1024.0) + 16) >> 5
        sy = Y >> 5
        if sy + 1 >= 0 and sy < int(t["crop_h"]):
            rows.append(y)
    return rows[0], rows[-1]


def test_radius_is_derived_from_the_layer_list():
    # 7x7; 3x3; 3x3 s2; 3x3 s2 on the half-size map; three 3x3 on the quarter-size map: 3 + 1 + 1 + 2 + 3 * 4
    assert _radius() == 19


@pytest.mark.parametrize("cw,ch,inp", [(900, 300, 1024), (1000, 240, 1024), (731, 333, 1024), (640, 333, 512), (1000, 150, 256), (900, 150, 256)])
def test_window_alignment_containment_and_kept_rows(cw, ch, inp):
    R = _radius()
    t = _table(cw, ch, inp, inp)
    (b,), ns, frac = _plan([t], inp, inp)
    c0, c1 = _content_rows(t, inp)
    print(f"{cw}x{ch} @ {inp}: content rows {c0}..{c1}, plan {b}, fraction {frac:.3f}")
    assert b["full"] == 0 and ns == 1 and b["stack"] == 0 and b["stack_row"] == 0
    assert b["row0"] % ALIGN == 0 and b["row1"] % ALIGN == 0
    assert ALIGN <= b["row0"] and b["row1"] <= inp - ALIGN
    # the window holds content +- (2 R + 2), and no more than the alignment asks for
    assert b["row0"] <= c0 - (2 * R + SLACK) and b["row1"] >= c1 + 1 + (2 * R + SLACK)
    assert b["row0"] > c0 - (2 * R + SLACK) - ALIGN and b["row1"] < c1 + 1 + (2 * R + SLACK) + ALIGN
    # kept rows: exactly the map rows whose receptive field [4 r - R, 4 r + R] meets content +- 2 ...
    want = [r for r in range(inp // 4) if 4 * r + R >= c0 - SLACK and 4 * r - R <= c1 + SLACK]
    assert (b["keep0"], b["keep1"]) == (want[0], want[-1] + 1)
    # ... each with its whole receptive field inside the window (so at least R from the seams)
    assert 4 * b["keep0"] - R >= b["row0"] and 4 * (b["keep1"] - 1) + R <= b["row1"] - 1
    assert frac == pytest.approx((b["row1"] - b["row0"]) / inp)


def test_every_full_rule():
    inp = 1024
    wide = _table(900, 300, inp, inp)
    cases = {
        "square": _table(500, 500, inp, inp),
        "tall": _table(300, 900, inp, inp),
        "upper_left": _table(900, 300, inp, inp, upper_left=True),
        "near_the_border": _table(1000, 800, inp, inp),      # content rows 102 .. 921: the window would start above row 64
    }
    rot = wide.copy()
    rot["minv"][1] = 1e-3
    cases["rotation_term"] = rot
    shear = wide.copy()
    shear["minv"][3] = -1e-3
    cases["shear_term"] = shear
    bands, ns, frac = _plan(list(cases.values()) + [wide], inp, inp)
    for name, b in zip(cases, bands):
        assert b["full"] == 1 and (b["row0"], b["row1"], b["keep0"], b["keep1"], b["stack"]) == (0, inp, 0, inp // 4, -1), name
    assert bands[-1]["full"] == 0 and ns == 1
    # the first and the last window that still fit: [64, inp - 64) exactly
    R = _radius()
    for ch in range(700, 900):
        t = _table(1000, ch, inp, inp)
        c0, c1 = _content_rows(t, inp)
        fits = c0 - (2 * R + SLACK) >= ALIGN and c1 + 1 + (2 * R + SLACK) <= inp - ALIGN
        (b,), _, _ = _plan([t], inp, inp)
        assert b["full"] == (0 if fits else 1), (ch, c0, c1, b)
    # an input height that is no multiple of the alignment runs in full
    (b,), _, _ = _plan([_table(900, 100, 288, 288)], 288, 288)
    assert b["full"] == 1


def test_stack_cap():
    inp = 1024
    tabs = [_table(900, 200 + 10 * i, inp, inp) for i in range(7)]
    free, ns1, f1 = _plan(tabs, inp, inp)
    rows = [b["row1"] - b["row0"] for b in free]
    assert ns1 == 1 and [b["stack_row"] for b in free] == list(np.cumsum([0] + rows[:-1]))
    cap = 2 * max(rows)
    capped, ns2, f2 = _plan(tabs, inp, inp, cap=cap)
    assert ns2 > 1 and f1 == f2
    used = {}
    for b, c in zip(free, capped):
        assert (c["row0"], c["row1"], c["keep0"], c["keep1"]) == (b["row0"], b["row1"], b["keep0"], b["keep1"])
        assert c["stack_row"] == used.get(c["stack"], 0)          # bands lie one under the other, in table order
        used[c["stack"]] = c["stack_row"] + c["row1"] - c["row0"]
    assert sorted(used) == list(range(ns2)) and max(used.values()) <= cap
    assert [c["stack"] for c in capped] == sorted(c["stack"] for c in capped)
    # a window larger than the cap cannot be stacked: the table runs in full
    small, ns3, _ = _plan(tabs, inp, inp, cap=min(rows) - ALIGN)
    assert all(b["full"] == 1 for b in small) and ns3 == 0
    # the default cap, and anything above it, is 32768 rows
    many = [_table(900, 400, inp, inp)] * 80
    a, nsa, _ = _plan(many, inp, inp)
    b, nsb, _ = _plan(many, inp, inp, cap=1 << 30)
    assert a == b and nsa == nsb == 2 and max(x["stack_row"] + x["row1"] - x["row0"] for x in a) <= 32768


def test_fraction_on_the_benchmark_generator_rectangles():
    """the 87 table rectangles of the benchmark's 64 synthetic pages, grown by 8 px like bench.py does"""
    from pdf_table_amd.synth_pages import make_page
    PAGE = 1024
    tabs = []
    for i in range(64):
        t = make_page(i, PAGE)[1]["tables"].astype(np.int64).reshape(-1, 4)
        for x1, y1, x2, y2 in t:
            x1, y1, x2, y2 = max(x1 - 8, 0), max(y1 - 8, 0), min(x2 + 8, PAGE), min(y2 + 8, PAGE)
            tabs.append(_table(int(x2 - x1), int(y2 - y1), 1024, 1024, page=i, x0=int(x1), y0=int(y1)))
    bands, ns, frac = _plan(tabs, 1024, 1024)
    nfull = sum(b["full"] for b in bands)
    print(f"{len(tabs)} tables, {nfull} in full, {ns} stacks, fraction of rows planned {frac:.4f}")
    assert len(tabs) == 87 and ns == PIN_STACKS
    assert nfull == PIN_FULL and frac == pytest.approx(PIN_FRACTION, abs=5e-5)
    assert frac == pytest.approx(sum(b["row1"] - b["row0"] for b in bands) / (87 * 1024))


PIN_FULL, PIN_STACKS, PIN_FRACTION = 1, 2, 0.5970      # (87 windows of about 600 rows pass the 32768-row cap once)


def test_radius_against_the_oracle_net():
    """the oracle's DLA base (fp64) at 256 x 256: an all-padding input against the same input with uniform noise in rows y0 .. y1.  Row r of the level-2
    map reads input rows 4 r - R .. 4 r + R: it must be unchanged where that misses the band, and changed where it touches the band's edge row only."""
    from oracle.lore_net import dla34_forward
    from pdf_table_amd.synth_weights import lore_dla34_state_dict
    R = _radius()
    sd = {k: v.double() for k, v in lore_dla34_state_dict(seed=3).items() if k.startswith("base.") and v.is_floating_point()}
    sd.update({k: v for k, v in lore_dla34_state_dict(seed=3).items() if k.startswith("base.") and not v.is_floating_point()})
    H = W = 256
    y0, y1 = 99, 141                      # 4 * 20 + R == y0 and 4 * 40 - R == y1: rows 20 and 40 touch the band with their outermost input row
    pad = torch.tensor([(0.0 - m) / s for m, s in zip((0.408, 0.447, 0.470), (0.289, 0.274, 0.278))], dtype=torch.float64)
    a = pad.view(1, 3, 1, 1).expand(1, 3, H, W).clone()
    b = a.clone()
    g = torch.Generator().manual_seed(5)
    b[:, :, y0:y1 + 1] = torch.rand(1, 3, y1 - y0 + 1, W, generator=g, dtype=torch.float64) * 4.0 - 2.0
    with torch.no_grad():
        la, lb = dla34_forward(sd, a)[2], dla34_forward(sd, b)[2]
    assert la.shape == (1, 64, H // 4, W // 4)
    changed = (la != lb).any(3).any(1)[0].numpy()                      # per map row
    rows = np.nonzero(changed)[0]
    print(f"R = {R}: level-2 rows that see the noise: {rows[0]} .. {rows[-1]}")
    assert 4 * 20 + R == y0 and 4 * 40 - R == y1
    assert rows[0] == 20 and rows[-1] == 40 and changed[20:41].all()
    assert not changed[:20].any() and not changed[41:].any()
