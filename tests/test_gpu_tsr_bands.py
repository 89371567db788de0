"""pt_tsr_warp_forward_decode: the DLA-34 detector's front segment (base_layer .. level2) on the row bands letterboxed crops fill, against the two
calls it replaces (pt_tsr_preprocess + pt_tsr_forward_decode, PT_TSR_BANDS=0 in TsrStage): `counts`, `dets`, `logi` and the assembled level-2 map
(`layers[2]`, pt_op_tsr_level2) must be the same bits.

Every value of the banded path is produced by the kernels of the full path from the same neighbourhood: a kept row of the level-2 map lies at least
the receptive-field radius R inside its band, every other row is what the same kernels give for an all-padding table at the same map position.  So
the comparison is exact, in every storage mode.

Inputs are small: 256 x 256 (level-2 map 64 x 64), where the only window that keeps 64 rows off the map's top and bottom is [64, 192) -- 128 rows --
and 320 x 256 for a 192-row window [64, 256).  The pages are uniform noise, so a crop is noise up to its first and last row: the worst case for the
band's border.  Batches mix banded, near-square and tall crops; a lowered stack cap (PT_TSR_BAND_STACK_ROWS) splits seven bands into four stacks;
PT_CONV_WS64=2 puts the 64 -> 64 layers on the weight-stationary kernel the benchmark's batches take."""
import numpy as np
import pytest
import torch

from pdf_table_amd import lib as L
from pdf_table_amd.engine import TSR_TABLE_DTYPE
from pdf_table_amd.tsr_stage import lore_geometry

pytestmark = pytest.mark.gpu

PAGE = 512
MODES = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "pair": L.PT_PRECISION_BF16X3, "pair_f16x2": L.PT_PRECISION_F16X2}


@pytest.fixture(scope="module")
def engines():
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_weights import lore_dla34_state_dict
    from pdf_table_amd.weights import pack_lore_dla34
    sd = lore_dla34_state_dict(seed=2, hm_bias=(-1.2, -0.6))      # head biases near the thresholds: cells and corners on noise input
    es = {}
    for fmt in ("bf16", "f16"):
        e = HipEngine(0)
        e.load_weights(L.PT_MODEL_LORE_DLA34, pack_lore_dla34(sd, fmt=fmt))
        es[fmt] = e
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def pages():
    g = torch.Generator().manual_seed(123)
    return torch.randint(0, 256, (3, PAGE, PAGE, 3), generator=g, dtype=torch.uint8).cuda()


def _table(page, x0, y0, cw, ch, inp_h, inp_w):
    minv, _ = lore_geometry(ch, cw, inp_h, inp_w)
    r = np.zeros((), dtype=TSR_TABLE_DTYPE)
    r["minv"], r["page"], r["x0"], r["y0"], r["crop_w"], r["crop_h"] = minv.reshape(6), page, x0, y0, cw, ch
    return r


def _tables(crops, inp_h, inp_w):
    return np.array([_table(i % 3, 3 + 2 * i, 5 + 3 * i, cw, ch, inp_h, inp_w) for i, (cw, ch) in enumerate(crops)], dtype=TSR_TABLE_DTYPE)


# name: (inp_h, inp_w, crops (w, h), environment, expected `full` flags, expected window rows of the banded ones, expected stacks)
CASES = {
    "window_128": (256, 256, [(500, 70)], {}, [0], [128], 1),
    "window_192": (320, 256, [(500, 180)], {}, [0], [192], 1),
    "mixed": (256, 256, [(500, 70), (300, 280), (120, 400), (480, 60), (400, 50)], {}, [0, 1, 1, 0, 0], [128, 128, 128], 1),
    "seven_bands_four_stacks": (256, 256, [(500, 70), (480, 60), (400, 50), (500, 40), (450, 66), (495, 75), (300, 30)],
                                {"PT_TSR_BAND_STACK_ROWS": "256"}, [0] * 7, [128] * 7, 4),
    "mixed_weight_stationary": (256, 256, [(500, 70), (300, 280), (480, 60)], {"PT_CONV_WS64": "2"}, [0, 1, 0], [128, 128], 1),
}


def _engine(engines, mode):
    e = engines["f16" if mode == "f16" else "bf16"]
    e.set_precision(MODES[mode])
    return e


def _two_calls(e, pages, tb, inp_h, inp_w):
    x = e.tsr_preprocess(pages, tb, inp_h, inp_w, bgr=True)
    c, d, l = e.tsr_forward_decode(x, wiz_rev=True, vis_thresh=0.2, sync=True)
    return np.asarray(c).copy(), d.cpu().numpy(), l.cpu().numpy()


def _one_call(e, pages, tb, inp_h, inp_w):
    c, d, l = e.tsr_warp_forward_decode(pages, tb, inp_h, inp_w, bgr=True, wiz_rev=True, vis_thresh=0.2, sync=True)
    return np.asarray(c).copy(), d.cpu().numpy(), l.cpu().numpy()


def _same_results(on, off, what):
    c1, d1, l1 = on
    c0, d0, l0 = off
    print(f"{what}: cells per table {c0.tolist()}")
    assert np.array_equal(c0, c1), (what, c0, c1)
    assert c0.sum() > 0, what
    for b in range(len(c0)):          # rows beyond a table's count are not part of the result
        k = int(c0[b])
        assert np.array_equal(d0[b, :k].view(np.int32), d1[b, :k].view(np.int32)), (what, b)
        assert np.array_equal(l0[b, :k].view(np.int32), l1[b, :k].view(np.int32)), (what, b)


# (the weight-stationary kernel is a single-pass kernel: no pair-mode case of it)
@pytest.mark.parametrize("case,mode", [(c, m) for c in CASES for m in MODES if not (m.startswith("pair") and "PT_CONV_WS64" in CASES[c][3])])
def test_bands_on_and_off_agree_bit_for_bit(engines, pages, case, mode, monkeypatch):
    inp_h, inp_w, crops, env, full, rows, stacks = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _engine(engines, mode)
    try:
        tb = _tables(crops, inp_h, inp_w)
        plan, ns, frac = e.tsr_plan_bands(tb, inp_h, inp_w, int(env.get("PT_TSR_BAND_STACK_ROWS", "0")))
        assert plan[:, 0].tolist() == full and ns == stacks, plan
        assert [int(p[2] - p[1]) for p in plan if not p[0]] == rows, plan
        on = _one_call(e, pages, tb, inp_h, inp_w)
        off = _two_calls(e, pages, tb, inp_h, inp_w)
        m1 = e.op_tsr_level2(pages, tb, inp_h, inp_w, bands=True).cpu().view(torch.int16).numpy()
        m0 = e.op_tsr_level2(pages, tb, inp_h, inp_w, bands=False).cpu().view(torch.int16).numpy()
        again = _one_call(e, pages, tb, inp_h, inp_w)          # the cached all-padding map, used a second time
    finally:
        e.set_precision(L.PT_PRECISION_BF16)
    what = f"[{mode}] {case} (rows planned {frac:.3f})"
    assert m0.shape == (len(crops), inp_h // 4, inp_w // 4, 128 if mode.startswith("pair") else 64)
    diff = np.nonzero((m1 != m0).any(axis=(2, 3)))
    assert np.array_equal(m1, m0), (what, "level-2 rows that differ (table, row):", list(zip(*diff))[:20])
    assert len(np.unique(m0[0])) > 100, what
    _same_results(on, off, what)
    _same_results(again, off, what + " again")


@pytest.mark.parametrize("mode", list(MODES))
def test_a_margin_below_the_radius_shows(engines, pages, mode):
    """the hook planned with a margin of 8 rows in place of R = 19: level-2 rows 9 .. 19 input rows from the content come from the all-padding map
    although they see the noise -- the comparison above can fail"""
    e = _engine(engines, mode)
    try:
        R = e.tsr_band_radius()
        tb = _tables([(500, 70), (480, 60)], 256, 256)
        m0 = e.op_tsr_level2(pages, tb, 256, 256, bands=False).cpu().view(torch.int16).numpy()
        m8 = e.op_tsr_level2(pages, tb, 256, 256, bands=True, margin=8).cpu().view(torch.int16).numpy()
        mr = e.op_tsr_level2(pages, tb, 256, 256, bands=True, margin=R).cpu().view(torch.int16).numpy()
    finally:
        e.set_precision(L.PT_PRECISION_BF16)
    assert R == 19 and np.array_equal(mr, m0)
    rows = np.nonzero((m8 != m0).any(axis=(2, 3)))
    print(f"[{mode}] margin 8: level-2 (table, row) pairs that differ: {list(zip(*rows))}")
    assert len(rows[0]) > 0 and set(rows[0].tolist()) == {0, 1}


def test_reloaded_weights_rebuild_the_padding_map(pages):
    from pdf_table_amd.engine import HipEngine
    from pdf_table_amd.synth_weights import lore_dla34_state_dict
    from pdf_table_amd.weights import pack_lore_dla34
    e = HipEngine(0)
    try:
        tb = _tables([(500, 70), (300, 280), (480, 60)], 256, 256)
        for seed in (2, 4):
            e.load_weights(L.PT_MODEL_LORE_DLA34, pack_lore_dla34(lore_dla34_state_dict(seed=seed, hm_bias=(-1.2, -0.6))))
            m1 = e.op_tsr_level2(pages, tb, 256, 256, bands=True).cpu().view(torch.int16).numpy()
            m0 = e.op_tsr_level2(pages, tb, 256, 256, bands=False).cpu().view(torch.int16).numpy()
            assert np.array_equal(m1, m0), seed
            _same_results(_one_call(e, pages, tb, 256, 256), _two_calls(e, pages, tb, 256, 256), f"seed {seed}")
    finally:
        e.close()


def test_stage_switch(engines, pages, monkeypatch):
    """TsrStage.start takes the one call by default and the two calls with PT_TSR_BANDS=0 (read per call): same tables out"""
    from pdf_table_amd.tsr_stage import LoreConfig, TsrStage
    e = _engine(engines, "bf16")
    cfg = LoreConfig(task_type="wtw")
    cfg.resolution = (256, 256)
    st = TsrStage(e, cfg, micro_batch=2, with_html=False)
    tb = _tables([(500, 70), (300, 280), (480, 60)], 256, 256)
    calls = []
    real = e.tsr_warp_forward_decode
    monkeypatch.setattr(e, "tsr_warp_forward_decode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = []
    for sw in ("1", "0"):
        monkeypatch.setenv("PT_TSR_BANDS", sw)
        (i, nt, counts, dets, logi, host, ev), = st.start(pages, tb)
        ev.synchronize()
        res.append((host.numpy().copy(), dets.cpu().numpy(), logi.cpu().numpy()))
    assert len(calls) == 2          # two micro-batches, with the switch on only
    _same_results(res[0], res[1], "stage")
