"""The MtlTabNet decoders' attention kernels (csrc/mtl_decoder.hip) one at a time, through pt_op_mtl_cross_attention / self_attention / kv_fp8 -- the
launch functions of the decoding loops -- against the float64 references of tests/mtl_attn_ref.py (tied to the oracle by tests/test_mtl_attn_host.py).
No model is loaded and no network runs.  The shapes sit at the seams of the key loops (64-key chunks, 128 in the e4m3 kernel, 32-key MFMA tiles) and of
the key slices, not at production size.

Every operand is generated already rounded to the storage format, so the reference reads what the kernel reads.  Every launch carries all score
patterns, one per head (mtl_attn_ref.HEAD_PATTERNS): random, a key that dominates by >= 20 at key 0 / the end of the first chunk / the start of the
last slice / key hw - 1, all scores equal, scores spread over +-80, wide random.  The bounds are stated with the references; every test prints its worst
error / tolerance ratio.

Worst error / tolerance measured on an MI355X when the tests were written (bf16, f16, BF16X3; in the single-pass modes the store's half-ulp is most of
the bound, so a correct kernel sits just under 1): stream 0.975 / 0.990 / 0.374, one slice against slices 0.000 / 0.478 / 0.131; stream8 0.995 / 0.987;
pair mode 0.972 / 0.973 / 0.354 (stream8 0.958 / 0.962); mfma 0.975 / 0.668 / 0.133, cell layout 0.857 / 0.752 / 0.114; self attention 0.996 / 0.992 /
0.427, pair mode 0.996 / 0.995 / 0.431; the e4m3 copy is bit-exact.

What test_stream_kernels_against_fp64 catches, checked by breaking mtl_cross_decode_kernel on a scratch copy (none of these reads or writes out of
bounds): the accumulator not rescaled by e^(m - mn) (first failure at hw 65, one slice: error 4.2 where the key of the second chunk dominates); hw
in place of kend in the key clamp and tail mask (hw 200, three slices); the slice maximum written before the stream merge (hw 65, two slices); no
tail mask (hw 7); slot (z R + qrow) + head without the x HEADS (the merge reads partials nobody wrote: NaN stored)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mtl_attn_ref as R  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MODES = {"bf16": L.PT_PRECISION_BF16, "f16": L.PT_PRECISION_F16, "bf16x3": L.PT_PRECISION_BF16X3}
ALL = ["bf16", "f16", "bf16x3"]
SINGLE = ["bf16", "f16"]
STREAM_CASES = [("stream", n) for n in ALL] + [("stream8", n) for n in SINGLE]      # the e4m3 kernel exists in the single-pass modes only
KERNEL = {"stream": L.PT_MTL_ATTN_STREAM, "stream8": L.PT_MTL_ATTN_STREAM8, "mfma": L.PT_MTL_ATTN_MFMA}
CHUNK = {"stream": 64, "stream8": 128, "mfma": 32}
SENTINEL = 7.5                       # exact in bf16 and f16
NT, MP = 3, 128                      # tables with different data; the row stride of a position
ONE_SLICE = [1, 7, 63, 64, 65, 129, 200]
SLICED = [(65, 64), (200, 96), (520, 128), (600, 96), (496, 32)]          # 2, 3, 5, 7 and 16 slices; last slices of 1, 8, 8, 24 and 16 keys


class Mode:
    def __init__(self, name, eng):
        self.name, self.eng = name, eng
        self.split = name == "bf16x3"
        self.dt = R.DT[R.fmt_of(name)]
        self.m = 2 if self.split else 1

    def put(self, v):
        """float64 values [.., C] already on the mode's grid -> the device tensor that holds them ([hi C | lo C] when split)"""
        if not self.split:
            t = v.to(self.dt)
            assert torch.equal(t.double(), v)
            return t.contiguous().to(DEV)
        hi, lo = R.split_pair(v)
        assert torch.equal(hi.double() + lo.double(), v)
        return torch.cat([hi, lo], -1).contiguous().to(DEV)

    def blank(self, *shape):
        return torch.full(shape[:-1] + (shape[-1] * self.m,), SENTINEL, dtype=self.dt, device=DEV)

    def get(self, t):
        t = t.cpu()
        assert bool(torch.isfinite(t.float()).all()), "Inf / NaN stored"
        if not self.split:
            return t.double()
        c = t.shape[-1] // 2
        return t[..., :c].double() + t[..., c:].double()


@pytest.fixture(scope="module")
def engines():
    from pdf_table_amd.engine import HipEngine
    made = {}

    def get(name):
        if name not in made:
            e = HipEngine(0)
            e.set_precision(MODES[name])
            made[name] = Mode(name, e)
            assert made[name].dt == e.act_dtype and made[name].split == e.split
        return made[name]
    yield get
    for m in made.values():
        m.eng.close()


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """a kernel fault poisons the process's context: end the session instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after an mtl attention op test, not continuing: {e}", returncode=3)


def _ratio(what, got, ref, tol):
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    i = int(r.flatten().argmax())
    worst = float(r.flatten()[i])
    assert worst <= 1.0, (f"{what}: {int((r > 1).sum())} of {r.numel()} values out of tolerance, worst err/tol {worst:.3f} "
                          f"(err {float(err.flatten()[i]):.3e} at ref {float(ref.flatten()[i]):.5g}, head {i % R.D // R.DK})")
    return worst


@functools.lru_cache(maxsize=4)
def _kv_case(hw, marks, mode, seed):
    """keys / values of NT tables with slots 0, 1, 3 and 4 planted (read-only: shared between tests)"""
    return R.cross_case(NT, hw, (0, 1, 3, 4), marks, mode, seed)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _cross(m, kind, kv_dev, n_tables, hw, slot, tiles, kps, nsplit, npos, M, q_vals, nb=1):
    """one pt_op_mtl_cross_attention call.  q_vals: nb tensors [npos * MP, 512].  -> (values [nb, npos * MP, 512], the raw output rows).
    The output starts as SENTINEL everywhere, the partials as NaN (a merge that read a slot nobody wrote would store it); the second layer of a
    pair sits behind strides that are not the buffer sizes."""
    rows = npos * MP
    row_bs = (rows + 8) * R.D * m.m
    opart_bs, ml_bs = nsplit * rows * R.D + 3 * R.D, nsplit * rows * 16 + 48
    q = m.blank(nb * (rows + 8), R.D)
    for b in range(nb):
        q[b * (rows + 8):b * (rows + 8) + rows] = m.put(q_vals[b])
    att = m.blank(nb * (rows + 8), R.D)
    opart = _nan(nb * opart_bs) if nsplit > 1 else None
    mlpart = _nan(nb * ml_bs) if nsplit > 1 else None
    m.eng.op_mtl_cross_attention(KERNEL[kind], q, kv_dev, n_tables, hw, slot, tiles, kps, nsplit, npos, M, MP, att, opart, mlpart, split=m.split, nb=nb,
                                 row_bs=row_bs if nb == 2 else 0, opart_bs=opart_bs if nb == 2 else 0, ml_bs=ml_bs if nb == 2 else 0)
    torch.cuda.synchronize()
    raw = att.cpu().reshape(nb, rows + 8, R.D * m.m)
    assert bool((raw[:, rows:].float() == SENTINEL).all()), "rows past the last position were written"
    return raw[:, :rows]


def _tile_rows(tiles):
    return [[t[1] + j * t[3] for j in range(t[2])] for t in tiles]


def _check_cross(m, what, kind, raw, kv_vals, hw, slot, tiles, kps, nsplit, q_vals, marks, want_patterns=True):
    """rows in the tiles against the reference of their table, within the bound; every other row still SENTINEL.  -> (worst ratio, got, refs)"""
    rows_used = sorted(r for tr in _tile_rows(tiles) for r in tr)
    mask = torch.ones(raw.shape[0], dtype=torch.bool)
    mask[rows_used] = False
    assert bool((raw[mask].float() == SENTINEL).all()), f"{what}: rows outside the tiles were written"
    got = m.get(raw)
    worst, refs = 0.0, {}
    for t, tr in zip(tiles, _tile_rows(tiles)):
        ref = R.cross_reference(q_vals[tr], kv_vals, hw, t[0], slot)
        if want_patterns:
            R.check_patterns(ref, marks)
        out = torch.stack([r["out"] for r, _ in ref], 1).reshape(len(tr), R.D)
        tol = torch.stack([R.attention_tol(r, v, kind, m.name, hw if nsplit == 1 else kps, nsplit, x3_products=m.split) for r, v in ref], 1).reshape(len(tr), R.D)
        worst = max(worst, _ratio(f"{what} table {t[0]}", got[tr], out, tol))
        refs[t[0]] = (ref, tr)
    return worst, got, refs


def _queries(us_slot, rows_of_table, npos, seed):
    """[npos * MP, 512] query rows: those of table b (rows_of_table[b]) look at table b's planted directions, every other row is noise"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(npos * MP, R.D, generator=g, dtype=torch.float64)
    for b, rows in rows_of_table.items():
        q[rows] = R.make_queries(len(rows), us_slot[b], g).reshape(len(rows), R.D)
    return q


def _grid(kind):
    one = ONE_SLICE + ([127, 128, 300] if kind == "stream8" else []) + ([33] if kind == "mfma" else [])
    return [(hw, (hw + 31) // 32 * 32, 1) for hw in one] + [(hw, kps, -(-hw // kps)) for hw, kps in SLICED]


# ---- the key-stream kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", STREAM_CASES)
def test_stream_kernels_against_fp64(engines, kind, name):
    """mtl_cross_decode_kernel<SPLIT> / mtl_cross_decode8_kernel + mtl_cross_combine_kernel: one query per table, three tables, one slice around
    the chunk length and 2 .. 16 slices with several chunks each and ragged last slices; layer slots 0 and 4.  Where both exist, the one-slice and
    the sliced result of the same operands agree within the fp32 terms of both plus the two stores.  The e4m3 kernel is compared with the reference on
    the decoded copy, which itself equals the reference round trip bit for bit."""
    m = engines(name)
    tiles = [(b, b, 1, MP) for b in range(NT)]
    worst = worst_ag = 0.0
    for i, (hw, kps, ns) in enumerate(_grid(kind)):
        slot = (0, 4)[i % 2]
        marks = R.seam_marks(hw, CHUNK[kind], kps, ns)
        kv_vals, us = _kv_case(hw, marks, name, 100 + hw)
        kv_dev = m.put(kv_vals)
        if kind == "stream8":
            kv_dev = m.eng.op_mtl_kv_fp8(kv_dev)
            want8 = R.e4m3_bytes(kv_vals)
            assert torch.equal(kv_dev.cpu(), want8), f"e4m3 copy hw={hw}"
            kv_vals = R.e4m3_decode(want8) / R.KV8_SCALE
        q = R.rnd(_queries(us[slot], {b: [b] for b in range(NT)}, 1, hw), name)
        what = f"{kind} hw={hw} kps={kps} nsplit={ns} slot={slot} [{name}]"
        raw = _cross(m, kind, kv_dev, NT, hw, slot, tiles, kps, ns, 1, NT, [q])[0]
        w, got, refs = _check_cross(m, what, kind, raw, kv_vals, hw, slot, tiles, kps, ns, q, marks)
        worst = max(worst, w)
        if ns > 1:
            kps1 = (hw + 31) // 32 * 32
            got1 = m.get(_cross(m, kind, kv_dev, NT, hw, slot, tiles, kps1, 1, 1, NT, [q])[0])
            for b, (ref, tr) in refs.items():
                out = torch.stack([r["out"] for r, _ in ref], 1).reshape(len(tr), R.D)
                tol = torch.stack([R.split_agreement_tol(r, v, kind, hw, kps, ns) for r, v in ref], 1).reshape(len(tr), R.D)
                tol = tol + 2 * R.U_OUT[name] * out.abs() + (2 * 2.0 ** -25 if name == "f16" else 0.0)
                worst_ag = max(worst_ag, _ratio(f"{what} vs one slice, table {b}", got[tr], got1[tr], tol))
    print(f"mtl {kind} [{name}]: worst err/tol {worst:.3f} over {len(_grid(kind))} shapes; one slice vs slices {worst_ag:.3f}")


@pytest.mark.parametrize("kind,name", STREAM_CASES)
def test_stream_pair_mode(engines, kind, name):
    """nb = 2: the structure-token and the box layer of a KV-cached step in the same launches -- a second set of queries behind row_bs, keys / values of
    the next slot, partials behind opart_bs / ml_bs.  Both layers against the reference, and each equal to its own single-layer call."""
    m = engines(name)
    tiles = [(b, b, 1, MP) for b in range(NT)]
    worst = 0.0
    for (hw, kps, ns), slot in (((65, 96, 1), 0), ((200, 96, 3), 3)):
        marks = R.seam_marks(hw, CHUNK[kind], kps, ns)
        kv_vals, us = _kv_case(hw, marks, name, 100 + hw)
        kv_dev = m.put(kv_vals)
        if kind == "stream8":
            kv_dev = m.eng.op_mtl_kv_fp8(kv_dev)
            kv_vals = R.e4m3_decode(R.e4m3_bytes(kv_vals)) / R.KV8_SCALE
        qs = [R.rnd(_queries(us[slot + b], {t: [t] for t in range(NT)}, 1, 7 * hw + b), name) for b in range(2)]
        raw = _cross(m, kind, kv_dev, NT, hw, slot, tiles, kps, ns, 1, NT, qs, nb=2)
        for b in range(2):
            what = f"{kind} pair layer {b} hw={hw} nsplit={ns} slot={slot + b} [{name}]"
            worst = max(worst, _check_cross(m, what, kind, raw[b], kv_vals, hw, slot + b, tiles, kps, ns, qs[b], marks)[0])
            alone = _cross(m, kind, kv_dev, NT, hw, slot + b, tiles, kps, ns, 1, NT, [qs[b]])[0]
            assert torch.equal(alone, raw[b]), what + ": differs from the single-layer call"
    print(f"mtl {kind} pair mode [{name}]: worst err/tol {worst:.3f}")


# ---- the MFMA kernel -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("cnt", [1, 5, 32])
def test_mfma_kernel_against_fp64(engines, cnt, name):
    """mtl_cross_attn_kernel<SPLIT> + mtl_cross_combine_kernel in the re-decode layout: `cnt` positions of each of three tables, rows position * 128 +
    table, one tile per table listed in the order 2, 0, 1; the stream kernels' grid of key counts and slices plus hw = 33 (one key in the second tile)."""
    m = engines(name)
    tiles = [(b, b, cnt, MP) for b in (2, 0, 1)]
    worst = 0.0
    for i, (hw, kps, ns) in enumerate(_grid("mfma")):
        slot = (4, 0)[i % 2]
        marks = R.seam_marks(hw, CHUNK["mfma"], kps, ns)
        kv_vals, us = _kv_case(hw, marks, name, 100 + hw)
        q = R.rnd(_queries(us[slot], {b: [b + j * MP for j in range(cnt)] for b in range(NT)}, cnt, hw + cnt), name)
        raw = _cross(m, "mfma", m.put(kv_vals), NT, hw, slot, tiles, kps, ns, cnt, NT, [q])[0]
        what = f"mfma queries={cnt} hw={hw} kps={kps} nsplit={ns} slot={slot} [{name}]"
        worst = max(worst, _check_cross(m, what, "mfma", raw, kv_vals, hw, slot, tiles, kps, ns, q, marks)[0])
    print(f"mtl mfma queries={cnt} [{name}]: worst err/tol {worst:.3f} over {len(_grid('mfma'))} shapes")


@pytest.mark.parametrize("name", ALL)
def test_mfma_kernel_cell_layout(engines, name):
    """the cell decoder's tiles: 1, 5 and 32 cells of three tables side by side in ONE position (row stride 1, 38 sequences), one slice and three"""
    m = engines(name)
    tiles = [(1, 1, 5, 1), (2, 6, 32, 1), (0, 0, 1, 1)]
    worst = 0.0
    for hw, kps, ns in ((33, 64, 1), (200, 96, 3)):
        marks = R.seam_marks(hw, 32, kps, ns)
        kv_vals, us = _kv_case(hw, marks, name, 100 + hw)
        q = R.rnd(_queries(us[1], {0: [0], 1: list(range(1, 6)), 2: list(range(6, 38))}, 1, 3 * hw), name)
        raw = _cross(m, "mfma", m.put(kv_vals), NT, hw, 1, tiles, kps, ns, 1, 38, [q])[0]
        worst = max(worst, _check_cross(m, f"mfma cells hw={hw} nsplit={ns} [{name}]", "mfma", raw, kv_vals, hw, 1, tiles, kps, ns, q, marks)[0])
    print(f"mtl mfma cell layout [{name}]: worst err/tol {worst:.3f}")


# ---- exact properties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", STREAM_CASES + [("mfma", n) for n in ALL])
def test_a_table_does_not_depend_on_the_other_tables(engines, kind, name):
    """table 1 of a three-table call == the same queries over a tensor that holds table 1 alone, bit for bit, with one slice and with three"""
    m = engines(name)
    cnt = 5 if kind == "mfma" else 1
    for hw, kps, ns in ((65, 96, 1), (200, 96, 3)):
        marks = R.seam_marks(hw, CHUNK[kind], kps, ns)
        kv_vals, us = _kv_case(hw, marks, name, 100 + hw)
        kv3, kv1 = m.put(kv_vals), m.put(kv_vals[hw:2 * hw])
        if kind == "stream8":
            kv3, kv1 = m.eng.op_mtl_kv_fp8(kv3), m.eng.op_mtl_kv_fp8(kv1)
        q3 = R.rnd(_queries(us[0], {b: [b + j * MP for j in range(cnt)] for b in range(NT)}, cnt, hw), name)
        q1 = torch.zeros_like(q3)
        q1[[j * MP for j in range(cnt)]] = q3[[1 + j * MP for j in range(cnt)]]
        all3 = _cross(m, kind, kv3, NT, hw, 0, [(b, b, cnt, MP) for b in range(NT)], kps, ns, cnt, NT, [q3])[0]
        alone = _cross(m, kind, kv1, 1, hw, 0, [(0, 0, cnt, MP)], kps, ns, cnt, 1, [q1])[0]
        assert torch.equal(all3[[1 + j * MP for j in range(cnt)]], alone[[j * MP for j in range(cnt)]]), (kind, name, hw, ns)


@pytest.mark.parametrize("name", ALL)
def test_kv_fp8_copy_is_the_reference_round_trip(engines, name):
    """mtl_kv_fp8_kernel over every finite 16-bit pattern of the format (saturation at both ends, the e4m3 subnormals, every tie of the grid, signed
    zeros) plus a ragged tail: 65536 + 8 * 37 values, so the last workgroup is partial; bytes past n_elems keep their sentinel"""
    m = engines(name)
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(m.dt)
    pats = torch.where(torch.isfinite(pats.float()), pats, torch.zeros_like(pats))
    g = torch.Generator().manual_seed(8)
    vals = torch.cat([pats, torch.randn(8 * 37, generator=g).to(m.dt)])
    out = torch.full((vals.numel() + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    m.eng.op_mtl_kv_fp8(vals.to(DEV), out=out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[vals.numel():] == 0xA5).all()), "bytes past n_elems were written"
    want = R.e4m3_bytes(vals.double())
    bad = (got[:vals.numel()] != want).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} bytes differ, first at value {float(vals[bad[0]])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}"
    assert {int(b) for b in want.unique()} >= set(range(0, 127)) | set(range(128, 255))       # the whole grid is reached


# ---- self attention --------------------------------------------------------------------------------------------------------------------------------
def _self(m, cache_vals, tok, pad, p0, p1, M, nb=1):
    L = p1 + 1
    npos = p1 - p0 + 1
    cache_bs, att_bs = (L * MP + 3) * 3 * R.D * m.m, (npos * MP + 5) * R.D * m.m
    cache = m.blank(nb * (L * MP + 3), 3 * R.D)
    for b in range(nb):
        cache[b * (L * MP + 3):b * (L * MP + 3) + L * MP] = m.put(cache_vals[b].reshape(L * MP, 3 * R.D))
    att = m.blank(nb * (npos * MP + 5), R.D)
    m.eng.op_mtl_self_attention(cache, tok.to(torch.int32).contiguous().to(DEV), pad, p0, p1, MP, M, att, split=m.split, nb=nb,
                                cache_bs=cache_bs if nb == 2 else 0, att_bs=att_bs if nb == 2 else 0)
    torch.cuda.synchronize()
    raw = att.cpu().reshape(nb, npos * MP + 5, R.D * m.m)
    assert bool((raw[:, npos * MP:].float() == SENTINEL).all()), "rows past the last position were written"
    raw = raw[:, :npos * MP].reshape(nb, npos, MP, R.D * m.m)
    assert bool((raw[:, :, M:].float() == SENTINEL).all()), "rows of sequences >= M were written"
    return m.get(raw[:, :, :M])


def _check_self(m, what, got, cache_vals, tok, pad, p0, p1, M):
    worst = 0.0
    for p in range(p0, p1 + 1):
        for s in range(M):
            ref = R.self_reference(cache_vals, tok, pad, p, s)
            nk = p1 + 1 if int(tok[p, s]) == pad else p + 1
            out = torch.cat([r["out"][0] for r, _ in ref])
            tol = torch.cat([R.attention_tol(r, v, "self", m.name, nk, 1)[0] for r, v in ref])
            worst = max(worst, _ratio(f"{what} position {p} sequence {s}", got[p - p0, s], out, tol))
    return worst


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("L_", [1, 8, 63, 64, 65, 130])
def test_self_attention_against_fp64(engines, L_, name):
    """mtl_self_decode_kernel<SPLIT> over a cache of L positions, three sequences (row stride 128): the KV-cached step (the last position alone) and
    the re-decode range (every position).  Sequence 1 holds <PAD> at the interior position L / 2 -- in the re-decode range that query attends with
    equal weights to all L positions, later ones included -- and sequence 2 at the last position, which the cached step computes too."""
    m = engines(name)
    pad = 17
    cache_vals, tok = R.self_case(L_, NT, MP, name, 300 + L_, pad)
    if L_ > 2:
        assert int(tok[L_ // 2, 1]) == pad and int(tok[L_ - 1, 2]) == pad
    step = _self(m, [cache_vals], tok, pad, L_ - 1, L_ - 1, NT)[0]
    w1 = _check_self(m, f"self L={L_} cached step [{name}]", step, cache_vals, tok, pad, L_ - 1, L_ - 1, NT)
    full = _self(m, [cache_vals], tok, pad, 0, L_ - 1, NT)[0]
    w2 = _check_self(m, f"self L={L_} re-decode [{name}]", full, cache_vals, tok, pad, 0, L_ - 1, NT)
    assert torch.equal(full[-1], step[0]), "the last position of the re-decode range differs from the cached step"
    print(f"mtl self attention L={L_} [{name}]: worst err/tol {max(w1, w2):.3f} (cached step {w1:.3f}, re-decode {w2:.3f})")


@pytest.mark.parametrize("name", ALL)
def test_self_attention_pair_mode(engines, name):
    """nb = 2: a second layer's cache and output behind cache_bs / att_bs, different data; both against the reference"""
    m = engines(name)
    pad, L_ = 17, 65
    cases = [R.self_case(L_, NT, MP, name, 400 + b, pad) for b in range(2)]
    tok = cases[0][1]
    got = _self(m, [c[0] for c in cases], tok, pad, 0, L_ - 1, NT, nb=2)
    worst = max(_check_self(m, f"self pair layer {b} [{name}]", got[b], cases[b][0], tok, pad, 0, L_ - 1, NT) for b in range(2))
    print(f"mtl self attention pair mode [{name}]: worst err/tol {worst:.3f}")


# ---- refused arguments ----------------------------------------------------------------------------------------------------------------------------
def test_arguments_the_kernels_cannot_take_are_refused(engines):
    """PT_ERR_INVALID with a message naming the value, and nothing is launched: the output keeps its sentinel.  Slices that do not cover hw and an
    empty last slice are the cases in which a kernel would index past its buffers; they are only ever passed as argument values here."""
    m = engines("bf16")
    x3 = engines("bf16x3")
    hw = 200
    kv = torch.zeros((NT * hw, R.KVC), dtype=m.dt, device=DEV)
    kv8 = torch.zeros((NT * hw, R.KVC), dtype=torch.uint8, device=DEV)
    q = torch.zeros((4 * MP, R.D), dtype=m.dt, device=DEV)
    tiles = [(b, b, 1, MP) for b in range(NT)]

    def refused(match, kind="stream", eng=m, kv_=kv, hw_=hw, tiles_=tiles, kps=96, ns=3, M=NT, nb=1, slot=0, q_=q, split=False, nt=NT, **kw):
        att = torch.full((4 * MP, R.D * (2 if split else 1)), SENTINEL, dtype=m.dt, device=DEV)
        op, ml = _nan(20 * MP * R.D), _nan(20 * MP * 16)
        with pytest.raises(L.PtError, match=match):
            eng.eng.op_mtl_cross_attention(KERNEL.get(kind, kind), q_, kv_, nt, hw_, slot, tiles_, kps, ns, 1, M, MP, att, op, ml, split=split, nb=nb, **kw)
        torch.cuda.synchronize()
        assert bool((att.float() == SENTINEL).all()) and bool(torch.isnan(op).all())

    refused("keys_per_split = 100", kps=100)                            # kps % 32 != 0
    refused("keys_per_split = 0", kps=0)
    refused("do not cover hw = 200", kps=64, ns=3)                   # 192 keys of 200
    refused("do not cover hw = 200", kps=192, ns=1)
    refused("is empty at hw = 200", kps=96, ns=4)                    # slice 3 would start at key 288
    refused("is empty at hw = 200", kps=224, ns=2)
    refused("hw = 0", hw_=0, kps=32, ns=1)
    refused("hw = 4097", hw_=4097, kps=4128, ns=1, nt=1, kv_=torch.zeros((4097, R.KVC), dtype=m.dt, device=DEV))
    refused("nsplit = 17", kps=32, ns=17)
    q2 = torch.zeros((4 * MP, 2 * R.D), dtype=m.dt, device=DEV)
    refused("stream8.*single-pass", kind="stream8", eng=x3, kv_=kv8, q_=q2, split=True)
    refused("table 3 of 3", tiles_=[(0, 0, 1, MP), (3, 1, 1, MP), (2, 2, 1, MP)])
    refused("exactly 1 for the stream kernels", tiles_=[(0, 0, 2, 1), (2, 2, 1, MP)])
    refused("1 .. 32 queries for mfma", kind="mfma", tiles_=[(0, 0, 33, 1)], M=64, ns=1, kps=224)
    refused("outside npos = 1 positions of M = 3", tiles_=[(0, 0, 1, MP), (1, 1, 1, MP), (2, 3, 1, MP)])
    refused("outside npos = 1", tiles_=[(0, 0, 1, MP), (1, 1, 1, MP), (2, MP + 2, 1, MP)])
    refused("is in two tiles", tiles_=[(0, 0, 1, MP), (1, 1, 1, MP), (2, 1, 1, MP)])
    refused("row 2 is in no tile", tiles_=[(0, 0, 1, MP), (1, 1, 1, MP)])
    refused("nb = 2", kind="mfma", nb=2, row_bs=MP * R.D, opart_bs=3 * MP * R.D, ml_bs=3 * MP * 16)
    refused("slot = 4 with nb = 2", nb=2, slot=4, row_bs=MP * R.D, opart_bs=3 * MP * R.D, ml_bs=3 * MP * 16)
    refused("slot = 5", slot=5)
    refused("overlap the first layer", nb=2, row_bs=MP * R.D - 8, opart_bs=3 * MP * R.D, ml_bs=3 * MP * 16)
    refused("kernel = 3", kind=3)
    # self attention and the e4m3 copy
    cache = torch.zeros((4 * MP, 3 * R.D), dtype=m.dt, device=DEV)
    tok = torch.zeros((4, MP), dtype=torch.int32, device=DEV)
    att = torch.full((4 * MP, R.D), SENTINEL, dtype=m.dt, device=DEV)
    for match, kw in (("p0 = 2 .. p1 = 1", dict(p0=2, p1=1)), ("p0 = -1", dict(p0=-1, p1=1)), ("M = 0", dict(p0=0, p1=3, M=0)),
                      ("M = 129", dict(p0=0, p1=3, M=129)), ("nb = 3", dict(p0=0, p1=3, nb=3)),
                      ("overlap the first layer", dict(p0=0, p1=1, nb=2, cache_bs=2 * MP * 3 * R.D - 8, att_bs=2 * MP * R.D))):
        args = dict(dict(M=NT, nb=1, cache_bs=0, att_bs=0), **kw)
        with pytest.raises(L.PtError, match=match):
            m.eng.op_mtl_self_attention(cache, tok, 17, args["p0"], args["p1"], MP, args["M"], att, nb=args["nb"], cache_bs=args["cache_bs"], att_bs=args["att_bs"])
    with pytest.raises(L.PtError, match="n_elems = 12"):
        m.eng.op_mtl_kv_fp8(torch.zeros(12, dtype=m.dt, device=DEV))
    torch.cuda.synchronize()
    assert bool((att.float() == SENTINEL).all())
