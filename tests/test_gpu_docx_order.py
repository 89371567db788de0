"""pt_op_docx_order (csrc/docx_order.hip) alone, through HipEngine.op_docx_order, against docx_page_result's chain on the same records
(tests/docx_order_ref.page_rows: the product's own host functions, keeping the raw float32 score): flags, counts and rows compared as raw words.
Every page here is axis-aligned (main angle exactly 0 in every sort: no condition) except the three turned pages, whose seeds were chosen on the CPU so
that the host chain alone passes the stability rule of tests/docx_order_ref.py -- the test asserts that it does before it looks at the device."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docx_order_ref as O  # noqa: E402
import docxlayout_synth as S  # noqa: E402
from pdf_table_amd import lib as L  # noqa: E402
from pdf_table_amd.docxlayout_stage import DocXLayoutConfig, DocXLayoutStage, quad_intersection_rate  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0x5A
PAGE, MAP = (768, 768), (192, 192)      # the map -> page affine is x4, offset 0: a quad given in page pixels is exact in map pixels
PAD = 256


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


# ---- building records ---------------------------------------------------------------------------------------------------------------------------
def box(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def row(quad, score, cls):
    """a record whose quad is `quad` in page pixels of PAGE"""
    r = np.zeros(12, np.float32)
    r[:8] = np.asarray(quad, np.float64) / 4.0
    r[8], r[9] = score, cls
    return r


def rows(items):
    return np.stack([row(*it) for it in items]).astype(np.float32) if len(items) else np.zeros((0, 12), np.float32)


def _score(rng):
    return float(np.float32(rng.uniform(0.35, 0.98)))


def pack(pages, K, junk=True):
    """pages: [(main rows [m,12], sub rows [s,12])] -> counts, recs, keep.  Between the rows lie junk rows with keep == 0 (a high score, a big quad) that
    only use_nms=False may read; everything behind a count is garbage that nothing may read"""
    B = len(pages)
    counts = np.zeros((B, 2), np.int32)
    recs = np.full((B, 2, K, 12), 3.0e30, np.float32)
    keep = np.full((B, 2, K), 1, np.uint8)
    for i, pg in enumerate(pages):
        for b in range(2):
            r = np.asarray(pg[b], np.float32).reshape(-1, 12)
            out, flags = [], []
            for k in range(len(r)):
                if junk and k % 3 == 1 and len(r) + len([f for f in flags if not f]) < K:
                    out.append(row(box(0, 0, 700, 700), 0.99, 0 if b else 2))
                    flags.append(0)
                out.append(r[k])
                flags.append(1)
            assert len(out) <= K, (len(out), K)
            counts[i, b] = len(out)
            if out:
                recs[i, b, :len(out)] = np.stack(out)
                keep[i, b, :len(out)] = flags
    return counts, recs, keep


def launch(eng, counts, recs, keep, cfg, page_hw=PAGE, map_hw=MAP):
    """two calls on the same canary-filled buffers -> (n_out, flag, rows) as numpy; rows behind every n_out and the bytes behind every buffer intact"""
    from pdf_table_amd.centernet_stage import centernet_decode_affine
    B, K = recs.shape[0], recs.shape[2]
    sizes = (B * 4, B * 4, B * 2 * K * 6 * 4)
    bufs = [torch.full((m + PAD,), CANARY, dtype=torch.uint8, device="cuda") for m in sizes]
    out = (bufs[0][:sizes[0]].view(torch.int32), bufs[1][:sizes[1]].view(torch.int32), bufs[2][:sizes[2]].view(torch.float32).view(B, 2 * K, 6))
    dev = [torch.from_numpy(v).cuda() for v in (counts, recs, keep)]
    inv = centernet_decode_affine(page_hw[0], page_hw[1], map_hw[0], map_hw[1])
    res = []
    for _ in range(2):
        eng.op_docx_order(*dev, inv, scores_thresh=cfg.scores_thresh, top_k=cfg.top_k, num_classes=cfg.num_classes, n_main=11, use_nms=cfg.use_nms,
                          out=out)
        torch.cuda.synchronize()
        res.append([b.cpu().numpy().copy() for b in bufs])
    for a, b in zip(*res):
        assert np.array_equal(a, b), "a second call on the same buffers changed bytes"
    for b, m in zip(res[0], sizes):
        assert (b[m:] == CANARY).all(), "bytes behind a buffer were written"
    n_out = res[0][0][:sizes[0]].view(np.int32)
    flag = res[0][1][:sizes[1]].view(np.int32)
    words = res[0][2][:sizes[2]].view(np.uint32).reshape(B, 2 * K, 6)
    for i in range(B):
        assert 0 <= n_out[i] <= 2 * K
        assert (words[i, n_out[i]:] == 0x5A5A5A5A).all(), f"page {i}: rows at or behind n_out were written"
    return n_out, flag, words


def check(eng, pages, cfg=None, K=None, junk=True, page_hw=PAGE, map_hw=MAP, stable=False):
    """the launch against the host chain, page by page -> (flags, [host rows per page])"""
    cfg = cfg or DocXLayoutConfig()
    K = K or cfg.top_k
    counts, recs, keep = pack(pages, K, junk)
    n_out, flag, words = launch(eng, counts, recs, keep, cfg, page_hw, map_hw)
    wants = []
    for i in range(len(pages)):
        main, sub = O.kept_rows(counts, recs, keep, i, cfg.use_nms)
        lengths = O.list_lengths(main, sub, page_hw, map_hw, cfg)
        if stable:
            assert O.page_is_stable(main, sub, page_hw, map_hw, cfg), f"page {i} does not pass the stability rule on the host: choose another seed"
        want = O.page_rows(main, sub, page_hw, map_hw, cfg)
        wants.append(want)
        if max(lengths) >= O.SORT_LIMIT:
            assert flag[i] == 1 and n_out[i] == 0, (i, lengths, flag[i], n_out[i])
            continue
        assert flag[i] == 0, (i, lengths, flag[i])
        assert n_out[i] == len(want), (i, n_out[i], len(want))
        got = words[i, :len(want)]
        assert np.array_equal(got, want.view(np.uint32)), (i, got.view(np.float32).tolist(), want.tolist())
    return flag, wants


def columns_page(seed, nf=2, per=6, loose=3, cls_of=None):
    """nf sub-fields side by side with `per` regions stacked in each, plus `loose` regions outside every field; rows in a seeded order"""
    rng = np.random.RandomState(seed)
    main, sub = [], []
    for f in range(nf):
        x0 = 20 + 240 * f
        sub.append((box(x0, 100, x0 + 220, 100 + 40 * per + 10), _score(rng), f % 2))
        for k in range(per):
            w = int(rng.randint(60, 200))
            main.append((box(x0 + 5, 105 + 40 * k, x0 + 5 + w, 105 + 40 * k + int(rng.randint(10, 35))), _score(rng), int(rng.randint(0, 11))))
    for k in range(loose):
        main.append((box(30 + 200 * k, 20, 30 + 200 * k + int(rng.randint(50, 150)), 60), _score(rng), int(rng.randint(0, 11))))
    order = rng.permutation(len(main))
    main = [main[i] for i in order]
    if cls_of is not None:
        main = [(q, s, cls_of) for q, s, _ in main]
    main.sort(key=lambda it: -it[1])      # a decode lists by score
    return rows(main), rows(sub)


# ---- the reference's fixtures -------------------------------------------------------------------------------------------------------------------
def _golden(golden_dir):
    with open(os.path.join(golden_dir, "docxlayout_post.json")) as f:
        return np.load(os.path.join(golden_dir, "docxlayout_post.npz")), json.load(f)


@pytest.mark.parametrize("case,size", [(c, s) for s in S.SIZES for c in S.REF_CASES])
def test_golden_cases(eng, golden_dir, case, size):
    npz, js = _golden(golden_dir)
    tag = f"{case}_{size[0]}x{size[1]}"
    main, sub = npz[f"kept_main_{tag}"][:, :12].astype(np.float32), npz[f"kept_sub_{tag}"][:, :12].astype(np.float32)
    sub[:, 9] -= 11
    flag, _ = check(eng, [(main, sub)], junk=False, page_hw=S.page_hw(size), map_hw=size)
    # all ten are served: many_48x48 keeps 68 + 67 rows, but behind the top-100 cut its longest lists are 42 sub-fields and 58 blocks
    assert flag[0] == 0, (tag, flag[0])
    # the stage-level result (flagged pages through the host route) is the reference's list
    cfg = DocXLayoutConfig()
    cfg.resolution = (size[0] * 4, size[1] * 4)
    stage = DocXLayoutStage(eng, cfg, device_order=True)
    got = stage.order_records(*pack([(main, sub)], cfg.top_k, junk=False), S.page_hw(size))[0]
    assert stage.last_fallback == []
    want = js[tag]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [float(v) for v in g["bbox"]] == w["bbox"] and g["label"] == w["label"] and g["category_id"] == w["category_id"], (tag, g, w)
        assert float(g["score"]) == w["score"] and g["bbox"].dtype == np.float64


# ---- the list and the cut -------------------------------------------------------------------------------------------------------------------------
def test_only_placeholders(eng):
    low = rows([(box(10, 10, 90, 40), 0.29, 2), (box(10, 50, 90, 80), 0.3, 3)])      # float32(0.3) is not > float32(0.3)
    flag, wants = check(eng, [(np.zeros((0, 12), np.float32), np.zeros((0, 12), np.float32)), (low, np.zeros((0, 12), np.float32))])
    assert [len(w) for w in wants] == [0, 0] and (flag == 0).all()


def _all_classes(n_extra, rng, scores=None):
    """one row in each of the 11 main and 2 sub classes (no placeholder), then n_extra more main rows"""
    main = [(box(10 + 60 * c, 10, 50 + 60 * c, 40), _score(rng), c) for c in range(11)]
    main += [(box(10 + 30 * k, 100, 35 + 30 * k, 130), _score(rng), int(rng.randint(0, 11))) for k in range(n_extra)]
    sub = [(box(0, 0, 350, 200), _score(rng), 0), (box(350, 0, 700, 200), _score(rng), 1)]
    if scores is not None:
        main = [(q, s, c) for (q, _, c), s in zip(main, scores)]
    return main, sub


def test_exactly_top_k_rows_placeholders_counted(eng):
    rng = np.random.RandomState(3)
    # 16 rows in 9 of the 13 classes + 4 placeholders = top_k = 20: nothing is cut
    main = [(box(10 + 40 * k, 10 + 35 * (k % 5), 45 + 40 * k, 40 + 35 * (k % 5)), _score(rng), k % 8) for k in range(15)]
    sub = [(box(0, 0, 300, 300), _score(rng), 1)]
    _, wants = check(eng, [(rows(main), rows(sub))], DocXLayoutConfig(top_k=20))
    assert len(wants[0]) == 15
    # one row more: the cut is the second smallest of (4 zeros, 17 scores) = 0 -- still nothing real is cut
    main.append((box(500, 500, 560, 530), 0.31, 2))
    _, wants = check(eng, [(rows(main), rows(sub))], DocXLayoutConfig(top_k=20))
    assert len(wants[0]) == 16


def test_ties_at_the_cut_stay(eng):
    rng = np.random.RandomState(4)
    # 21 rows, no placeholder, top_k 20: the cut is the second smallest score; the two smallest are equal -> all 21 stay
    main, sub = _all_classes(8, rng)
    sc = [0.5 + 0.01 * k for k in range(len(main))]
    sc[3] = sc[12] = 0.4
    main = [(q, s, c) for (q, _, c), s in zip(main, sc)]
    sub = [(q, 0.9, c) for q, _, c in sub]
    _, wants = check(eng, [(rows(main), rows(sub))], DocXLayoutConfig(top_k=20))
    assert len(wants[0]) == 19
    # 22 rows: one smaller score goes, the pair at the cut stays
    main.append((box(600, 300, 660, 330), 0.35, 5))
    _, wants = check(eng, [(rows(main), rows(sub))], DocXLayoutConfig(top_k=20))
    assert len(wants[0]) == 19 and not (wants[0][:, 4] == np.float32(0.35)).any() and (wants[0][:, 4] == np.float32(0.4)).sum() == 2
    # the cut falls on a sub-field's score: the fields below it go, the regions are loose
    sub = [(q, 0.32, c) for q, _, c in sub]
    _, wants = check(eng, [(rows(main), rows(sub))], DocXLayoutConfig(top_k=19), K=32)
    assert len(wants[0]) == 19


@pytest.mark.parametrize("top_k", (1, 128))
def test_top_k_extremes(eng, top_k):
    rng = np.random.RandomState(top_k)
    if top_k == 1:      # 13 "rows" (11 placeholders): only the best score stays
        main, sub = rows([(box(10, 10, 200, 60), 0.9, 7)]), rows([(box(0, 0, 400, 400), 0.8, 0)])
        _, wants = check(eng, [(main, sub), (rows([(box(10, 10, 200, 60), 0.7, 7)]), sub)], DocXLayoutConfig(top_k=1), junk=False)
        assert [len(w) for w in wants] == [1, 0]
    else:               # 120 regions in 3 fields of 40
        main, sub = columns_page(7, nf=3, per=40, loose=0)
        _, wants = check(eng, [(main, sub)], DocXLayoutConfig(top_k=128), junk=False)
        assert len(wants[0]) == 120


@pytest.mark.parametrize("nf", (0, 1, 3))
def test_sub_field_counts(eng, nf):
    pages = [columns_page(10 * nf + s, nf=nf, per=5, loose=4) for s in range(2)]
    _, wants = check(eng, pages)
    assert all(len(w) == 5 * nf + 4 for w in wants)


# ---- the overlap rate -------------------------------------------------------------------------------------------------------------------------------
def test_equal_rates_first_sorted_field_wins(eng):
    left, right = box(0, 100, 200, 500), box(200, 100, 400, 500)
    astride = box(150, 200, 250, 240)      # half in each
    assert quad_intersection_rate(astride, left) == quad_intersection_rate(astride, right) == 0.5
    main = [(astride, 0.9, 2), (box(10, 120, 150, 160), 0.8, 2), (box(210, 120, 390, 160), 0.7, 2), (box(210, 300, 390, 340), 0.6, 2)]
    for subs in ([(left, 0.9, 0), (right, 0.8, 0)], [(right, 0.9, 0), (left, 0.8, 0)]):      # whatever the list order, the left field sorts first
        _, wants = check(eng, [(rows(main), rows(subs))])
        got = [tuple(int(v) for v in r[:4]) for r in wants[0]]
        assert got.index((150, 200, 250, 240)) < got.index((210, 120, 390, 160)), got      # inside the left field's block


RATE_UP = ([1, 0, 6, 0, 6, 25, 1, 25], [-46, -14, 53, 19, 53, -14, -46, -37])       # one double step above 0.1 (found by search on the CPU)
RATE_EQ = ([1, 1, 7, 1, 7, 21, 1, 21], [-23, -6, 31, 12, 31, -26, -23, -32])        # exactly the double 0.1
RATE_DN = ([3, 1, 8, 1, 8, 31, 3, 31], [-26, -17, 37, 25, 37, -40, -26, -38])       # one step below


@pytest.mark.parametrize("name,pair,assigned", [("up", RATE_UP, True), ("eq", RATE_EQ, False), ("dn", RATE_DN, False)])
def test_rate_at_a_tenth(eng, name, pair, assigned):
    region, field = pair
    rate = quad_intersection_rate([float(v) for v in region], [float(v) for v in field])
    assert rate == {"up": np.nextafter(0.1, 1), "eq": 0.1, "dn": np.nextafter(0.1, 0)}[name]
    # a second region far below the field and left of everything: loose.  Whether `region` is in the field decides the order of the two
    other = box(-40, 300, -10, 330)
    main, sub = rows([(region, 0.9, 2), (other, 0.8, 2)]), rows([(field, 0.9, 0)])
    lengths = O.list_lengths(main, sub, PAGE, MAP, DocXLayoutConfig())
    assert lengths[1] == (1 if assigned else 2), lengths
    check(eng, [(main, sub)], junk=False)


def test_odd_quads(eng):
    field = box(0, 0, 400, 400)
    bow = [10, 10, 90, 50, 90, 10, 10, 50]            # not convex: both bounding boxes
    flat = [100, 100, 180, 100, 180, 100, 100, 100]   # zero area: rate 0, loose
    cw = [10, 200, 10, 240, 120, 240, 120, 200]       # clockwise
    dia = [300, 380, 340, 420, 300, 460, 260, 420]    # a diamond half outside the field
    main = [(bow, 0.9, 1), (flat, 0.8, 2), (cw, 0.7, 3), (dia, 0.6, 4), (box(200, 20, 380, 60), 0.5, 2)]
    for f in (field, [0, 0, 0, 400, 400, 400, 400, 0], [0, 0, 400, 400, 400, 0, 0, 400], [5, 5, 5, 5, 5, 5, 5, 5]):      # a clockwise, a bow-tie, a point field
        _, wants = check(eng, [(rows(main), rows([(f, 0.9, 0)]))])
        assert len(wants[0]) == 5


# ---- the sort -------------------------------------------------------------------------------------------------------------------------------------------
def test_comparison_cycle_as_regions(eng):
    """t < u < l < t (tests/test_docxlayout_host.py), shifted into the page: the three rotations of the list give different results"""
    t, u, l = box(20, 0, 30, 30), box(32, 0, 42, 10), box(8, 18, 18, 28)
    pages = []
    for order in ((t, u, l), (l, t, u), (u, l, t)):
        pages.append((rows([(q, 0.9 - 0.1 * k, 2) for k, q in enumerate(order)]), np.zeros((0, 12), np.float32)))
    _, wants = check(eng, pages, junk=False)
    assert len({tuple(w[0, :4]) for w in wants}) > 1


@pytest.mark.parametrize("n", (2, 3, 10, 40))
def test_strictly_descending_initial_order(eng, n):
    main = [(box(10, 20 * (n - k), 200, 20 * (n - k) + 12), 0.9 - 0.01 * k, 2) for k in range(n)]      # listed bottom to top
    _, wants = check(eng, [(rows(main), np.zeros((0, 12), np.float32))], junk=False)
    assert [int(r[1]) for r in wants[0]] == [20 * k for k in range(1, n + 1)]


def _scatter(n, rng, x0=0, y0=0, w=600, h=600, cls=2):
    out = []
    for k in range(n):
        x, y = x0 + int(rng.randint(0, w - 60)), y0 + int(rng.randint(0, h - 30))
        out.append((box(x, y, x + int(rng.randint(10, 60)), y + int(rng.randint(5, 30))), _score(rng), cls))
    return out


@pytest.mark.parametrize("n", (1, 2, 63, 64))
def test_list_lengths_loose(eng, n):
    rng = np.random.RandomState(n)
    flag, _ = check(eng, [(rows(_scatter(n, rng)), np.zeros((0, 12), np.float32))], K=100, junk=False)
    assert flag[0] == (1 if n == 64 else 0)


@pytest.mark.parametrize("n", (63, 64))
def test_list_lengths_inside_a_field_and_of_fields_and_blocks(eng, n):
    rng = np.random.RandomState(100 + n)
    none = np.zeros((0, 12), np.float32)
    inside = (rows(_scatter(n, rng) + [(box(700, 700, 760, 720), 0.5, 3)]), rows([(box(-10, -10, 650, 650), 0.9, 0)]))
    fields = (rows([(box(5, 5, 60, 20), 0.5, 3)]), rows([(box(10 * (k % 8) * 9, 40 * (k // 8), 10 * (k % 8) * 9 + 80, 40 * (k // 8) + 30), _score(rng), k % 2)
                                                           for k in range(n)]))
    blocks = (rows(_scatter(n - 30, rng, y0=700, h=300)), rows([(box(90 * (k % 8), 40 * (k // 8), 90 * (k % 8) + 80, 40 * (k // 8) + 30), _score(rng), k % 2)
                                                                 for k in range(30)]))
    flag, _ = check(eng, [inside, fields, blocks, (none, none)], K=100, junk=False)
    assert flag.tolist() == ([1, 1, 1, 0] if n == 64 else [0, 0, 0, 0])


# seeds chosen on the CPU: the host chain alone gives one list in all nine perturbed runs (docx_order_ref.page_is_stable)
TURNED = [(3.0, 0), (-7.0, 1), (15.0, 2)]


def turned_page(deg, seed):
    """a two-column page turned by `deg` degrees about its centre, vertices rounded to integers"""
    rng = np.random.RandomState(seed)
    th = math.radians(deg)
    c, s = math.cos(th), math.sin(th)

    def turn(q):
        out = []
        for k in range(0, 8, 2):
            x, y = q[k] - 384, q[k + 1] - 384
            out += [round(384 + x * c - y * s), round(384 + x * s + y * c)]
        return out

    main, sub = [], []
    for f in range(2):
        x0 = 120 + 280 * f
        sub.append((turn(box(x0, 150, x0 + 250, 650)), _score(rng), f))
        y = 160
        for k in range(7):
            h = int(rng.randint(25, 55))
            main.append((turn(box(x0 + 8, y, x0 + 8 + int(rng.randint(150, 235)), y + h)), _score(rng), int(rng.randint(0, 11))))
            y += h + int(rng.randint(9, 20))
    main.append((turn(box(130, 90, 640, 120)), _score(rng), 3))      # a header and a footer outside the columns
    main.append((turn(box(330, 690, 440, 715)), _score(rng), 4))
    main.sort(key=lambda it: -it[1])
    return rows(main), rows(sub)


@pytest.mark.parametrize("deg,seed", TURNED)
def test_turned_pages(eng, deg, seed):
    _, wants = check(eng, [turned_page(deg, seed)], stable=True)
    assert len(wants[0]) == 16


def test_use_nms_false_reads_every_row(eng):
    pages = [columns_page(21, nf=2, per=4, loose=2), columns_page(22, nf=1, per=6, loose=1)]
    cfg = DocXLayoutConfig(use_nms=False)
    _, with_junk = check(eng, pages, cfg)               # the keep == 0 rows between the others count now
    _, without = check(eng, pages, DocXLayoutConfig())
    assert all(len(a) > len(b) for a, b in zip(with_junk, without))


def test_batch_with_empty_first_and_last_page(eng):
    none = (np.zeros((0, 12), np.float32), np.zeros((0, 12), np.float32))
    _, wants = check(eng, [none, columns_page(31, nf=2, per=5, loose=3), none])
    assert [len(w) for w in wants] == [0, 13, 0]


def test_non_positive_threshold_and_non_finite_vertex_are_flagged(eng):
    main, sub = columns_page(41, nf=1, per=3, loose=1)
    counts, recs, keep = pack([(main, sub)], 100)
    _, flag, _ = launch(eng, counts, recs, keep, DocXLayoutConfig(scores_thresh=0.0))
    assert flag[0] == 1
    bad = main.copy()
    bad[1, 3] = np.inf
    counts, recs, keep = pack([(bad, sub), (main, sub)], 100)
    n_out, flag, _ = launch(eng, counts, recs, keep, DocXLayoutConfig())
    assert flag.tolist() == [1, 0] and n_out[0] == 0 and n_out[1] == 4


def test_refusals_write_nothing(eng):
    def attempt(B=1, K=8, num_classes=13, n_main=11):
        bufs = [torch.full((64 + max(B, 1) * 2 * K * 24,), CANARY, dtype=torch.uint8, device="cuda") for _ in range(3)]
        out = (bufs[0][:max(B, 1) * 4].view(torch.int32), bufs[1][:max(B, 1) * 4].view(torch.int32),
               bufs[2][:max(B, 1) * 2 * K * 24].view(torch.float32).view(max(B, 1), 2 * K, 6))
        dev = (torch.zeros((B, 2), dtype=torch.int32, device="cuda"), torch.zeros((B, 2, K, 12), dtype=torch.float32, device="cuda"),
               torch.ones((B, 2, K), dtype=torch.uint8, device="cuda"))
        with pytest.raises(L.PtError, match="pt_op_docx_order"):
            eng.op_docx_order(*dev, np.eye(2, 3), num_classes=num_classes, n_main=n_main, out=out)
        torch.cuda.synchronize()
        assert all((b.cpu().numpy() == CANARY).all() for b in bufs)

    attempt(K=L.PT_DOCX_MAX_K + 1)
    attempt(num_classes=17)
    attempt(num_classes=13, n_main=13)
    attempt(B=0)
