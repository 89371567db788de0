"""pt_op_layout_decode (csrc/layout_decode.hip) alone, through HipEngine.op_layout_decode, against LayoutStage.decode_page on the same records.

Every call decodes B = 3 pages of different counts (tests/layout_decode_ref.py: batches()).  The class and pick sequence must equal
decode_page's exactly; boxes and scores must lie within 4 x the largest |decode_page - decode64| of that case, computed here -- no number is
fixed in advance; the measured values go to profiles/r20/layout_decode_tests.txt when PT_WRITE_PROFILES is set.  The margin checker says beforehand
that no decision of a case can flip within that bound (test_layout_decode_host.py keeps the seeds such that none does)."""
import os
import warnings

import numpy as np
import pytest
import torch

import layout_decode_ref as R
from pdf_table_amd import lib as L

pytestmark = pytest.mark.gpu

MAXC = 272            # records per page in these buffers: above every case's count
GUARD = 64            # canary elements behind a buffer
BATCHES = R.batches()
LOG = []


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    return HipEngine(0)


@pytest.fixture(scope="module", autouse=True)
def _write_log():
    yield
    path = os.environ.get("PT_WRITE_PROFILES")
    if path and LOG:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "layout_decode_tests.txt"), "w") as f:
            f.write("case  records  detections  host-vs-float64 (box, score)  device-vs-host (box, score)  bound = 4 x host-vs-float64\n")
            f.write("\n".join(LOG) + "\n")


def upload(eng, cases, max_cands=MAXC, counts=None, fill=0.0):
    """pages of one call -> (counts, cands) on the device; the slab behind a page's records holds `fill`"""
    B = len(cases)
    cands = np.full((B, max_cands, R.REC), fill, np.float32)
    for i, c in enumerate(cases):
        k = min(len(c["rec"]), max_cands)
        cands[i, :k] = c["rec"][:k]
    cnt = np.array([len(c["rec"]) for c in cases] if counts is None else counts, np.int32)
    return torch.from_numpy(cnt).to(eng._tdev), torch.from_numpy(cands).to(eng._tdev)


def run(eng, cases, counts_d, cands_d, max_dets=None, out=None):
    cfg, org, probs = cases[0]["cfg"], cases[0]["org"], cases[0]["probs"]
    assert all(c["org"] == org and c["probs"] == probs and c["cfg"].strides == cfg.strides and c["cfg"].labels == cfg.labels for c in cases)
    ndet, dets = eng.op_layout_decode(counts_d, cands_d, len(cfg.labels), cfg.strides, cfg.img_height, cfg.img_width, org[0], org[1], probs=probs,
                                      score_threshold=cfg.score_threshold, nms_threshold=cfg.nms_threshold, nms_top_k=cfg.nms_top_k,
                                      candidate_size=R.CANDIDATE_SIZE, keep_top_k=cfg.keep_top_k, max_dets=max_dets, out=out)
    return ndet.cpu().numpy(), dets.cpu().numpy()


def host(case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return R.host_decode(case), R.host_vs_64(case)


def compare(case, got_n, got, tag=""):
    """one page: device rows against decode_page within 4 x the case's own host-vs-float64 difference"""
    ref, (d_box, d_score, same) = host(case)
    assert same and R.margins_ok(case, 4 * d_box, 4 * d_score), f"{case['name']}: the case does not keep its decisions clear of the bound"
    n = len(ref)
    e_box = max((float(np.abs(got[k, :4] - ref[k]["bbox"]).max()) for k in range(min(n, got_n))), default=0.0)
    e_score = max((abs(float(got[k, 4]) - float(ref[k]["score"])) for k in range(min(n, got_n))), default=0.0)
    line = (f"{tag}{case['name']:<14} {len(case['rec']):>4} {n:>4}   {d_box:.3g} {d_score:.3g}   {e_box:.3g} {e_score:.3g}   "
            f"{4 * d_box:.3g} {4 * d_score:.3g}")
    print(line)
    LOG.append(line)
    assert got_n == n, f"{case['name']}: {got_n} detections, decode_page has {n}"
    assert [int(got[k, 5]) for k in range(n)] == [d["category_id"] for d in ref]
    assert e_box <= 4 * d_box and e_score <= 4 * d_score, line
    return ref


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_matches_decode_page(eng, name):
    cases = BATCHES[name]
    assert len(cases) == 3 and len({len(c["rec"]) for c in cases}) == 3
    counts_d, cands_d = upload(eng, cases, fill=np.nan)          # whatever lies behind a page's records is never read
    got_n, got = run(eng, cases, counts_d, cands_d)
    for i, c in enumerate(cases):
        ref = compare(c, int(got_n[i]), got[i], tag=f"{name}/")
        if c["name"] == "chain":
            assert len(ref) == 2
        if c["name"] == "nan":
            assert not np.isnan(got[i, :got_n[i]]).any()


@pytest.mark.parametrize("name", ["ten_classes_four_levels_probs", "both_cuts", "five_classes_three_levels"])
def test_arrival_order_does_not_matter(eng, name):
    cases = BATCHES[name]
    outs = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        shuffled = [dict(c, rec=c["rec"][rng.permutation(len(c["rec"]))]) for c in cases]
        got_n, got = run(eng, shuffled, *upload(eng, shuffled))
        outs.append((got_n, np.concatenate([got[i, :got_n[i]].ravel() for i in range(3)])))
    for got_n, flat in outs[1:]:
        assert np.array_equal(got_n, outs[0][0]) and flat.tobytes() == outs[0][1].tobytes()


def test_equal_scores_follow_the_key(eng):
    """two exactly equal scores on overlapping boxes: no host order to match.  Bit-identical over three arrivals, and a valid greedy outcome under
    (score descending, level, anchor ascending): the lower anchor is taken, the other suppressed"""
    tie = R.tie_case()
    assert not R.margins_ok(tie, 0.0, 0.0)
    outs = []
    for perm in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
        cases = [dict(tie, rec=tie["rec"][perm]), R.chain_case(), R.zero_width_case()]
        got_n, got = run(eng, cases, *upload(eng, cases))
        outs.append(got[0, :got_n[0]].copy())
    assert all(o.tobytes() == outs[0].tobytes() for o in outs[1:])
    ref = R.decode64(tie["rec"], tie["cfg"], tie["org"], True)
    assert [d["src"][1] % 76 for d in ref] == [20, 40] and len(outs[0]) == 2
    assert np.abs(outs[0][:, :4] - np.array([d["bbox"] for d in ref])).max() < 1e-3
    assert outs[0][:, 4].tolist() == [float(np.float32(0.8)), float(np.float32(0.7))] and outs[0][:, 5].tolist() == [2.0, 2.0]


def test_count_above_max_cands_and_canaries(eng):
    """counts[b] = max_cands + 5 reads max_cands records: what lies behind them would win every class.  Nothing is written behind dets"""
    cfg = R.make_cfg(ncls=5, strides=(8, 16, 32))
    max_cands = 24
    cases = [R.random_case(f"full{k}", 200 + k, max_cands, cfg, (800, 608), True, hot=1.0) for k in range(3)]
    cases[1] = dict(cases[1], rec=cases[1]["rec"][:7])
    cases[0] = dict(cases[0], rec=cases[0]["rec"][:15])
    flat = torch.zeros((3 * max_cands + GUARD) * R.REC, dtype=torch.float32)
    bait = R.record(5, 0, 5, np.full(5, 0.999, np.float32), sides=(6, 6, 6, 6))
    flat.view(-1, R.REC)[3 * max_cands:] = torch.from_numpy(bait)
    view = flat[:3 * max_cands * R.REC].view(3, max_cands, R.REC)
    for i, c in enumerate(cases):
        view[i, :len(c["rec"])] = torch.from_numpy(c["rec"])
    flat_d = flat.to(eng._tdev)
    cands_d = flat_d[:3 * max_cands * R.REC].view(3, max_cands, R.REC)
    counts_d = torch.tensor([15, 7, max_cands + 5], dtype=torch.int32, device=eng._tdev)
    max_dets = 5 * 100
    dets_flat = torch.full((3 * max_dets * 6 + GUARD,), -7.0, dtype=torch.float64, device=eng._tdev)
    ndet_d = torch.full((3 + GUARD,), -7, dtype=torch.int32, device=eng._tdev)
    out = (ndet_d[:3], dets_flat[:3 * max_dets * 6].view(3, max_dets, 6))
    got_n, got = run(eng, cases, counts_d, cands_d, max_dets=max_dets, out=out)
    for i, c in enumerate(cases):
        compare(c, int(got_n[i]), got[i], tag="canary/")
        assert (got[i, got_n[i]:] == -7.0).all()          # rows behind a page's detections are left as they were
    assert (dets_flat[3 * max_dets * 6:] == -7.0).all() and (ndet_d[3:] == -7).all()
    assert torch.equal(flat_d.cpu(), flat)


def test_more_detections_than_max_dets_are_counted_not_written(eng):
    cases = BATCHES["five_classes_three_levels"]
    counts_d, cands_d = upload(eng, cases)
    full_n, full = run(eng, cases, counts_d, cands_d)
    assert full_n.max() > 4
    dets_flat = torch.full((3 * 4 * 6 + GUARD,), -7.0, dtype=torch.float64, device=eng._tdev)
    ndet_d = torch.zeros(3, dtype=torch.int32, device=eng._tdev)
    got_n, got = run(eng, cases, counts_d, cands_d, max_dets=4, out=(ndet_d, dets_flat[:72].view(3, 4, 6)))
    assert np.array_equal(got_n, full_n)
    for i in range(3):
        k = min(4, int(full_n[i]))
        assert got[i, :k].tobytes() == full[i, :k].tobytes() and (got[i, k:] == -7.0).all()
    assert (dets_flat[72:] == -7.0).all()


def test_second_call_on_the_same_buffers(eng):
    cases = BATCHES["ten_classes_four_levels_probs"]
    counts_d, cands_d = upload(eng, cases)
    ndet_d = torch.zeros(3, dtype=torch.int32, device=eng._tdev)
    dets_d = torch.zeros((3, 1000, 6), dtype=torch.float64, device=eng._tdev)
    n1, d1 = run(eng, cases, counts_d, cands_d, max_dets=1000, out=(ndet_d, dets_d))
    n2, d2 = run(eng, cases, counts_d, cands_d, max_dets=1000, out=(ndet_d, dets_d))
    assert np.array_equal(n1, n2) and d1.tobytes() == d2.tobytes() and n1.sum() > 0


def test_refused_without_a_launch(eng):
    cases = BATCHES["crafted"]
    counts_d, cands_d = upload(eng, cases)
    ndet_d = torch.full((3,), -7, dtype=torch.int32, device=eng._tdev)
    dets_d = torch.full((3, 8, 6), -7.0, dtype=torch.float64, device=eng._tdev)
    kw = dict(inp_h=800, inp_w=608, org_h=800, org_w=608, probs=True, score_threshold=0.5, nms_threshold=0.5, max_dets=8, out=(ndet_d, dets_d))
    with pytest.raises(L.PtError, match="15 classes"):
        eng.op_layout_decode(counts_d, cands_d, 15, (8, 16, 32), **kw)
    with pytest.raises(L.PtError, match="5 levels"):
        eng.op_layout_decode(counts_d, cands_d, 5, (8, 16, 32, 64, 128), **kw)
    with pytest.raises(L.PtError, match="candidate_size 257"):
        eng.op_layout_decode(counts_d, cands_d, 5, (8, 16, 32), candidate_size=257, **kw)
    big = torch.zeros((1, 4097, R.REC), dtype=torch.float32, device=eng._tdev)
    with pytest.raises(L.PtError, match="max_cands 4097"):
        eng.op_layout_decode(counts_d[:1], big, 5, (8, 16, 32), **dict(kw, out=(ndet_d[:1], dets_d[:1])))
    with pytest.raises(ValueError):
        eng.op_layout_decode(counts_d[:2], cands_d, 5, (8, 16, 32), **kw)
    torch.cuda.synchronize()
    assert (ndet_d == -7).all() and (dets_d == -7.0).all()
