"""The yardstick of the layout decode on the device, without a GPU (tests/layout_decode_ref.py): decode64 -- decode_page with every step in
float64 -- picks what LayoutStage.decode_page picks on every seeded builder case, and every case keeps all its decisions (score threshold,
candidate order, the level cut, every IoU test) clear of 4 x the host-vs-float64 difference measured on it, so that no GPU case is ever left out."""
import warnings

import numpy as np
import pytest

import layout_decode_ref as R

CASES = R.all_cases()


@pytest.fixture(scope="module", autouse=True)
def _built():
    from pdf_table_amd.build import build
    build(verbose=False)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_decode64_picks_what_decode_page_picks(case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # the NaN case compares NaN on the host
        host = R.host_decode(case)
        d_box, d_score, same = R.host_vs_64(case)
    ref = R.decode64(case["rec"], case["cfg"], case["org"], case["probs"])
    assert same and [d["category_id"] for d in host] == [d["category_id"] for d in ref]
    assert d_box < 1e-3 and d_score < 1e-6      # float32 rounding of coordinates below 2048 and of scores below 1, nothing coarser
    assert len({(d["category_id"],) + d["src"] for d in ref}) == len(ref)
    print(f"{case['name']}: {len(case['rec'])} records, {len(ref)} detections, host vs float64: box {d_box:.3g}, score {d_score:.3g}")
    assert R.margins_ok(case, 4 * d_box, 4 * d_score)


def test_builders_cover_what_the_gpu_tests_need():
    by = {c["name"]: c for c in CASES}
    assert sorted({len(c["rec"]) for c in CASES} & {0, 1, 37, 260}) == [0, 1, 37, 260]
    assert {len(c["cfg"].labels) for c in CASES} == {1, 5, 10} and {len(c["cfg"].strides) for c in CASES} == {1, 3, 4}
    n260 = R._walk64(by["n260"]["rec"], by["n260"]["cfg"], False)[1]["class_scores"]
    assert max(len(s) for s in n260) > R.CANDIDATE_SIZE
    cut = by["cut40"]
    lv = cut["rec"][:, 0].view(np.int32)
    assert (lv == 0).sum() == 40 > cut["cfg"].nms_top_k == 16 and cut["cfg"].keep_top_k == 3
    assert R._walk64(cut["rec"], cut["cfg"], False)[1]["cut"]
    assert [d["src"][1] % 76 for d in R.decode64(by["chain"]["rec"], by["chain"]["cfg"], (800, 608), True)] == [10, 16]      # A and C; B is gone
    tc = by["tenth_column"]
    assert (tc["rec"][:, 1].view(np.int32) % 10 == 9).any() and tc["cfg"].img_width == 608
    zw = R.decode64(by["zero_width"]["rec"], by["zero_width"]["cfg"], (800, 608), True)
    assert len(zw) == 6 and all(d["bbox"][0] == d["bbox"][2] for d in zw)
    cl = np.array([d["bbox"] for d in R.decode64(by["clip"]["rec"], by["clip"]["cfg"], by["clip"]["org"], True)])
    assert (cl[:, 0] == 0).any() and (cl[:, 1] == 0).any() and np.isclose(cl[:, 2], 410 * 410 / 608).any() and np.isclose(cl[:, 3], 500 * 500 / 800).any()      # clipped at the page size, then rescaled
    te = R.decode64(by["threshold_edge"]["rec"], by["threshold_edge"]["cfg"], (800, 608), True)
    assert len(te) == 3 and len(by["threshold_edge"]["rec"]) == 4      # the record one step below the threshold is gone


def test_margin_checker_refuses_what_could_flip():
    chain = R.chain_case()
    assert R.margins_ok(chain, 1e-4, 1e-7)
    assert not R.margins_ok(chain, 1e-4, 0.06)          # 0.9 / 0.8 / 0.7: neighbours within 2 x 0.06
    assert not R.margins_ok(chain, 6.0, 1e-7)           # boxes shrunk by 6 px: the 0.54 IoU falls to 0.48, the interval contains 0.5
    assert not R.margins_ok(R.tie_case(), 0.0, 0.0)     # exactly equal scores
    edge = R.threshold_edge_case()
    assert R.margins_ok(edge, 0.0, 0.0) and not R.margins_ok(edge, 0.0, 1e-7)


def test_decode64_does_not_depend_on_arrival():
    case = R.batches()["ten_classes_four_levels_probs"][0]
    a = R.decode64(case["rec"], case["cfg"], case["org"], True)
    b = R.decode64(case["rec"][::-1], case["cfg"], case["org"], True)
    assert [(d["category_id"], d["src"]) for d in a] == [(d["category_id"], d["src"]) for d in b]
