"""pt_op_teds_cost and pt_op_teds_dist (csrc/teds.hip) alone, through HipEngine.op_teds_cost / op_teds_dist.

Cost: against tests/teds_ref.py's two-row Levenshtein, the integers divided in float64 -- BIT-EQUAL, it is one division of two exact integers.  Lengths 0,
1, 63, 64, 65 and the limit 1024 on either side (the thread path takes a pair whose shorter side, after the common prefix and suffix are stripped, is at
most 64 tokens; the wave path both-longer pairs), equal contents, contents that differ in the last token only, token ids 0 and 2^31 - 1, 1024 against
1024 without a common token; several table pairs per call with different content counts, one with none, overlapping row / column ranges.

Dist: against the brute-force forest recursion (exact rationals) for trees up to 20 nodes and the host Zhang-Shasha (itself checked against the brute
force in tests/test_teds_host.py) above, within |d_dev - d_ref| <= (N1 + N2)^2 2^-52 -- derived, not measured: an edit script has at most N1 + N2 terms of
at most 1, each sum rounded once.  Node counts 1, 2, 63, 64, 65, 130 (a pair goes to one lane below 64 nodes on a side, to the workgroup's anti-diagonals
from 64 on both), 7 against 130, sections on one side only, two wide sections on both sides, a chain of nested elements.

Both: refusals leave a canary-filled output untouched, a canary behind the outputs survives, and a second call on the same buffers gives the same bits."""
import random

import numpy as np
import pytest
import torch

import teds_ref as R
from pdf_table_amd import table_metric as M
from pdf_table_amd.lib import PtError

pytestmark = pytest.mark.gpu

CANARY = -12345.5


@pytest.fixture(scope="module")
def eng():
    from pdf_table_amd.engine import HipEngine
    return HipEngine(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- cost -----------------------------------------------------------------------------------------------------------------------------------------
def cost_contents():
    rng = np.random.default_rng(7)
    small = lambda n: rng.integers(0, 3, n).astype(np.int32)
    c63, c64, c65 = small(63), small(64), small(65)
    last = c65.copy()
    last[-1] = 2 ** 31 - 1
    first = c65.copy()
    first[0] = 2 ** 31 - 1
    l1 = small(1024)
    l2 = l1.copy()
    l2[rng.integers(0, 1024, 40)] = 7                                   # the limit against the limit, about 40 substitutions
    l3 = np.delete(l1, rng.integers(0, 1024, 30))                       # and about 30 deletions (994 tokens)
    short = [np.zeros(0, np.int32), np.zeros(0, np.int32), np.asarray([0], np.int32), np.asarray([2 ** 31 - 1], np.int32), c63, c64, c65, c65.copy(),
             last, first, small(65), small(130), small(72)]
    long_ = [l1, l2, l3, np.arange(1000, 2024, dtype=np.int32), np.arange(5000, 6024, dtype=np.int32)]
    return short, long_


@pytest.fixture(scope="module")
def cost_case():
    """contents, table pairs and the reference matrix of every pair, computed once"""
    short, long_ = cost_contents()
    contents = short + long_
    ns, nl = len(short), len(long_)
    # (first row content, rows, first column content, columns): short x all; nothing; long x long (l1, l2 against l2, l3) and 1024 distinct tokens against
    # themselves and 1024 others (the 1024-token reference runs are the slow part of this file, 5 of them); an overlapping range; one row
    ranges = [(0, ns, 0, ns + 1), (3, 0, 5, 0), (ns, 2, ns + 1, 2), (ns + 3, 1, ns + 3, 2), (2, 6, 4, 5), (ns - 1, 1, 0, ns)]
    pairs, off = [], 0
    for r0, nr, c0, nc in ranges:
        pairs.append((r0, nr, c0, nc, off))
        off += nr * nc
    want = []
    for r0, nr, c0, nc, _ in pairs:
        w = np.zeros((nr, nc))
        for r in range(nr):
            for c in range(nc):
                a, b = contents[r0 + r].tolist(), contents[c0 + c].tolist()
                w[r, c] = R.levenshtein(a, b) / max(len(a), len(b)) if (a or b) else 0.0
        want.append(w)
    coff = np.concatenate([[0], np.cumsum([len(c) for c in contents])]).astype(np.int32)
    return dict(tok=np.concatenate(contents).astype(np.int32), coff=coff, pairs=np.asarray(pairs, np.int64), want=want, c_elems=off)


def test_cost_bit_equal_canary_and_second_call(eng, cost_case):
    k = cost_case
    out = torch.full((k["c_elems"] + 16,), CANARY, dtype=torch.float64, device="cuda")
    args = (dev(k["tok"]), dev(k["coff"]), dev(k["pairs"]), k["coff"], k["pairs"])
    eng.op_teds_cost(*args, out=out, c_elems=k["c_elems"])
    got = out.cpu().numpy()
    assert np.all(got[k["c_elems"]:] == CANARY)
    for (r0, nr, c0, nc, off), w in zip(k["pairs"].tolist(), k["want"]):
        g = got[off:off + nr * nc].reshape(nr, nc)
        assert np.array_equal(g, w), (r0, nr, c0, nc, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])
    assert k["want"][0][6, 7] == 0.0 and k["want"][0][6, 8] == 1 / 65 and k["want"][0][0, 1] == 0.0 and k["want"][0][0, 2] == 1.0      # the cases by name
    assert k["want"][3][0, 1] == 1.0 and k["want"][3][0, 0] == 0.0                                                                    # 1024 distinct against 1024
    eng.op_teds_cost(*args, out=out, c_elems=k["c_elems"])
    assert np.array_equal(out.cpu().numpy(), got)


def test_cost_refuses_long_content_without_a_launch(eng):
    tok = np.zeros(1025 + 3, np.int32)
    coff = np.asarray([0, 3, 1028], np.int32)
    pairs = np.asarray([[0, 2, 0, 2, 0]], np.int64)
    out = torch.full((8,), CANARY, dtype=torch.float64, device="cuda")
    with pytest.raises(PtError, match="1025 tokens"):
        eng.op_teds_cost(dev(tok), dev(coff), dev(pairs), coff, pairs, out=out)
    with pytest.raises(PtError, match="C holds 3"):                      # a matrix that does not fit
        eng.op_teds_cost(dev(tok[:6]), dev(np.asarray([0, 3, 6], np.int32)), dev(pairs), np.asarray([0, 3, 6], np.int32), pairs, out=out, c_elems=3)
    with pytest.raises(PtError, match="names contents"):
        bad = np.asarray([[0, 2, 1, 2, 0]], np.int64)
        eng.op_teds_cost(dev(tok[:6]), dev(np.asarray([0, 3, 6], np.int32)), dev(bad), np.asarray([0, 3, 6], np.int32), bad, out=out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == CANARY)
    tok[:1024 + 3] = np.arange(1027)                                     # exactly at the limit: accepted
    coff = np.asarray([0, 3, 1027], np.int32)
    eng.op_teds_cost(dev(tok), dev(coff), dev(pairs), coff, pairs, out=out)
    assert out.cpu().numpy()[:4].tolist() == [0.0, 1.0, 1.0, 0.0]                  # 3 tokens against 1024, none in common


# ---- dist -----------------------------------------------------------------------------------------------------------------------------------------
def sized_table(rng, n, sections=(), width=7, alphabet="ab"):
    """a table of exactly n nodes: rows of up to `width` cells, directly under the table or spread over `sections`"""
    if n == 1:
        return R.node("table")
    budget = n - 1 - len(sections)
    rows = []
    while budget > 0:
        cells = min(budget - 1, rng.randint(1, width))
        rows.append(R.node("tr", *[R.td([rng.choice(alphabet) for _ in range(rng.randrange(4))], rng.choice((1, 1, 2)), 1) for _ in range(cells)]))
        budget -= 1 + cells
    if not sections:
        return R.node("table", *rows)
    per = (len(rows) + len(sections) - 1) // len(sections)
    return R.node("table", *[R.node(s, *rows[k * per:(k + 1) * per]) for k, s in enumerate(sections)])


def chain(depth, leaf):
    t = leaf
    for k in range(depth):
        t = R.node("div" if k % 2 else "span", t)
    return R.node("table", t)


def dist_cases():
    rng = random.Random(11)
    T = lambda n, **kw: sized_table(rng, n, **kw)
    three = R.node("table", *[R.node("tr", *[R.td("abc"[c] + "x" * r) for c in range(3)]) for r in range(3)])
    cases = {
        "single": (R.node("table"), R.node("table")),
        "no_rows_vs_3x3": (R.node("table"), three),
        "3x3_vs_no_rows": (three, R.node("table")),
        "chain6": (chain(6, R.td("ab")), chain(4, R.node("tr", R.td("ac")))),
        "chain6_same": (chain(6, R.td("ab")), chain(6, R.td("abc"))),
        "n1_vs_2": (T(1), T(2)),
        "n2": (T(2), T(2)),
        "n12_vs_9": (T(12), T(9)),
        "n63": (T(63), T(63)),
        "n64": (T(64), T(64)),
        "n65_vs_64": (T(65), T(64)),
        "n65_vs_130": (T(65), T(130)),
        "n130": (T(130), T(130)),
        "n7_vs_130": (T(7), T(130)),
        "n130_vs_7": (T(130), T(7)),
        "sections_vs_none": (T(40, sections=("thead", "tbody")), T(40)),
        "wide_sections": (T(300, sections=("thead", "tbody"), width=12), T(290, sections=("thead", "tbody"), width=12)),
        "wide_sections_vs_rows": (T(200, sections=("thead", "tbody", "tfoot")), T(150)),
    }
    same = T(130, sections=("thead", "tbody"))
    cases["identical_130"] = (same, same)
    return cases


@pytest.fixture(scope="module")
def dist_case():
    """flattened pairs and reference distances, computed once"""
    out = {}
    for name, (a, b) in dist_cases().items():
        p = M._prepare(R.to_html(a), R.to_html(b), False, None, False)
        N1, N2 = R.size((a,)), R.size((b,))
        assert (p.t1.n, p.t2.n) == (N1, N2)
        ref = float(R.tree_distance(a, b)) if max(N1, N2) <= 20 else M._host_distance(p)
        out[name] = (p, ref, R.bound(N1, N2))
    return out


def run_dist(eng, flat, canary=4, scratch_bytes=None):
    b = M.pack_batch(flat)
    C = np.zeros(max(b.c_elems, 1))
    for p, rec in zip(flat, b.dist_pairs.tolist()):
        C[rec[12]:rec[12] + p.n_rows * p.n_cols] = M.levenshtein_costs(p.contents, p.n_rows, p.n_cols).ravel()
    out = torch.full((len(flat) + canary,), CANARY, dtype=torch.float64, device="cuda")
    scratch = torch.empty((max(b.scratch_bytes, 8),), dtype=torch.uint8, device="cuda")
    args = (dev(b.dist_pairs), b.dist_pairs, dev(b.node), dev(b.lml), dev(b.kr), dev(b.grp), dev(C), scratch)
    eng.op_teds_dist(*args, out=out, c_elems=b.c_elems, scratch_bytes=scratch_bytes)
    return out, args, b


@pytest.mark.parametrize("name", list(dist_cases().keys()))
def test_dist_single_pair(eng, dist_case, name):
    p, ref, bound = dist_case[name]
    out, args, b = run_dist(eng, [p])
    got = out.cpu().numpy()
    print(f"teds dist {name}: N1 {p.t1.n} N2 {p.t2.n} keyroots {len(p.t1.kr)} x {len(p.t2.kr)} device {got[0]!r} reference {ref!r} "
          f"|diff| {abs(got[0] - ref):.3e} bound {bound:.3e}")
    assert np.all(got[1:] == CANARY)
    assert abs(got[0] - ref) <= bound
    if name == "identical_130":
        assert got[0] == 0.0
    eng.op_teds_dist(*args, out=out, c_elems=b.c_elems)                  # the same buffers again: the scratch of the first call is overwritten
    assert np.array_equal(out.cpu().numpy(), got)


def test_dist_batch_of_different_sizes(eng, dist_case):
    names = ["n7_vs_130", "single", "wide_sections", "n12_vs_9", "n64", "chain6", "n130_vs_7"]
    flat = [dist_case[n][0] for n in names]
    out, _, _ = run_dist(eng, flat)
    got = out.cpu().numpy()
    assert np.all(got[len(names):] == CANARY)
    for n, g in zip(names, got):
        assert abs(g - dist_case[n][1]) <= dist_case[n][2], n


def test_dist_refusals_launch_nothing(eng, dist_case):
    p = dist_case["n12_vs_9"][0]
    b = M.pack_batch([p])
    out = torch.full((4,), CANARY, dtype=torch.float64, device="cuda")
    scratch = torch.empty((b.scratch_bytes,), dtype=torch.uint8, device="cuda")
    C = dev(M.levenshtein_costs(p.contents, p.n_rows, p.n_cols).ravel())
    call = lambda hp, **kw: eng.op_teds_dist(dev(hp), hp, dev(b.node), dev(b.lml), dev(b.kr), dev(b.grp), C, scratch, out=out, c_elems=b.c_elems, **kw)
    big = b.dist_pairs.copy()
    big[0, 0] = 4097
    with pytest.raises(PtError, match="4097"):
        call(big)
    with pytest.raises(PtError, match="scratch"):
        call(b.dist_pairs, scratch_bytes=b.scratch_bytes - 8)
    off = b.dist_pairs.copy()
    off[0, 3] = b.lml.size - p.t2.n + 1                                  # tree 2 would end behind the node arrays
    with pytest.raises(PtError, match="outside the arrays"):
        call(off)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == CANARY)
    from pdf_table_amd.engine import teds_scratch_bytes
    assert teds_scratch_bytes(12, 9) == M.scratch_bytes(12, 9) == b.scratch_bytes == 16 * 12 * 9
    assert teds_scratch_bytes(4096, 4096) == M.scratch_bytes(4096, 4096)
    with pytest.raises(PtError, match="4097"):
        teds_scratch_bytes(4097, 1)
    call(b.dist_pairs)
    assert abs(out.cpu().numpy()[0] - dist_case["n12_vs_9"][1]) <= dist_case["n12_vs_9"][2]
