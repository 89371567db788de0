"""TEDS, the Tree-Edit-Distance-based Similarity of two HTML tables (Zhong, ShafieiBavani, Jimeno Yepes: "Image-based table recognition: data, model,
and evaluation", 2020): what ``OcrTableTask.eval`` scores table HTML with (ocr_pdf/ocr_table_task.py:281-285, table/table_metric/table_metric.py).

    TEDS(structure_only=False, n_jobs=1, ignore_nodes=None, engine=None, wrap=False)
        .evaluate(pred, true) -> float
        .batch_evaluate(pred_json, true_json) -> {name: score}
        .batch_evaluate_html(pred_htmls, true_htmls) -> [score]

``engine=None`` is the HOST ROUTE: the standard library's HTML parser, numpy, and Zhang-Shasha in Python floats (float64); ``n_jobs > 1`` spreads a
batch over a process pool.  With a ``HipEngine`` the batch takes the DEVICE ROUTE: the same parser and flattening, then one upload, two launches
(pt_op_teds_cost: every distinct cell content of a table against every distinct content of the other; pt_op_teds_dist: the tree edit distance, one
workgroup per table pair, csrc/teds.hip) and one copy back per chunk of pairs.  A pair the device route refuses -- a tree above 4096 nodes, a cell
above 1024 tokens, a scratch above the budget -- is computed by the host route, and its index is listed in ``last_fallback``.

The metric: an empty string on either side is 0.0; both strings are parsed, the first ``body/table`` of each is taken (none: 0.0); ``ignore_nodes``
removes those tags first and keeps their text and children; n_nodes = the larger count of the tables' descendant elements; each table becomes an
ordered tree in which a ``td`` is a leaf with colspan, rowspan (default 1) and its content tokens, every other element a node with its tag only;
distance = the ordered tree edit distance with insert = delete = 1 and rename = 1 where tag, colspan or rowspan differ, levenshtein(tokens) /
max(len) between two ``td`` of which one has content, 0 otherwise; score = 1 - distance / n_nodes.

Unpinned: lxml, apted and rapidfuzz are not dependencies of this project, so nothing here is compared with their own run.  The tree edit distance is
unique (any exact algorithm gives APTED's value up to the order of its sums); the parser is the standard library's, and lxml's recovery from malformed
HTML is not restated: a close tag that does not match the open element raises ValueError."""
from __future__ import annotations

from html.parser import HTMLParser
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_NODES = 4096        # pt_op_teds_dist: nodes per tree
MAX_TOKENS = 1024       # pt_op_teds_cost: tokens per cell content
_VOID = frozenset(["area", "base", "br", "col", "embed", "hr", "img", "input", "link", "meta", "param", "source", "track", "wbr"])


# ---- parser -------------------------------------------------------------------------------------------------------------------------------------
class _Element:
    __slots__ = ("tag", "attrib", "text", "tail", "children")

    def __init__(self, tag: str, attrib: Dict[str, str]):
        self.tag, self.attrib, self.text, self.tail, self.children = tag, attrib, None, None, []


class _TreeBuilder(HTMLParser):
    """Elements with text and tail as lxml / ElementTree keep them; comments, declarations and processing instructions are dropped."""

    def __init__(self, src: str):
        super().__init__(convert_charrefs=True)
        self.roots: List[_Element] = []
        self.stack: List[_Element] = []
        self._lines = None
        self._src = src

    def _offset(self) -> int:
        if self._lines is None:
            self._lines = [0]
            for ln in self._src.split("\n"):
                self._lines.append(self._lines[-1] + len(ln) + 1)
        line, col = self.getpos()
        return self._lines[line - 1] + col

    def _open(self, tag, attrs, push):
        el = _Element(tag, {k: ("" if v is None else v) for k, v in attrs})
        (self.stack[-1].children if self.stack else self.roots).append(el)
        if push and tag not in _VOID:
            self.stack.append(el)

    def handle_starttag(self, tag, attrs):
        self._open(tag, attrs, True)

    def handle_startendtag(self, tag, attrs):
        self._open(tag, attrs, False)

    def handle_endtag(self, tag):
        if tag in _VOID:
            return
        if not self.stack or self.stack[-1].tag != tag:
            raise ValueError(f"malformed HTML: </{tag}> at offset {self._offset()} closes "
                             f"{'<' + self.stack[-1].tag + '>' if self.stack else 'nothing'}")
        self.stack.pop()

    def handle_data(self, data):
        if not self.stack:
            return
        el = self.stack[-1]
        if el.children:
            el.children[-1].tail = (el.children[-1].tail or "") + data
        else:
            el.text = (el.text or "") + data


def parse_html(src: str) -> Optional[_Element]:
    """The first top-level element of `src` (elements left open at the end are closed there), or None."""
    b = _TreeBuilder(src)
    b.feed(src)
    b.close()
    return b.roots[0] if b.roots else None


def _find_table(root: Optional[_Element]) -> Optional[_Element]:
    """xpath ``body/table`` from an ``html`` root; any other root has no such path (a bare ``<table>`` fragment's root is the table itself)."""
    if root is None or root.tag != "html":
        return None
    for body in root.children:
        if body.tag == "body":
            for t in body.children:
                if t.tag == "table":
                    return t
    return None


def _strip_tags(el: _Element, tags) -> None:
    """lxml's strip_tags below `el`: an element with one of `tags` goes, its text, children and tail stay in its place"""
    old, el.children = el.children, []

    def text(s):
        if s:
            if el.children:
                el.children[-1].tail = (el.children[-1].tail or "") + s
            else:
                el.text = (el.text or "") + s

    for ch in old:
        _strip_tags(ch, tags)
        if ch.tag in tags:
            text(ch.text)
            el.children.extend(ch.children)
            text(ch.tail)
        else:
            el.children.append(ch)


def _count_descendants(el: _Element) -> int:
    n, todo = 0, list(el.children)
    while todo:
        e = todo.pop()
        n += 1
        todo.extend(e.children)
    return n


def _cell_tokens(td: _Element) -> Tuple[str, ...]:
    out: List[str] = []

    def walk(e, top):
        if not top:
            out.append("<%s>" % e.tag)
        if e.text:
            out.extend(e.text)
        for c in e.children:
            walk(c, False)
        if not top and e.tag != "unk":
            out.append("</%s>" % e.tag)
        if not top and e.tag != "td" and e.tail:
            out.extend(e.tail)

    walk(td, True)
    return tuple(out)


# ---- flattening (shared by both routes) ----------------------------------------------------------------------------------------------------------
class FlatTree:
    """A table in postorder: per node tag id, colspan, rowspan (-1 where none), leftmost leaf, height and content id (-1 where none); its keyroots
    ordered by (height, size descending) and the offsets of their height groups."""
    __slots__ = ("n", "tag", "colspan", "rowspan", "lml", "height", "cid", "kr", "grp")


def _flatten(table: _Element, structure_only: bool, tag_ids: Dict[str, int], tok_ids: Dict[str, int], cont_ids: Dict[tuple, int],
             contents: List[np.ndarray]) -> FlatTree:
    tag, cs, rs, lml, hgt, cid = [], [], [], [], [], []
    # iterative postorder: (element, next child) frames; a td is a leaf
    stack = [[table, 0, -1, 0]]          # element, child cursor, leftmost leaf, height so far
    while stack:
        fr = stack[-1]
        el = fr[0]
        kids = () if el.tag == "td" else el.children
        if fr[1] < len(kids):
            fr[1] += 1
            stack.append([kids[fr[1] - 1], 0, -1, 0])
            continue
        stack.pop()
        me = len(tag)
        tag.append(tag_ids.setdefault(el.tag, len(tag_ids)))
        if el.tag == "td":
            cs.append(int(el.attrib.get("colspan", "1")))
            rs.append(int(el.attrib.get("rowspan", "1")))
            toks = () if structure_only else _cell_tokens(el)
            key = tuple(tok_ids.setdefault(t, len(tok_ids)) for t in toks)
            k = cont_ids.get(key)
            if k is None:
                k = cont_ids[key] = len(contents)
                contents.append(np.asarray(key, dtype=np.int32))
            cid.append(k)
        else:
            cs.append(-1)
            rs.append(-1)
            cid.append(-1)
        lml.append(me if fr[2] < 0 else fr[2])
        hgt.append(fr[3])
        if stack:
            up = stack[-1]
            if up[2] < 0:
                up[2] = lml[me]
            up[3] = max(up[3], fr[3] + 1)
    t = FlatTree()
    t.n = len(tag)
    t.tag, t.colspan, t.rowspan, t.lml, t.height, t.cid = (np.asarray(a, dtype=np.int32) for a in (tag, cs, rs, lml, hgt, cid))
    last = {}
    for i, l in enumerate(lml):
        last[l] = i                      # a keyroot is the highest node of its leftmost leaf
    kr = np.asarray(sorted(last.values()), dtype=np.int32)
    size = kr - t.lml[kr] + 1
    order = np.lexsort((kr, -size, t.height[kr]))
    t.kr = kr[order]
    h = t.height[t.kr]
    t.grp = np.concatenate([[0], np.flatnonzero(np.diff(h)) + 1, [len(h)]]).astype(np.int32)
    return t


class FlatPair:
    """Two flattened tables with their contents interned together: equal token tuples share one id, token strings are int32 ids.  Contents
    0 .. n_rows - 1 are the first table's (the rows of the cost matrix), all n_cols contents are the columns."""
    __slots__ = ("t1", "t2", "contents", "n_rows", "n_cols", "n_nodes")


def _prepare(pred: str, true: str, structure_only: bool, ignore_nodes, wrap: bool) -> Optional[FlatPair]:
    if (not pred) or (not true):
        return None
    tables = []
    for src in (pred, true):
        if wrap and src.lstrip()[:6].lower() == "<table":
            src = "<html><body>" + src + "</body></html>"
        t = _find_table(parse_html(src))
        if t is None:
            return None
        if ignore_nodes:
            _strip_tags(t, frozenset(ignore_nodes))
        tables.append(t)
    p = FlatPair()
    p.n_nodes = max(_count_descendants(tables[0]), _count_descendants(tables[1]))
    tag_ids, tok_ids, cont_ids, contents = {}, {}, {}, []
    p.t1 = _flatten(tables[0], structure_only, tag_ids, tok_ids, cont_ids, contents)
    p.n_rows = len(contents)
    p.t2 = _flatten(tables[1], structure_only, tag_ids, tok_ids, cont_ids, contents)
    p.n_cols = len(contents)
    p.contents = contents
    return p


# ---- host route -----------------------------------------------------------------------------------------------------------------------------------
def levenshtein_costs(contents: Sequence[np.ndarray], n_rows: int, n_cols: int) -> np.ndarray:
    """float64 [n_rows, n_cols]: levenshtein(contents[r], contents[c]) / max(len), 0 where both are empty.  The row-wise recurrence on all content
    pairs at once: t[j] = min(up + 1, diag + sub), then the insert chain cur[j] = min_k<=j (t[k] + j - k) as a running minimum of t[k] - k."""
    out = np.zeros((n_rows, n_cols), dtype=np.float64)
    if n_rows == 0 or n_cols == 0:
        return out
    la = np.asarray([len(contents[r]) for r in range(n_rows)], dtype=np.int64)
    lb = np.asarray([len(contents[c]) for c in range(n_cols)], dtype=np.int64)
    N = int(lb.max())
    B = np.full((n_cols, max(N, 1)), -2, dtype=np.int64)
    for c in range(n_cols):
        B[c, :lb[c]] = contents[c]
    B = B[:, :N]
    ar = np.arange(N + 1, dtype=np.int32)
    cols = np.arange(n_cols)
    dist = np.zeros((n_rows, n_cols), dtype=np.int64)
    step = max(1, (4 << 20) // max(1, n_cols * (N + 1)))
    order = np.argsort(la, kind="stable")
    for s in range(0, n_rows, step):
        rows = order[s:s + step]
        M = int(la[rows].max())
        A = np.full((len(rows), max(M, 1)), -1, dtype=np.int64)
        for k, r in enumerate(rows):
            A[k, :la[r]] = contents[r]
        prev = np.broadcast_to(ar, (len(rows), n_cols, N + 1)).copy()
        done = la[rows] == 0
        dist[rows[done]] = lb[None, :]
        for i in range(1, M + 1):
            sub = (A[:, i - 1, None, None] != B[None, :, :]).astype(np.int32)
            cur = np.empty_like(prev)
            cur[..., 0] = i
            np.minimum(prev[..., 1:] + 1, prev[..., :-1] + sub, out=cur[..., 1:])
            cur -= ar
            np.minimum.accumulate(cur, axis=-1, out=cur)
            cur += ar
            prev = cur
            hit = np.flatnonzero(la[rows] == i)
            if len(hit):
                dist[rows[hit]] = prev[hit][:, cols, lb]
    longest = np.maximum(la[:, None], lb[None, :])
    np.divide(dist.astype(np.float64), longest.astype(np.float64), out=out, where=longest > 0)
    return out


def rename_costs(p: FlatPair, C: np.ndarray) -> np.ndarray:
    """float64 [n1, n2]: 1 where tag, colspan or rowspan differ, else the cells' content cost, else 0"""
    a, b = p.t1, p.t2
    same = (a.tag[:, None] == b.tag[None, :]) & (a.colspan[:, None] == b.colspan[None, :]) & (a.rowspan[:, None] == b.rowspan[None, :])
    R = np.where(same, 0.0, 1.0)
    i1, i2 = np.flatnonzero(a.cid >= 0), np.flatnonzero(b.cid >= 0)
    if len(i1) and len(i2):
        sub = C[a.cid[i1]][:, b.cid[i2]]
        blk = R[np.ix_(i1, i2)]
        R[np.ix_(i1, i2)] = np.where(same[np.ix_(i1, i2)], sub, blk)
    return R


def zhang_shasha(t1: FlatTree, t2: FlatTree, R: np.ndarray) -> float:
    """The ordered tree edit distance with insert = delete = 1 and rename costs R (<= 1), in Python floats (float64).  Keyroot pairs in the classic
    order (ascending postorder index), one forest-distance table per pair."""
    l1, l2 = t1.lml.tolist(), t2.lml.tolist()
    Rl = R.tolist()
    TD = [row[:] for row in Rl]          # leaf against leaf: min(2, rename) = rename; every other entry is written before it is read
    kr1, kr2 = sorted(t1.kr.tolist()), sorted(t2.kr.tolist())
    for k1 in kr1:
        a = l1[k1]
        m = k1 - a + 2
        for k2 in kr2:
            b = l2[k2]
            if a == k1 and b == k2:
                continue
            n = k2 - b + 2
            fd = [[0.0] * n for _ in range(m)]
            fd[0] = [float(y) for y in range(n)]
            for xx in range(1, m):
                i = a + xx - 1
                fx, fu = fd[xx], fd[xx - 1]
                left = fx[0] = float(xx)
                TDi, Ri = TD[i], Rl[i]
                spine = l1[i] == a
                base = fd[l1[i] - a]
                for y in range(1, n):
                    j = b + y - 1
                    v = fu[y] + 1.0
                    w = left + 1.0
                    if w < v:
                        v = w
                    if spine and l2[j] == b:
                        w = fu[y - 1] + Ri[j]
                        if w < v:
                            v = w
                        TDi[j] = v
                    else:
                        w = base[l2[j] - b] + TDi[j]
                        if w < v:
                            v = w
                    fx[y] = left = v
    return TD[t1.n - 1][t2.n - 1]


def _host_distance(p: FlatPair) -> float:
    return zhang_shasha(p.t1, p.t2, rename_costs(p, levenshtein_costs(p.contents, p.n_rows, p.n_cols)))


def _host_score(args) -> float:
    pred, true, structure_only, ignore_nodes, wrap = args
    p = _prepare(pred, true, structure_only, ignore_nodes, wrap)
    if p is None:
        return 0.0
    return _score(_host_distance(p), p.n_nodes)


def _score(distance: float, n_nodes: int) -> float:
    """1 - distance / n_nodes; two tables without any element below them (the reference divides by zero there) are identical: 1.0"""
    return 1.0 - distance / n_nodes if n_nodes else 1.0


# ---- device route ---------------------------------------------------------------------------------------------------------------------------------
def scratch_bytes(n1: int, n2: int) -> int:
    """pt_op_teds_scratch_bytes: two n1 x n2 float64 planes"""
    return 16 * int(n1) * int(n2)


def device_refuses(p: FlatPair, budget: int) -> bool:
    return (p.t1.n > MAX_NODES or p.t2.n > MAX_NODES or any(len(c) > MAX_TOKENS for c in p.contents)
            or scratch_bytes(p.t1.n, p.t2.n) + 8 * p.n_rows * p.n_cols > budget)


class PackedBatch:
    """The host arrays of one pt_op_teds_cost + pt_op_teds_dist call over `pairs` (names as in include/pdftable_hip.h)"""
    __slots__ = ("tok", "coff", "cost_pairs", "node", "lml", "kr", "grp", "dist_pairs", "c_elems", "scratch_bytes")


def pack_batch(pairs: Sequence[FlatPair]) -> PackedBatch:
    b = PackedBatch()
    toks, coff, cost_pairs, node, lml, kr, grp, dist_pairs = [], [0], [], [], [], [], [], []
    n_nodes = n_kr = n_grp = c_off = s_off = 0
    for p in pairs:
        c0 = len(coff) - 1
        for c in p.contents:
            toks.append(c)
            coff.append(coff[-1] + len(c))
        cost_pairs.append((c0, p.n_rows, c0, p.n_cols, c_off))
        rec = []
        for t in (p.t1, p.t2):
            node.append(np.stack([t.tag, t.colspan, t.rowspan, t.cid], axis=1))
            lml.append(t.lml)
            rec += [t.n, n_nodes]
            n_nodes += t.n
        for t in (p.t1, p.t2):
            kr.append(t.kr)
            grp.append(t.grp)
            rec += [n_kr, len(t.kr), n_grp, len(t.grp) - 1]
            n_kr += len(t.kr)
            n_grp += len(t.grp)
        dist_pairs.append(rec + [c_off, p.n_rows, p.n_cols, s_off])
        c_off += p.n_rows * p.n_cols
        s_off += 2 * p.t1.n * p.t2.n
    cat = lambda parts, dt, shape=(0,): np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros(shape, dtype=dt)
    b.tok = cat(toks, np.int32)
    b.coff = np.asarray(coff, dtype=np.int32)
    b.cost_pairs = np.asarray(cost_pairs, dtype=np.int64).reshape(-1, 5)
    b.node = np.ascontiguousarray(cat(node, np.int32, (0, 4)))
    b.lml, b.kr, b.grp = cat(lml, np.int32), cat(kr, np.int32), cat(grp, np.int32)
    b.dist_pairs = np.asarray(dist_pairs, dtype=np.int64).reshape(-1, 16)
    b.c_elems, b.scratch_bytes = c_off, 8 * s_off
    return b


def device_distances(engine, pairs: Sequence[FlatPair], events: Optional[list] = None) -> np.ndarray:
    """float64 [len(pairs)]: one upload, pt_op_teds_cost, pt_op_teds_dist, one copy back.  events: a list that receives the three device events around
    the two launches (tools/teds_bench.py times the kernels alone with them)."""
    import torch
    b = pack_batch(pairs)
    parts = [b.cost_pairs.view(np.uint8).ravel(), b.dist_pairs.view(np.uint8).ravel(), b.node.view(np.uint8).ravel()]
    parts += [a.view(np.uint8).ravel() for a in (b.tok, b.coff, b.lml, b.kr, b.grp)]
    offs, total = [], 0
    for a in parts:
        offs.append(total)
        total += (a.size + 15) // 16 * 16
    host = torch.empty((max(total, 16),), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    for o, a in zip(offs, parts):
        hv[o:o + a.size] = a
    dev = host.to(engine._tdev, non_blocking=True)

    def view(k, dtype, shape):
        n = parts[k].size
        return dev[offs[k]:offs[k] + n].view(dtype).reshape(shape)

    cost_pairs, dist_pairs = view(0, torch.int64, (-1, 5)), view(1, torch.int64, (-1, 16))
    node = view(2, torch.int32, (-1, 4))
    tok, coff, lml, kr, grp = (view(k, torch.int32, (-1,)) for k in range(3, 8))
    C = torch.empty((max(b.c_elems, 1),), dtype=torch.float64, device=engine._tdev)
    scratch = torch.empty((max(b.scratch_bytes, 8),), dtype=torch.uint8, device=engine._tdev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if events is not None else None
    if ev:
        ev[0].record()
    engine.op_teds_cost(tok, coff, cost_pairs, b.coff, b.cost_pairs, C, c_elems=b.c_elems)
    if ev:
        ev[1].record()
    out = engine.op_teds_dist(dist_pairs, b.dist_pairs, node, lml, kr, grp, C, scratch, c_elems=b.c_elems)
    if ev:
        ev[2].record()
        events.append(ev)
    return out.cpu().numpy()


# ---- the public interface -------------------------------------------------------------------------------------------------------------------------
class TEDS:
    """Tree Edit Distance based Similarity (see the module docstring).  scratch_budget: bytes of device memory one chunk of the device route may take
    for its cost matrices and distance planes."""

    def __init__(self, structure_only: bool = False, n_jobs: int = 1, ignore_nodes=None, engine=None, wrap: bool = False):
        if not (isinstance(n_jobs, int) and n_jobs >= 1):
            raise ValueError("n_jobs must be an integer >= 1")
        self.structure_only = structure_only
        self.n_jobs = n_jobs
        self.ignore_nodes = ignore_nodes
        self.engine = engine
        self.wrap = wrap
        self.scratch_budget = 1 << 30
        self.max_pairs = 4096
        self.last_fallback: List[int] = []
        self.events = None          # a list: receives the device events of every chunk (device_distances)
        self._pool = None

    def _args(self, pred, true):
        return (pred, true, self.structure_only, self.ignore_nodes, self.wrap)

    def evaluate(self, pred: str, true: str) -> float:
        return self._batch([pred], [true])[0]

    def _batch(self, preds, trues) -> List[float]:
        preds, trues = list(preds), list(trues)
        n = min(len(preds), len(trues))
        self.last_fallback = []
        if self.engine is None:
            return self._host([self._args(preds[k], trues[k]) for k in range(n)])
        scores = [0.0] * n
        flat = [_prepare(preds[k], trues[k], self.structure_only, self.ignore_nodes, self.wrap) for k in range(n)]
        todo, host = [], []
        for k, p in enumerate(flat):
            if p is None:
                continue                                             # an empty or table-less side: 0.0 without a launch
            (host if device_refuses(p, self.scratch_budget) else todo).append(k)
        for k in host:
            scores[k] = _score(_host_distance(flat[k]), flat[k].n_nodes)
        self.last_fallback = host
        for chunk in self._chunks(flat, todo):
            d = device_distances(self.engine, [flat[q] for q in chunk], self.events)
            for q, dq in zip(chunk, d.tolist()):
                scores[q] = _score(dq, flat[q].n_nodes)
        return scores

    def _chunks(self, flat, todo):
        """the device route's calls: indices of `todo` in order, cut where the scratch budget or max_pairs is reached"""
        chunk, used = [], 0
        for k in todo:
            need = scratch_bytes(flat[k].t1.n, flat[k].t2.n) + 8 * flat[k].n_rows * flat[k].n_cols
            if chunk and (used + need > self.scratch_budget or len(chunk) >= self.max_pairs):
                yield chunk
                chunk, used = [], 0
            chunk.append(k)
            used += need
        if chunk:
            yield chunk

    def _host(self, args) -> List[float]:
        if self.n_jobs == 1 or len(args) < 2:
            return [_host_score(a) for a in args]
        if self._pool is None:
            import multiprocessing
            self._pool = multiprocessing.get_context("spawn").Pool(self.n_jobs)
        return self._pool.map(_host_score, args, chunksize=1)

    def close(self) -> None:
        """Ends the process pool of the host route, if one was started"""
        if self._pool is not None:
            self._pool.terminate()
            self._pool.join()
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch_evaluate(self, pred_json: Dict[str, str], true_json: Dict[str, Dict[str, str]]) -> Dict[str, float]:
        """pred_json {name: html}, true_json {name: {'html': html}} -> {name: score} in true_json's order; a missing prediction scores 0.0"""
        names = list(true_json.keys())
        return dict(zip(names, self._batch([pred_json.get(k, "") for k in names], [true_json[k]["html"] for k in names])))

    def batch_evaluate_html(self, pred_htmls: Sequence[str], true_htmls: Sequence[str]) -> List[float]:
        return self._batch(pred_htmls, true_htmls)
