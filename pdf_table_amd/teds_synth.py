"""Seeded PubTabNet-like (truth, prediction) table HTML for the TEDS tests and tools/teds_bench.py: a ``thead`` of one or two bold rows and a ``tbody``,
cells of a few characters (one token each), some column and row spans; the prediction is the truth with seeded edits -- some cells' text perturbed, now and
then a row dropped and a span changed.  No file is read; the same arguments give the same strings."""
from __future__ import annotations

import random
from typing import List, Sequence, Tuple

_ALPHABET = "abcdefghijklmnopqrstuvwxyz0123456789 .,-%"


def _serialise(sections, document: bool) -> str:
    out = ["<table>"]
    for name, rows in sections:
        out.append("<%s>" % name)
        for row in rows:
            out.append("<tr>")
            for text, cs, rs, bold in row:
                attrs = ("" if cs == 1 else ' colspan="%d"' % cs) + ("" if rs == 1 else ' rowspan="%d"' % rs)
                out.append("<td%s>%s</td>" % (attrs, "<b>%s</b>" % text if bold and text else text))
            out.append("</tr>")
        out.append("</%s>" % name)
    out.append("</table>")
    s = "".join(out)
    return "<html><body>" + s + "</body></html>" if document else s


def table_pairs(n: int, seed: int = 0, rows: Sequence[int] = (20, 40), cols: Sequence[int] = (8, 15), tokens: Sequence[int] = (3, 20),
                document: bool = True, edit_rate: float = 0.08) -> Tuple[List[str], List[str]]:
    """(predictions, truths): n pairs of tables of rows[0] .. rows[1] rows and cols[0] .. cols[1] columns with tokens[0] .. tokens[1] characters a cell
    (one cell in ten is empty); document=False gives bare ``<table>`` fragments (TEDS(wrap=True))"""
    rng = random.Random(seed)
    preds, trues = [], []
    for _ in range(n):
        nr, nc = rng.randint(*rows), rng.randint(*cols)
        n_head = rng.randint(1, 2)
        words = ["".join(rng.choice(_ALPHABET) for _ in range(rng.randint(*tokens))) for _ in range(12)]      # tables repeat cell texts

        def text():
            r = rng.random()
            if r < 0.1:
                return ""
            if r < 0.3:
                return rng.choice(words)
            return "".join(rng.choice(_ALPHABET) for _ in range(rng.randint(*tokens)))

        grid = []
        for r in range(nr):
            row, c = [], 0
            while c < nc:
                cs = 2 if c + 1 < nc and rng.random() < 0.05 else 1
                rs = 2 if rng.random() < 0.02 else 1
                row.append((text(), cs, rs, r < n_head))
                c += cs
            grid.append(row)
        pred = [list(row) for row in grid]
        for row in pred:
            for k, (t, cs, rs, bold) in enumerate(row):
                if t and rng.random() < edit_rate:
                    q = rng.randrange(len(t))
                    t = t[:q] + (rng.choice(_ALPHABET) if rng.random() < 0.7 else "") + t[q + 1:]
                    row[k] = (t, cs, rs, bold)
        if rng.random() < 0.3 and len(pred) > n_head + 1:
            del pred[rng.randrange(n_head, len(pred))]
        if rng.random() < 0.3:
            row = pred[rng.randrange(len(pred))]
            k = rng.randrange(len(row))
            t, cs, rs, bold = row[k]
            row[k] = (t, 3 - cs, rs, bold)
        n_head_p = min(n_head, len(pred))
        trues.append(_serialise([("thead", grid[:n_head]), ("tbody", grid[n_head:])], document))
        preds.append(_serialise([("thead", pred[:n_head_p]), ("tbody", pred[n_head_p:])], document))
    return preds, trues
