"""What the TEDS tests compare with: the ordered tree edit distance as the textbook recursion over forests (memoised, on nested tuples, in exact
rationals) and a plain two-row Levenshtein distance.  Nothing here is shared with pdf_table_amd/table_metric.py: trees are written down as nested
tuples by the tests' own generators, which also serialise them to HTML, so the package's parser and flattening are on the tested side.

A tree is ``(label, children)`` with ``children`` a tuple of trees; a label is ``(tag, colspan, rowspan, content)`` with ``content`` a tuple of token
strings for a ``td`` (spans are ints) and ``(tag, None, None, None)`` for every other element."""
import functools
from fractions import Fraction


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def rename(l1, l2):
    if l1[:3] != l2[:3]:
        return Fraction(1)
    if l1[0] == "td" and (l1[3] or l2[3]):
        return Fraction(levenshtein(l1[3], l2[3]), max(len(l1[3]), len(l2[3])))
    return Fraction(0)


def size(forest):
    return sum(1 + size(t[1]) for t in forest)


@functools.lru_cache(maxsize=None)
def forest_distance(F, G):
    if not F:
        return Fraction(size(G))
    if not G:
        return Fraction(size(F))
    v, w = F[-1], G[-1]
    return min(forest_distance(F[:-1] + v[1], G) + 1,
               forest_distance(F, G[:-1] + w[1]) + 1,
               forest_distance(v[1], w[1]) + forest_distance(F[:-1], G[:-1]) + rename(v[0], w[0]))


def tree_distance(t1, t2):
    """exact (a Fraction)"""
    d = forest_distance((t1,), (t2,))
    forest_distance.cache_clear()
    return d


# ---- the tests' own trees: a table spec -> nested tuples, and -> HTML -----------------------------------------------------------------------------
def node(tag, *children):
    return ((tag, None, None, None), tuple(children))


def td(tokens=(), colspan=1, rowspan=1):
    """a cell whose content is plain characters (one token each)"""
    return (("td", colspan, rowspan, tuple(tokens)), ())


def to_html(tree, document=True):
    def ser(t):
        (tag, cs, rs, content), kids = t
        if tag == "td":
            attrs = ("" if cs == 1 else ' colspan="%d"' % cs) + ("" if rs == 1 else ' rowspan="%d"' % rs)
            return "<td%s>%s</td>" % (attrs, "".join(content))
        return "<%s>%s</%s>" % (tag, "".join(ser(k) for k in kids), tag)
    s = ser(tree)
    return "<html><body>%s</body></html>" % s if document else s


def random_table(rng, alphabet="abc"):
    """0-3 rows per section and 0-4 cells per row; optional thead and tbody sections and rows directly under the table; spans 1-2; contents of 0-4
    tokens (single characters of a small alphabet, so that equal and near-equal contents are common)"""
    def row():
        return node("tr", *[td([alphabet[rng.randrange(len(alphabet))] for _ in range(rng.randrange(5))], rng.choice((1, 1, 1, 2)), rng.choice((1, 1, 1, 2)))
                            for _ in range(rng.randrange(5))])
    kids = []
    if rng.random() < 0.5:
        kids.append(node("thead", *[row() for _ in range(rng.randrange(4))]))
    if rng.random() < 0.5:
        kids.append(node("tbody", *[row() for _ in range(rng.randrange(4))]))
    if rng.random() < 0.5 or not kids:
        kids += [row() for _ in range(rng.randrange(4))]
    return node("table", *kids)


def n_nodes(t1, t2):
    return max(size(t1[1]), size(t2[1]))


def bound(N1, N2):
    """|distance - exact| for any float64 evaluation: an edit script has at most N1 + N2 terms of at most 1, each sum rounded once"""
    return (N1 + N2) ** 2 * 2.0 ** -52
