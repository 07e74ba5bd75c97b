"""What the covariation tests share: the definitions of Covariation restated twice in plain Python, and the alignments.

The NAIVE reference classifies bytes with string operations and forms cov as the sum, over itertools.combinations of the rows
that hold a canonical pair, of the Hamming distance of the two two-letter strings: no count table.  It is for tiny shapes
(R <= 12, L <= 40).  The COUNT reference counts the rows of every pair type and weighs the products with the distance table;
the tests first assert it equal to the naive one on tiny shapes and then use it at the larger ones."""
import itertools
import random
from collections import Counter

TYPES = ("AU", "UA", "GC", "CG", "GU", "UG")
GAPS = "-.~"
#: the tests' alphabet: both cases, T, the three gap characters, a letter that is no base and a separator
ALPHABET = "ACGUacgutT-.~N&"
#: d(t, t'), rows and columns in the order of TYPES
D = ((0, 2, 2, 2, 1, 2), (2, 0, 2, 2, 2, 1), (2, 2, 0, 2, 1, 2), (2, 2, 2, 0, 2, 1), (1, 2, 1, 2, 0, 2), (2, 1, 2, 1, 2, 0))
EVERY_CELL = dict(minspan=1, min_rows=0, min_cov=0)
DEFAULTS = dict(minspan=4, min_rows=1, min_cov=1)


def normalise(row):
    return row.upper().replace("T", "U")


def hamming(p, q):
    return sum(x != y for x, y in zip(p, q))


def naive_cell(rows, v, w):
    """(seven counts, cov) of columns v < w, rows as given."""
    pairs = [normalise(r)[v] + normalise(r)[w] for r in rows]
    counts = [pairs.count(t) for t in TYPES] + [sum(p[0] in GAPS and p[1] in GAPS for p in pairs)]
    cov = sum(hamming(p, q) for p, q in itertools.combinations([p for p in pairs if p in TYPES], 2))
    return counts, cov


def _columns(rows):
    rows = [normalise(r) for r in rows]
    return ["".join(r[c] for r in rows) for c in range(len(rows[0]))]


_MEMO = {}


def count_columns(col_v, col_w):
    """(seven counts, cov) of two columns given as strings of normalised letters, with per-type counts and the table D; formed
    once per distinct pair of column strings."""
    key = (col_v, col_w)
    if key not in _MEMO:
        if len(_MEMO) > 1 << 18:
            _MEMO.clear()
        seen = Counter(zip(col_v, col_w))
        c = [seen[(t[0], t[1])] for t in TYPES]
        both = sum(n for (x, y), n in seen.items() if x in GAPS and y in GAPS)
        _MEMO[key] = (c + [both], sum(c[s] * c[t] * D[s][t] for s in range(6) for t in range(s + 1, 6)))
    return _MEMO[key]


def count_cells(rows):
    """{(v, w): (seven counts, cov)} of every v < w: the count reference."""
    cols = _columns(rows)
    return {(v, w): count_columns(cols[v], cols[w]) for v in range(len(cols)) for w in range(v + 1, len(cols))}


def count_select(rows, minspan=4, min_rows=1, min_cov=1):
    """select(count_cells(rows), ...) without the dict of every cell, for alignments of many columns."""
    cols, out = _columns(rows), []
    for v in range(len(cols)):
        for w in range(v + max(minspan, 1), len(cols)):
            c, cov = count_columns(cols[v], cols[w])
            if cov >= min_cov and sum(c[:6]) >= min_rows:
                out.append((v, w, c, cov))
    return out


def naive_cells(rows):
    assert len(rows) <= 12 and len(rows[0]) <= 40, "the naive reference is for tiny shapes"
    L = len(rows[0])
    return {(v, w): naive_cell(rows, v, w) for v in range(L) for w in range(v + 1, L)}


def select(cells, minspan=4, min_rows=1, min_cov=1):
    """The cells a scan emits: [(v, w, counts, cov)] sorted by (v, w)."""
    return [(v, w, c, cov) for (v, w), (c, cov) in sorted(cells.items())
            if w - v >= minspan and sum(c[:6]) >= min_rows and cov >= min_cov]


def random_rows(seed, R, L, alphabet=ALPHABET, helices=2):
    """R rows of L characters of `alphabet`; where they fit, `helices` planted helices whose column pairs hold a canonical
    pair in most rows, with the pair type drawn per row (covariation) and a few rows mutated (incompatible rows)."""
    rng = random.Random(seed)
    rows = [[rng.choice(alphabet) for _ in range(L)] for _ in range(R)]
    for h in range(helices):
        n = min(5, (L - 4) // (2 * helices))
        if n < 1:
            break
        i0 = rng.randrange(0, L - 2 * n - 3)
        j0 = rng.randrange(i0 + 2 * n + 3, L) if i0 + 2 * n + 3 < L else L - 1
        for k in range(n):
            for r in range(R):
                if rng.random() < 0.85:
                    t = rng.choice(TYPES)
                    rows[r][i0 + k], rows[r][j0 - k] = t[0], t[1]
    return ["".join(r) for r in rows]


def check_records(got_cols, got_counts, got_cov, expected, what=""):
    """Record lists (host lists) against select()'s / the given pairs' expectation, in the same order."""
    assert len(got_cols) == len(got_counts) == len(got_cov) == len(expected), (what, len(got_cols), len(expected))
    for k, (v, w, c, cov) in enumerate(expected):
        assert tuple(got_cols[k]) == (v, w) and list(got_counts[k]) == list(c) and got_cov[k] == cov, \
            (what, k, got_cols[k], got_counts[k], got_cov[k], (v, w, c, cov))
