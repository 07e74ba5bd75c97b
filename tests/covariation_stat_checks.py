"""What the covariation-statistics tests share: the definitions of CovariationStatistics restated in plain Python, and the
float bound.

The reference keeps a dict of counts per cell (collections.Counter over the rows' two letters), takes every logarithm with
math.log of one true quotient of Python ints and every sum with math.fsum; it knows neither the numpy fallback's one-hot
products nor the header's bit planes.

The float bound.  The counters are integers and exact, so the reference and the code under test start from the same numbers.
A term of S costs a few ulp (one division, one fp64 log, one product) and S is a sum of at most 16 terms, whatever L.  A
column sum has at most L - 1 addends of one sign (S >= 0 up to its own rounding): added in any order it errs by at most
(L - 1) ulp/2 = (L - 1) * 2^-53 of the sum, on top of the few ulp of every addend; the corrections are three or four more
operations.  So the error of any number is below about (L + 8) * 2^-53 of its scale: 2^-46 at L = 3 tiles + 1 = 97, 2^-42 at
the largest shape of the tests, L = 64 tiles + 1 = 2049.  The bound is BOUND = 2^-40 of the scale for every shape, a factor 4
and more above that.  The scale of `raw` is the sum of the absolute terms of S, that of `value` is |S| + |the correction
term|, that of a column mean is the mean itself."""
import math
from collections import Counter

from tests.covariation_checks import TYPES, normalise

LETTERS = "ACGU"
CELLS = tuple(a + b for a in LETTERS for b in LETTERS)
STATISTICS = ("mi", "gt", "chi")
CORRECTIONS = (None, "apc", "asc")
BOUND = 2.0 ** -40
EVERY_CELL = dict(minspan=1, min_rows=0, min_stat=None)
DEFAULTS = dict(minspan=4, min_rows=1, min_stat=None)


def columns(rows):
    rows = [normalise(r) for r in rows]
    return ["".join(r[c] for r in rows) for c in range(len(rows[0]))]


def joint(col_v, col_w):
    """[n[a * 4 + b]] of two columns given as strings of normalised letters."""
    seen = Counter(zip(col_v, col_w))
    return [seen[(a, b)] for a in LETTERS for b in LETTERS]


def raw_terms(n, statistic):
    """The terms of S in the table's order (gt: each already doubled)."""
    N = sum(n)
    if N == 0:
        return []
    na = [sum(n[a * 4 + b] for b in range(4)) for a in range(4)]
    nb = [sum(n[a * 4 + b] for a in range(4)) for b in range(4)]
    terms = []
    for a in range(4):
        for b in range(4):
            x = n[a * 4 + b]
            if statistic == "chi":
                if na[a] * nb[b] > 0:
                    e = na[a] * nb[b] / N
                    terms.append((x - e) ** 2 / e)
            elif x > 0:
                l = math.log(x * N / (na[a] * nb[b]))
                terms.append(x / N * l if statistic == "mi" else 2 * x * l)
    return terms


_MEMO = {}


def cell(col_v, col_w):
    """(n, {statistic: (S, the sum of its absolute terms)}) of two column strings, formed once per distinct pair of them."""
    key = (col_v, col_w)
    if key not in _MEMO:
        if len(_MEMO) > 1 << 18:
            _MEMO.clear()
        n = joint(col_v, col_w)
        stats = {}
        for s in STATISTICS:
            terms = raw_terms(n, s)
            stats[s] = (math.fsum(terms), math.fsum(abs(t) for t in terms))
        _MEMO[key] = (n, stats)
    return _MEMO[key]


class Reference:
    """Every cell v < w of an alignment: .n[(v, w)], .S[statistic][(v, w)], .scale[statistic][(v, w)], and per statistic the
    column means .mean[statistic][c] and .mean_all[statistic]."""

    def __init__(self, rows):
        cols = columns(rows)
        L = self.L = len(cols)
        self.n, self.S, self.scale = {}, {s: {} for s in STATISTICS}, {s: {} for s in STATISTICS}
        for v in range(L):
            for w in range(v + 1, L):
                n, stats = cell(cols[v], cols[w])
                self.n[(v, w)] = n
                for s in STATISTICS:
                    self.S[s][(v, w)], self.scale[s][(v, w)] = stats[s]
        self.mean, self.mean_all = {}, {}
        for s in STATISTICS:
            S = self.S[s]
            self.mean[s] = [math.fsum(S[(min(c, d), max(c, d))] for d in range(L) if d != c) / (L - 1) if L > 1 else 0.0 for c in range(L)]
            self.mean_all[s] = math.fsum(S.values()) / (L * (L - 1) // 2) if L > 1 else 0.0

    def term(self, statistic, correction, v, w):
        """The correction term: C = S - term."""
        m, mall = self.mean[statistic], self.mean_all[statistic]
        if correction == "apc":
            return m[v] * m[w] / mall if mall != 0 else 0.0
        if correction == "asc":
            return m[v] + m[w] - mall
        return 0.0

    def value(self, statistic, correction, v, w):
        return self.S[statistic][(v, w)] - self.term(statistic, correction, v, w)

    def record(self, statistic, correction, v, w):
        """(v, w, n, S, C)."""
        return v, w, self.n[(v, w)], self.S[statistic][(v, w)], self.value(statistic, correction, v, w)

    def select(self, statistic, correction, minspan=4, min_rows=1, min_stat=None):
        """The records a scan emits, sorted by (v, w)."""
        return [self.record(statistic, correction, v, w) for (v, w) in sorted(self.n)
                if w - v >= minspan and sum(self.n[(v, w)]) >= min_rows
                and (min_stat is None or self.value(statistic, correction, v, w) >= min_stat)]

    def gap_threshold(self, statistic, correction, minspan=4, min_rows=1):
        """(a threshold in the middle of the widest gap of the sorted values of the cells in scope, half that gap)."""
        vals = sorted(r[4] for r in self.select(statistic, correction, minspan, min_rows))
        gap, k = max((b - a, k) for k, (a, b) in enumerate(zip(vals, vals[1:])))
        return (vals[k] + vals[k + 1]) / 2, gap / 2


def check_records(ref, statistic, correction, cols, joint_, raw, value, expected, what="", bound=BOUND):
    """Record lists (host lists) against the reference's records, in the same order: pairs and counters exactly, raw and value
    under the bound of their scales."""
    assert len(cols) == len(joint_) == len(raw) == len(value) == len(expected), (what, len(cols), len(expected))
    for k, (v, w, n, S, C) in enumerate(expected):
        assert tuple(cols[k]) == (v, w) and list(joint_[k]) == n, (what, k, cols[k], joint_[k], (v, w, n))
        assert abs(raw[k] - S) <= bound * ref.scale[statistic][(v, w)], (what, "raw", k, (v, w), raw[k], S)
        assert abs(value[k] - C) <= bound * (abs(S) + abs(ref.term(statistic, correction, v, w))), (what, "value", k, (v, w), value[k], C)
        assert not math.isnan(raw[k]) and not math.isnan(value[k])


def check_means(ref, statistic, col_mean, mean_all, what="", bound=BOUND):
    assert len(col_mean) == ref.L
    for c, (got, exp) in enumerate(zip(col_mean, ref.mean[statistic])):
        assert abs(got - exp) <= bound * abs(exp), (what, "mean", c, got, exp)
    assert abs(mean_all - ref.mean_all[statistic]) <= bound * abs(ref.mean_all[statistic]), (what, "mean_all", mean_all)


def canonical(n):
    """The six canonical entries of a joint table in the order of Covariation's TYPES."""
    return [n[CELLS.index(t)] for t in TYPES]
