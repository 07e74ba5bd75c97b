"""What the tests of the weighted covariation statistics (CovariationStatistics(weights=)) share: the definitions restated in
plain Python, and the float bound.

The reference shares nothing with the header or numpy.  A weight becomes q = round(w * 2**20), a Python int (round() rounds
ties to even); the counters of a cell are a collections.Counter of int sums of q over the rows' two letters; every quotient is
one fractions.Fraction of Python ints rounded once to a float (the argument of a logarithm, the weight n / N of an MI term, a
whole chi-square term), every logarithm is math.log of such a float and every sum math.fsum.  Q is always compared exactly.

The float bound.  It carries over from covariation_stat_checks.py, whose derivation is repeated here for the weighted terms.
The counters are integers and exact, and so are x = Q / 2^20 as doubles: the reference and the code under test start from the
same numbers.  A term of S costs a few ulp.  The quotient under the logarithm is Q_k Q_N / (Q_a Q_b), and the code forms it
from the exact products, rounded once (SqCovarWstat::ratio), as the Fraction here is: with two rounded products in front of
the division, x_k * X_N and x_a * x_b, it would be off by up to two more ulp, which a logarithm near 1 takes whole -- a row of
weight 2048 among rows of weight 2^-20 makes such tables, and MI and the G-test, whose terms cancel to second order there, would
miss this bound by a factor 1.6 in two cells of the shapes of the tests.  Then one fp64 log and one product as in the unweighted code; the two products of a
chi-square term's e are rounded, a few ulp of a term that does not cancel.  S is a sum of at most 16 terms, whatever L.  A
column sum has at most L - 1 addends of one sign (S >= 0 up to its own rounding): added in any order it errs by at most
(L - 1) ulp/2 = (L - 1) * 2^-53 of the sum, on top of the few ulp of every addend; the corrections are three or four more
operations.  So the error of any number is below about (L + 10) * 2^-53 of its scale: 2^-46 at L = 3 tiles + 1 = 97, 2^-42
at the largest shape of the tests, L = 64 tiles + 1 = 2049.  The bound stays BOUND = 2^-40 of the scale for every shape, a
factor 4 above that, and is not tuned.  The scales are those of covariation_stat_checks.py: of `raw` the sum of the absolute
terms of S, of `value` |S| + |the correction term|, of a column mean the mean itself."""
import math
import random
from collections import Counter
from fractions import Fraction

from tests.covariation_stat_checks import BOUND, LETTERS, STATISTICS, Reference, columns  # noqa: F401  (BOUND: for the tests)

ONE = 2 ** 20
#: the weights the tests draw from: nothing, the smallest step, fractions that are not multiples of 2^-20, 1 and the largest
WEIGHTS = (0.0, 2.0 ** -20, 1 / 3, 0.5, 1.0, 1 / 7, 2048.0)


def quantise(weights):
    return [round(w * ONE) for w in weights]


def random_weights(seed, R, pool=WEIGHTS):
    rng = random.Random(seed)
    return [rng.choice(pool) for _ in range(R)]


def joint_w(col_v, col_w, q):
    """[Q[a * 4 + b]] of two columns given as strings of normalised letters, q the rows' quantised weights."""
    seen = Counter()
    for a, b, x in zip(col_v, col_w, q):
        seen[(a, b)] += x
    return [seen[(a, b)] for a in LETTERS for b in LETTERS]


def raw_terms_w(Q, statistic):
    """The terms of S in the table's order (gt: each already doubled), from the integer table Q."""
    N = sum(Q)
    if N == 0:
        return []
    Qa = [sum(Q[a * 4 + b] for b in range(4)) for a in range(4)]
    Qb = [sum(Q[a * 4 + b] for a in range(4)) for b in range(4)]
    terms = []
    for a in range(4):
        for b in range(4):
            x = Q[a * 4 + b]
            if statistic == "chi":
                if Qa[a] * Qb[b] > 0:
                    e = Fraction(Qa[a] * Qb[b], N * ONE)             # (Qa / ONE) * (Qb / ONE) / (N / ONE)
                    terms.append(float((Fraction(x, ONE) - e) ** 2 / e))
            elif x > 0:
                l = math.log(float(Fraction(x * N, Qa[a] * Qb[b])))
                terms.append(float(Fraction(x, N)) * l if statistic == "mi" else 2 * float(Fraction(x, ONE)) * l)
    return terms


class WeightedReference(Reference):
    """covariation_stat_checks.Reference for weighted rows: .n[(v, w)] is the integer table Q, .q the quantised weights; the
    means, term(), value(), record() and gap_threshold() are the parent's, select() compares the weighted N with min_rows."""

    def __init__(self, rows, weights):
        assert len(rows) == len(weights)
        cols = columns(rows)
        L = self.L = len(cols)
        q = self.q = quantise(weights)
        self.n, self.S, self.scale = {}, {s: {} for s in STATISTICS}, {s: {} for s in STATISTICS}
        memo = {}
        for v in range(L):
            for w in range(v + 1, L):
                Q = self.n[(v, w)] = joint_w(cols[v], cols[w], q)
                key = tuple(Q)
                if key not in memo:
                    memo[key] = {}
                    for s in STATISTICS:
                        terms = raw_terms_w(Q, s)
                        memo[key][s] = (math.fsum(terms), math.fsum(abs(t) for t in terms))
                for s in STATISTICS:
                    self.S[s][(v, w)], self.scale[s][(v, w)] = memo[key][s]
        self.mean, self.mean_all = {}, {}
        for s in STATISTICS:
            S = self.S[s]
            self.mean[s] = [math.fsum(S[(min(c, d), max(c, d))] for d in range(L) if d != c) / (L - 1) if L > 1 else 0.0 for c in range(L)]
            self.mean_all[s] = math.fsum(S.values()) / (L * (L - 1) // 2) if L > 1 else 0.0

    def rows_of(self, v, w):
        """The weighted N of a cell, exactly."""
        return Fraction(sum(self.n[(v, w)]), ONE)

    def select(self, statistic, correction, minspan=4, min_rows=1, min_stat=None):
        return [self.record(statistic, correction, v, w) for (v, w) in sorted(self.n)
                if w - v >= minspan and self.rows_of(v, w) >= min_rows
                and (min_stat is None or self.value(statistic, correction, v, w) >= min_stat)]


_REFERENCES = {}


def reference(rows, weights):
    """The WeightedReference of (rows, weights), formed once per test session."""
    key = (tuple(rows), tuple(weights))
    if key not in _REFERENCES:
        _REFERENCES[key] = WeightedReference(rows, weights)
    return _REFERENCES[key]
