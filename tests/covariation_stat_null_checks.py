"""What the tests of CovariationStatisticsSignificance share: the null restated in plain Python and the bracket.

The reference is the two restatements that exist: shuffled() of tests/covariation_null_checks.py forms sample k of the null as
strings (Python ints, `sorted`), and Reference of tests/covariation_stat_checks.py gives every cell of that shuffled alignment
its S, its column means and its C (Counter, math.log, math.fsum).  Nothing of the numpy fallback or the kernels is used.

The bracket.  The counts compare doubles, and the reference's doubles differ from the code's by the float bound of
tests/covariation_stat_checks.py: BOUND = 2^-40 of the scale of a value, the scale of C being |S| + |the correction term|
(derived there; not retuned here).  A comparison `C_null >= obs` can therefore come out either way only when the two lie
within band = BOUND * (the scale of obs + the scale of the null cell) of one another.  So for every observed pair
    lo = #{C_ref >= obs + band} <= the count <= hi = #{C_ref >= obs - band},
for the pooled count over all in-scope cells of all samples and for the pair's own cell over the samples.  Both sides are
found by bisection in two sorted lists: C_ref >= obs + BOUND * (s_obs + s_cell) is C_ref - BOUND * s_cell >= obs + BOUND *
s_obs (the products and sums round at 2^-53 of numbers 2^-40 of the scales: far inside the factor 4 that BOUND leaves)."""
import bisect
import functools

from tests.covariation_null_checks import scope, shuffled
from tests.covariation_stat_checks import BOUND, Reference


@functools.lru_cache(8)
def references(rows, samples, seed):
    """(Reference of the rows, [Reference of sample k of their null]) of a tuple of rows."""
    return Reference(list(rows)), [Reference(shuffled(list(rows), k, seed)) for k in range(samples)]


def cell_scale(ref, statistic, correction, v, w):
    """The scale of C of a cell: |S| + |the correction term|."""
    return abs(ref.S[statistic][(v, w)]) + abs(ref.term(statistic, correction, v, w))


class Bracket:
    """The reference's null of `rows` for one statistic and correction: for observed pairs (v, w) with the reference's own
    observed values, lo and hi of the pooled count and of the own-cell count, and the samples' maxima with their bands."""

    def __init__(self, rows, statistic, correction, minspan, samples, seed, bound=BOUND):
        self.observed, self.nulls = references(tuple(rows), samples, seed)
        self.statistic, self.correction, self.bound, self.samples = statistic, correction, bound, samples
        self.cells = scope(len(rows[0]), minspan)
        low, high, self.max_low, self.max_high = [], [], [], []
        for ref in self.nulls:
            mine = [(ref.value(statistic, correction, v, w), bound * cell_scale(ref, statistic, correction, v, w)) for v, w in self.cells]
            low += [c - b for c, b in mine]
            high += [c + b for c, b in mine]
            self.max_low.append(max((c - b for c, b in mine), default=float("-inf")))
            self.max_high.append(max((c + b for c, b in mine), default=float("-inf")))
        self.low, self.high = sorted(low), sorted(high)

    def value(self, v, w):
        """(the reference's observed C of the pair, its band)."""
        return (self.observed.value(self.statistic, self.correction, v, w),
                self.bound * cell_scale(self.observed, self.statistic, self.correction, v, w))

    def pooled(self, v, w):
        """(lo, hi) of null_ge of the pair."""
        obs, band = self.value(v, w)
        return len(self.low) - bisect.bisect_left(self.low, obs + band), len(self.high) - bisect.bisect_left(self.high, obs - band)

    def own(self, v, w):
        """(lo, hi) of own_ge of the pair."""
        obs, band = self.value(v, w)
        lo = hi = 0
        for ref in self.nulls:
            c, b = ref.value(self.statistic, self.correction, v, w), self.bound * cell_scale(ref, self.statistic, self.correction, v, w)
            lo += c - b >= obs + band
            hi += c + b >= obs - band
        return lo, hi

    def table(self, pairs):
        """([(lo, hi)] of null_ge, [(lo, hi)] of own_ge) of the pairs."""
        return [self.pooled(v, w) for v, w in pairs], [self.own(v, w) for v, w in pairs]


def sharp_enough(pooled):
    """The condition under which the bracket says something, on the reference alone: the uncertain share of the pooled counts
    is at most 1 % of them, and at least 90 % of the pairs have lo == hi."""
    return (sum(hi - lo for lo, hi in pooled) * 100 <= sum(hi for lo, hi in pooled)
            and sum(lo == hi for lo, hi in pooled) * 10 >= 9 * len(pooled))


def check_bracket(bracket, pairs, null_ge, own_ge, null_max, what=""):
    """Host lists of a result against the bracket of its pairs."""
    pooled, own = bracket.table(pairs)
    assert len(null_ge) == len(own_ge) == len(pairs) and len(null_max) == bracket.samples, what
    for k, ((lo, hi), (olo, ohi)) in enumerate(zip(pooled, own)):
        assert lo <= null_ge[k] <= hi, (what, "null_ge", k, pairs[k], lo, null_ge[k], hi)
        assert olo <= own_ge[k] <= ohi, (what, "own_ge", k, pairs[k], olo, own_ge[k], ohi)
    for k, got in enumerate(null_max):
        assert bracket.max_low[k] <= got <= bracket.max_high[k], (what, "null_max", k, bracket.max_low[k], got, bracket.max_high[k])
