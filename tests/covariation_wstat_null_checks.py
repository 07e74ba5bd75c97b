"""What the tests of CovariationStatisticsSignificance(weights=) share: the weighted null restated in plain Python, under the
bracket of tests/covariation_stat_null_checks.py.

The reference is the restatements that exist: shuffled() of tests/covariation_null_checks.py forms sample k of the null as
strings, and WeightedReference of tests/covariation_wstat_checks.py gives every cell of that shuffled alignment its weighted
table, S, column means and C with the weights of the row slots -- row r of the shuffled alignment keeps weights[r].  Nothing
of the numpy fallback or the kernels is used.

The bracket is Bracket of covariation_stat_null_checks.py with these references in the place of the unweighted ones: the same
BOUND = 2^-40 (covariation_wstat_checks.py derives it for the weighted terms), the same scales (|S| + |the correction term|),
the same bisection.  Nothing is retuned."""
import functools

from tests.covariation_null_checks import scope, shuffled
from tests.covariation_stat_null_checks import Bracket, cell_scale, check_bracket, sharp_enough  # noqa: F401  (for the tests)
from tests.covariation_stat_checks import BOUND
from tests.covariation_wstat_checks import WeightedReference


@functools.lru_cache(8)
def weighted_references(rows, weights, samples, seed):
    """(WeightedReference of the rows, [WeightedReference of sample k of their null]) of tuples of rows and weights."""
    return (WeightedReference(list(rows), list(weights)),
            [WeightedReference(shuffled(list(rows), k, seed), list(weights)) for k in range(samples)])


class WeightedBracket(Bracket):
    """Bracket for weighted rows: pooled(), own(), value() and table() are the parent's, on the weighted references."""

    def __init__(self, rows, weights, statistic, correction, minspan, samples, seed, bound=BOUND):
        self.observed, self.nulls = weighted_references(tuple(rows), tuple(weights), samples, seed)
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
