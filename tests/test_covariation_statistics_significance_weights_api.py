"""CPU tests of CovariationStatisticsSignificance(weights=) (no GPU): the numpy path under the test-only OracleEngine against
the unweighted call (weights of 1: the same three tensors, bit for bit), against CovariationStatistics(weights=) for
``.observed``, and under the bracket of tests/covariation_wstat_null_checks.py against the plain-Python restatement."""
import numpy as np
import pytest

from squarna_amd import engine as E
from squarna_amd.covariation_significance import scope_cells
from tests.covariation_checks import random_rows
from tests.covariation_null_checks import MASK
from tests.covariation_stat_checks import CORRECTIONS, STATISTICS
from tests.covariation_wstat_checks import random_weights
from tests.covariation_wstat_null_checks import WeightedBracket, check_bracket
from tests.oracle_engine import OracleEngine

NULL = ("null_ge", "own_ge", "null_max")


def significance(**kw):
    from squarna_amd import CovariationStatisticsSignificance
    with E.use_engine(OracleEngine()):
        return CovariationStatisticsSignificance(**kw)


def statistics(**kw):
    from squarna_amd import CovariationStatistics
    with E.use_engine(OracleEngine()):
        return CovariationStatistics(**kw)


def same_observed(a, b):
    assert (a.names, a.sequences, a.R, a.L, a.mode, a.source, a.statistic, a.correction) == \
        (b.names, b.sequences, b.R, b.L, b.mode, b.source, b.statistic, b.correction)
    for key in ("pair_cols", "joint", "raw", "value", "col_mean", "mean_all", "weights"):
        x, y = getattr(a, key), getattr(b, key)
        assert (x is None) == (y is None), key
        assert x is None or (x.dtype == y.dtype and x.shape == y.shape and x.tolist() == y.tolist()), key      # equal bits: no NaN


def same_null(a, b):
    import torch
    assert (a.samples, a.seed, a.null_cells, a.source) == (b.samples, b.seed, b.null_cells, b.source)
    for key in NULL:
        x, y = getattr(a, key), getattr(b, key)
        assert x.dtype == y.dtype and torch.equal(x, y), key


def against_the_bracket(res, rows, weights, minspan, what=""):
    pairs = [tuple(p) for p in res.observed.pair_cols.tolist()]
    bracket = WeightedBracket(rows, weights, res.observed.statistic, res.observed.correction, minspan, res.samples, res.seed)
    check_bracket(bracket, pairs, res.null_ge.tolist(), res.own_ge.tolist(), res.null_max.tolist(), what)
    assert res.null_cells == res.samples * len(bracket.cells) == res.samples * scope_cells(len(rows[0]), minspan)


def test_the_keyword_and_observed_is_the_weighted_statistics():
    import torch
    rows, weights = random_rows(41, 30, 33, "ACGU-", helices=2), random_weights(41, 30)
    every = significance(sequences=rows, weights=weights, samples=3, seed=5, min_rows=0)
    N = sorted(every.observed.rows.tolist())
    floor = N[len(N) // 2] - 2.0 ** -21                                     # a float between two multiples of 2^-20
    assert N[0] < floor < N[-1] and not float(floor).is_integer()
    res = significance(sequences=rows, weights=weights, samples=3, seed=5, min_rows=floor)
    same_observed(res.observed, statistics(sequences=rows, weights=weights, min_rows=floor))
    P = len(res.observed)
    assert res.source == "host" and res.device.type == "cpu" and len(res) == P > 100 and res.samples == 3
    for key, shape, dtype in (("null_ge", (P,), torch.int64), ("own_ge", (P,), torch.int32), ("null_max", (3,), torch.float64),
                              ("weights", (30,), torch.float64)):
        assert tuple(getattr(res, key).shape) == shape and getattr(res, key).dtype == dtype, key
    assert res.weights is res.observed.weights and res.weights.tolist() == weights and res.cpu().weights.tolist() == weights
    assert res.observed.joint.dtype == torch.float64
    # a float min_rows drops observed pairs of the weighted N and leaves the null what it was
    assert len(res) < len(every) and res.null_max.tolist() == every.null_max.tolist() and res.null_cells == every.null_cells
    keep = [k for k, n in enumerate(every.observed.rows.tolist()) if n >= floor]
    assert res.null_ge.tolist() == every.null_ge[keep].tolist() and res.own_ge.tolist() == every.own_ge[keep].tolist()
    v, w = res.observed.pair_cols[P // 2].tolist()
    assert res.of(v, w)["null_ge"] == int(res.null_ge[P // 2]) and res.of(v, w)["value"] == float(res.observed.value[P // 2])
    assert res.evalue().tolist() == (res.null_ge.numpy() / np.float64(3)).tolist() and res.max_ge().dtype == torch.int64
    # the last keyword: every positional call of before means what it meant
    import inspect
    from squarna_amd import CovariationStatisticsSignificance
    assert list(inspect.signature(CovariationStatisticsSignificance).parameters)[-2:] == ["ignorewarn", "weights"]


def test_weights_as_a_list_an_array_and_a_tensor():
    import torch
    rows, weights = random_rows(7, 12, 20, "ACGU-"), random_weights(7, 12)
    first = significance(sequences=rows, weights=weights, samples=2, seed=1)
    for given in (tuple(weights), np.array(weights), torch.tensor(weights, dtype=torch.float64)):
        other = significance(sequences=rows, weights=given, samples=2, seed=1)
        same_observed(first.observed, other.observed)
        same_null(first, other)
    ints = significance(sequences=rows, weights=[k % 3 for k in range(12)], samples=2, seed=1)     # Python ints
    assert ints.weights.tolist() == [float(k % 3) for k in range(12)]


def test_the_value_errors_are_those_of_the_weighted_statistics():
    rows = random_rows(9, 4, 12, "ACGU-")
    for bad, message in (([1.0] * 3, "weights has 3 entries for 4 rows"), ([1.0] * 5, "weights has 5 entries for 4 rows"),
                         ([1.0, float("nan"), 1.0, 1.0], "finite numbers from 0 to 2048"), ([1.0, float("inf"), 1.0, 1.0], "finite numbers"),
                         ([1.0, -1e-9, 1.0, 1.0], "finite numbers from 0 to 2048"), ([1.0, 2048.5, 1.0, 1.0], "finite numbers from 0 to 2048"),
                         ("abcd", "weights is a sequence")):
        with pytest.raises(ValueError, match=message) as ours:
            significance(sequences=rows, weights=bad, samples=2)
        with pytest.raises(ValueError) as theirs:
            statistics(sequences=rows, weights=bad)
        assert str(ours.value) == str(theirs.value)
    for bad in (-1, "2", True):
        with pytest.raises(ValueError, match="min_rows"):
            significance(sequences=rows, weights=[1.0] * 4, min_rows=bad, samples=2)
    with pytest.raises(ValueError, match="samples"):
        significance(sequences=rows, weights=[1.0] * 4, samples=0)
    with pytest.raises(ValueError, match="65,535"):
        significance(sequences=["A"] * 65536, weights=[1.0] * 65536, samples=1)
    assert significance(sequences=rows, weights=[2048.0, 0.0, 0, 2.0 ** -20], samples=1).samples == 1


def test_without_weights_nothing_changes():
    """weights=None, given or not, is the call of before: the observed result has no weights and an integer table, and the null
    is the unweighted one (tests/test_covariation_statistics_significance_api.py pins it against its reference)."""
    import torch
    rows = random_rows(31, 25, 25, "ACGU-")
    for kw in (dict(), dict(pairs=[(5, 20), (0, 1), (5, 20)]), dict(statistic="mi", correction=None, minspan=1)):
        a, b = significance(sequences=rows, samples=3, seed=3, **kw), significance(sequences=rows, samples=3, seed=3, weights=None, **kw)
        same_observed(a.observed, b.observed)
        same_null(a, b)
        assert a.weights is None and b.weights is None and a.observed.joint.dtype == torch.int32


@pytest.mark.parametrize("statistic", STATISTICS)
def test_weights_of_one_give_the_unweighted_null_bit_for_bit(statistic):
    rows = random_rows(11030, 11, 30)
    for correction in CORRECTIONS:
        for kw in (dict(), dict(minspan=1, min_rows=0), dict(pairs=[(5, 20), (0, 1), (5, 20), (3, 29)])):
            kw = dict(sequences=rows, statistic=statistic, correction=correction, samples=3, seed=MASK, **kw)
            weighted, plain = significance(weights=[1.0] * 11, **kw), significance(**kw)
            assert len(plain) > 0 and weighted.observed.value.tolist() == plain.observed.value.tolist()
            same_null(weighted, plain)


@pytest.mark.parametrize("statistic", STATISTICS)
def test_the_fallback_under_the_bracket_of_the_restatement(statistic):
    rows, weights = random_rows(41, 30, 33, "ACGU-", helices=2), random_weights(41, 30)
    for correction in CORRECTIONS:
        for minspan, min_rows, samples, seed in ((4, 1, 3, 0), (1, 0, 2, MASK)):
            res = significance(sequences=rows, weights=weights, statistic=statistic, correction=correction, minspan=minspan,
                               min_rows=min_rows, samples=samples, seed=seed)
            same_observed(res.observed, statistics(sequences=rows, weights=weights, statistic=statistic, correction=correction,
                                                   minspan=minspan, min_rows=min_rows))
            against_the_bracket(res, rows, weights, minspan, (statistic, correction, minspan))
    some = [(5, 20), (0, 1), (5, 20), (3, 24), (2, 3)]                      # as given: unsorted, a repeat, below minspan
    res = significance(sequences=rows, weights=weights, statistic=statistic, pairs=some, samples=4, seed=3, min_rows=50, min_stat=1e9)
    assert [tuple(p) for p in res.observed.pair_cols.tolist()] == some and res.null_ge[0] == res.null_ge[2]
    against_the_bracket(res, rows, weights, 4, (statistic, "pairs"))


def test_a_row_of_weight_zero_is_shuffled_and_counts_nothing():
    """Rows of weight 0 take part in the shuffle: the null differs from that of the alignment without them (whose rows are
    permuted among fewer slots), and stays under the bracket of the restatement, whose shuffle moves their letters too."""
    rows = random_rows(17, 16, 24, "ACGU-", helices=1)
    weights = [0.0 if r % 4 == 0 else 1.0 for r in range(16)]
    res = significance(sequences=rows, weights=weights, samples=3, seed=2, min_rows=0)
    against_the_bracket(res, rows, weights, 4)
    kept = significance(sequences=[r for r, x in zip(rows, weights) if x], samples=3, seed=2, min_rows=0)
    assert res.observed.value.tolist() == kept.observed.value.tolist()     # observed: a row of weight 0 counts nothing
    assert res.null_max.tolist() != kept.null_max.tolist()
