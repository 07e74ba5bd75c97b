"""CPU tests of CovariationStatisticsSignificance() / StatisticsSignificanceResult (no GPU): the numpy path under the test-only
OracleEngine against the plain-Python restatement and bracket of tests/covariation_stat_null_checks.py.  Counts are compared
under the bracket (the docstring there says why a count of float comparisons has one); evalue(), pvalue() and pvalue_max() are
one IEEE division of two integers below 2^53 each and are compared with the same division in numpy: equal floats."""
import math

import numpy as np
import pytest

from squarna_amd import engine as E
from squarna_amd.covariation_significance import scope_cells
from tests.covariation_checks import random_rows
from tests.covariation_null_checks import MASK, PLANTED, planted_rows
from tests.covariation_stat_checks import CORRECTIONS, STATISTICS
from tests.covariation_stat_null_checks import Bracket, check_bracket
from tests.oracle_engine import OracleEngine

ALI = "examples/ali_input.afa"


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
    for key in ("pair_cols", "joint", "raw", "value", "col_mean", "mean_all"):
        x, y = getattr(a, key), getattr(b, key)
        assert (x is None) == (y is None), key
        assert x is None or (x.dtype == y.dtype and x.shape == y.shape and x.tolist() == y.tolist()), key      # equal bits: no NaN


def check_shapes(res, samples):
    import torch
    P = len(res.observed)
    assert res.source == "host" and res.device.type == "cpu" and len(res) == P and res.samples == samples
    for key, shape, dtype in (("null_ge", (P,), torch.int64), ("own_ge", (P,), torch.int32), ("null_max", (samples,), torch.float64)):
        assert tuple(getattr(res, key).shape) == shape and getattr(res, key).dtype == dtype, key
    assert not torch.isnan(res.null_max).any() and (res.own_ge <= samples).all() and (res.null_ge <= res.null_cells).all()


def against_the_bracket(res, rows, minspan, what=""):
    pairs = [tuple(p) for p in res.observed.pair_cols.tolist()]
    bracket = Bracket(rows, res.observed.statistic, res.observed.correction, minspan, res.samples, res.seed)
    check_bracket(bracket, pairs, res.null_ge.tolist(), res.own_ge.tolist(), res.null_max.tolist(), what)
    assert res.null_cells == res.samples * len(bracket.cells) == res.samples * scope_cells(len(rows[0]), minspan)


@pytest.mark.parametrize("statistic", STATISTICS)
def test_scan_under_the_bracket_of_the_restatement(statistic):
    rows = random_rows(41, 30, 33, "ACGU-", helices=2)
    for correction in CORRECTIONS:
        for minspan, min_rows, samples, seed in ((4, 1, 3, 0), (1, 0, 2, MASK)):
            res = significance(sequences=rows, statistic=statistic, correction=correction, minspan=minspan, min_rows=min_rows,
                               samples=samples, seed=seed)
            check_shapes(res, samples)
            same_observed(res.observed, statistics(sequences=rows, statistic=statistic, correction=correction, minspan=minspan,
                                                   min_rows=min_rows))
            against_the_bracket(res, rows, minspan, (statistic, correction, minspan))


def test_given_pairs_and_thresholds_filter_the_observed_only():
    rows = random_rows(31, 25, 25, "ACGU-")
    some = [(5, 20), (0, 1), (5, 20), (3, 24), (2, 3)]                      # as given: unsorted, a repeat, below minspan
    res = significance(sequences=rows, pairs=some, samples=6, seed=3, min_rows=50, min_stat=1e9)       # thresholds: not for given pairs
    check_shapes(res, 6)
    same_observed(res.observed, statistics(sequences=rows, pairs=some))
    assert res.observed.mode == "pairs" and [tuple(p) for p in res.observed.pair_cols.tolist()] == some
    against_the_bracket(res, rows, 4)
    assert res.null_ge[0] == res.null_ge[2] and res.own_ge[0] == res.own_ge[2]
    empty = significance(sequences=rows, pairs=[], samples=2, seed=3)
    check_shapes(empty, 2)
    assert len(empty) == 0 and empty.evalue().numel() == 0 and empty.null_max.tolist() == res.null_max.tolist()[:2]
    # min_stat and min_rows drop observed pairs and leave the null what it was
    scan, high = (significance(sequences=rows, samples=3, seed=3, min_stat=m) for m in (None, 0.5))
    assert 0 < len(high) < len(scan) and high.null_max.tolist() == scan.null_max.tolist() and high.null_cells == scan.null_cells
    keep = [k for k, x in enumerate(scan.observed.value.tolist()) if x >= 0.5]
    assert high.null_ge.tolist() == scan.null_ge[keep].tolist() and high.own_ge.tolist() == scan.own_ge[keep].tolist()


def test_alignment_and_file_inputs():
    from squarna_amd import FoldAlignment
    with E.use_engine(OracleEngine()):
        folded = FoldAlignment(inputfile=ALI)
    res = significance(alignment=folded, samples=2, seed=11)                # the default with an alignment: "steps"
    same_observed(res.observed, statistics(alignment=folded))
    assert res.observed.mode == "pairs" and len(res) and res.source == "host"
    scan = significance(inputfile=ALI, samples=2, seed=11, min_rows=20, min_stat=5.0)
    same_observed(scan.observed, statistics(inputfile=ALI, min_rows=20, min_stat=5.0))
    assert scan.null_max.tolist() == res.null_max.tolist()                  # the null is the alignment's, whatever the pairs


def test_seeds_repeat_and_differ():
    rows = random_rows(77, 20, 30, "ACGU-")
    a, b, c = (significance(sequences=rows, samples=8, seed=s) for s in (5, 5, 6))
    for key in ("null_ge", "own_ge", "null_max"):
        assert getattr(a, key).tolist() == getattr(b, key).tolist(), key
    same_observed(a.observed, c.observed)
    assert a.null_max.tolist() != c.null_max.tolist() and a.null_ge.tolist() != c.null_ge.tolist()


def test_null_ge_falls_with_value_and_the_helpers():
    import torch
    rows = random_rows(5, 20, 33, "ACGU-")
    K = 9
    res = significance(sequences=rows, samples=K, seed=1)
    value, ge = res.observed.value.tolist(), res.null_ge.tolist()
    by_value = sorted(zip(value, ge))
    assert all(g0 >= g1 for (_, g0), (_, g1) in zip(by_value, by_value[1:])) and len(set(ge)) > 3
    assert all(g0 == g1 for (c0, g0), (c1, g1) in zip(by_value, by_value[1:]) if c0 == c1)
    null_ge, own_ge, null_max = res.null_ge.numpy(), res.own_ge.numpy(), res.null_max.numpy()
    max_ge = (null_max[None, :] >= np.array(value)[:, None]).sum(1)
    for got, exp in ((res.evalue(), null_ge.astype(np.float64) / np.float64(K)), (res.pvalue(), (1 + own_ge).astype(np.float64) / np.float64(K + 1)),
                     (res.pvalue_max(), (1 + max_ge).astype(np.float64) / np.float64(K + 1))):
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), exp)
    assert res.max_ge().tolist() == max_ge.tolist() and 0 < max_ge.max() and max_ge.min() < K
    assert res.significant().tolist() == (null_ge / K <= 0.05).tolist() and res.significant(evalue=2.0).tolist() == (null_ge / K <= 2.0).tolist()
    k = len(res) // 2
    v, w = res.observed.pair_cols[k].tolist()
    rec = res.of(w, v)
    assert rec["value"] == value[k] and rec["null_ge"] == ge[k] and rec["own_ge"] == int(own_ge[k]) and rec["evalue"] == ge[k] / K
    assert rec["pvalue"] == (1 + int(own_ge[k])) / (K + 1) and rec["pvalue_max"] == (1 + int(max_ge[k])) / (K + 1)
    assert rec["rows"] == sum(res.observed.joint[k].tolist()) and rec["raw"] == float(res.observed.raw[k])
    with pytest.raises(KeyError):
        res.of(0, 1)
    for field, exp in (("null_ge", null_ge), ("own_ge", own_ge), ("evalue", res.evalue().numpy()), ("pvalue", res.pvalue().numpy()),
                       ("pvalue_max", res.pvalue_max().numpy()), ("value", np.array(value)), ("rows", res.observed.rows.numpy())):
        m = res.to_matrix(field)
        dense = np.zeros((33, 33), exp.dtype if exp.dtype.kind == "f" else np.int64)
        for (a, b), x in zip(res.observed.pair_cols.tolist(), exp.tolist()):
            dense[a, b] = dense[b, a] = x
        assert tuple(m.shape) == (33, 33) and np.array_equal(m.numpy(), dense), field
    assert torch.equal(res.to_matrix(), res.to_matrix("evalue")) and torch.equal(res.to_matrix("GC"), res.observed.to_matrix("GC"))
    with pytest.raises(ValueError):
        res.to_matrix("nothing")
    host = res.cpu()
    assert host.null_ge.tolist() == ge and host.observed.value.tolist() == value and host.null_cells == res.null_cells and len(host) == len(res)


def test_no_cell_in_scope():
    rows = random_rows(3, 6, 10, "ACGU-")
    res = significance(sequences=rows, pairs=[(1, 7)], minspan=10, samples=4)
    assert res.null_cells == 0 and res.null_max.tolist() == [-math.inf] * 4 and res.null_ge.tolist() == [0]
    assert res.max_ge().tolist() == [0] and res.pvalue_max().tolist() == [1 / 5]
    one = significance(sequences=["ACGU"[k % 4] for k in range(9)], pairs=[], samples=2)     # one column: no pair of columns at all
    assert one.null_cells == 0 and one.null_max.tolist() == [-math.inf] * 2


def test_the_planted_helices_stand_out():
    """40 rows x 60 columns, two planted helices of five pairs, 50 samples, GTp: no null cell of any sample reaches a planted
    pair's value, and fewer than 5 % of the other pairs of the scan are significant at the default E-value."""
    rows, planted = planted_rows()
    res = significance(sequences=rows, statistic="gt", correction="apc", samples=PLANTED["samples"], seed=PLANTED["seed"])
    pairs = [tuple(p) for p in res.observed.pair_cols.tolist()]
    at = [pairs.index(p) for p in planted]
    evalue, significant = res.evalue().tolist(), res.significant().tolist()
    assert all(evalue[k] == 0 for k in at) and all(significant[k] for k in at) and all(res.own_ge[k] == 0 for k in at)
    others = [k for k in range(len(pairs)) if k not in at]
    assert len(others) > 1000 and sum(significant[k] for k in others) * 20 < len(others)
    assert res.null_cells == PLANTED["samples"] * scope_cells(PLANTED["L"], 4)


def test_argument_errors():
    rows = random_rows(9, 4, 12, "ACGU-")
    for bad in (0, -3, 2.0, "7", None, True):
        with pytest.raises(ValueError, match="samples"):
            significance(sequences=rows, samples=bad)
    for bad in (-1, MASK + 1, 0.5, "1", None, False):
        with pytest.raises(ValueError, match="seed"):
            significance(sequences=rows, seed=bad)
    assert significance(sequences=rows, samples=np.int64(2), seed=MASK).samples == 2
    for kw, message in ((dict(statistic="mutual"), "statistic is one of mi, gt, chi"), (dict(correction="APC"), "correction is 'apc', 'asc' or None"),
                        (dict(min_stat="1"), "min_stat is a number or None"), (dict(min_stat=float("nan")), "min_stat")):
        with pytest.raises(ValueError, match=message) as ours:
            significance(sequences=rows, **kw)
        with pytest.raises(ValueError) as theirs:
            statistics(sequences=rows, **kw)
        assert str(ours.value) == str(theirs.value)                         # the same errors as CovariationStatistics
    with pytest.raises(ValueError):
        significance(sequences=rows, inputfile=ALI)                         # two inputs
    with pytest.raises(ValueError):
        significance()                                                      # none
    with pytest.raises(AssertionError, match="not aligned"):
        significance(sequences=rows + ["ACGU"])
    with pytest.raises(RuntimeError, match="a pair is not"):
        significance(sequences=rows, pairs=[(3, 12)])
    for kw in (dict(pairs="everything"), dict(pairs="steps"), dict(minspan=-1), dict(names=["a"])):
        with pytest.raises(ValueError):
            significance(sequences=rows, **kw)
    with pytest.raises(ValueError, match="65,535"):
        significance(sequences=["A"] * 65536, samples=1)
