"""CPU tests of CovariationStatistics(weights=) (no GPU): the numpy path under the test-only OracleEngine against the unweighted
call (weights of 1 and integer weights: the same bits) and against the plain-Python reference of
tests/covariation_wstat_checks.py.  The weighted counters are compared exactly, floats under the bound derived there."""
import random
from fractions import Fraction

import numpy as np
import pytest

from squarna_amd import engine as E
from tests.covariation_checks import random_rows
from tests.covariation_stat_checks import CORRECTIONS, DEFAULTS, EVERY_CELL, STATISTICS, check_means, check_records
from tests.covariation_wstat_checks import ONE, WEIGHTS, random_weights, reference
from tests.oracle_engine import OracleEngine


def statistics(**kw):
    from squarna_amd import CovariationStatistics
    with E.use_engine(OracleEngine()):
        return CovariationStatistics(**kw)


def same_bits(weighted, plain, correction):
    """A weighted result against an unweighted one that counts the same: the pairs, the table and every float as bits."""
    import torch
    assert torch.equal(weighted.pair_cols, plain.pair_cols) and len(plain) > 0
    assert weighted.joint.dtype == torch.float64 and torch.equal(weighted.joint, plain.joint.double())
    assert torch.equal(weighted.rows, plain.rows.double())
    assert torch.equal(weighted.raw, plain.raw) and torch.equal(weighted.value, plain.value)
    if correction is None:
        assert weighted.col_mean is None and weighted.mean_all is None
    else:
        assert torch.equal(weighted.col_mean, plain.col_mean) and torch.equal(weighted.mean_all, plain.mean_all)


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("correction", CORRECTIONS, ids=["none", "apc", "asc"])
def test_weights_of_one_give_the_unweighted_bits(statistic, correction):
    rows = random_rows(11030, 11, 30)
    for thr in (DEFAULTS, EVERY_CELL):
        kw = dict(sequences=rows, statistic=statistic, correction=correction, **thr)
        same_bits(statistics(weights=[1.0] * 11, **kw), statistics(**kw), correction)
    some = [(5, 20), (0, 1), (5, 20), (3, 29)]
    kw = dict(sequences=rows, statistic=statistic, correction=correction, pairs=some)
    same_bits(statistics(weights=np.ones(11), **kw), statistics(**kw), correction)


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("correction", CORRECTIONS, ids=["none", "apc", "asc"])
def test_integer_weights_give_the_bits_of_the_repeated_rows(statistic, correction):
    rows = random_rows(13035, 13, 35)
    rng = random.Random(5)
    k = [rng.randrange(4) for _ in rows]
    assert set(k) == {0, 1, 2, 3}
    repeated = [r for r, times in zip(rows, k) for _ in range(times)]
    for thr in (DEFAULTS, EVERY_CELL):
        same_bits(statistics(sequences=rows, weights=k, statistic=statistic, correction=correction, **thr),
                  statistics(sequences=repeated, statistic=statistic, correction=correction, **thr), correction)
    some = [(5, 20), (0, 1), (3, 34)]
    same_bits(statistics(sequences=rows, weights=k, statistic=statistic, correction=correction, pairs=some),
              statistics(sequences=repeated, statistic=statistic, correction=correction, pairs=some), correction)


def check_result(res, ref, weights, expected, mode, statistic, correction):
    import torch
    P = len(expected)
    assert (res.mode, res.source, res.device.type, len(res)) == (mode, "host", "cpu", P)
    for key, shape, dtype in (("pair_cols", (P, 2), torch.int32), ("joint", (P, 16), torch.float64), ("raw", (P,), torch.float64),
                              ("value", (P,), torch.float64), ("rows", (P,), torch.float64), ("weights", (ref_R(ref),), torch.float64)):
        t = getattr(res, key)
        assert tuple(t.shape) == shape and t.dtype == dtype, key
    assert res.weights.tolist() == [float(w) for w in weights]
    Q = (res.joint * ONE).tolist()                                           # (multiples of 2^-20 times 2^20: exact)
    assert all(float(x).is_integer() for row in Q for x in row)
    check_records(ref, statistic, correction, res.pair_cols.tolist(), [[int(x) for x in row] for row in Q], res.raw.tolist(),
                  res.value.tolist(), expected, mode)
    assert res.rows.tolist() == [float(Fraction(sum(r[2]), ONE)) for r in expected]
    if correction is None:
        assert res.col_mean is None and res.mean_all is None and torch.equal(res.raw, res.value)
    else:
        check_means(ref, statistic, res.col_mean.tolist(), float(res.mean_all), mode)


def ref_R(ref):
    return len(ref.q)


@pytest.fixture(scope="module")
def fractional():
    rows = random_rows(66, 65, 33)
    weights = random_weights(66, 65)
    assert set(weights) == set(WEIGHTS)
    return rows, weights, reference(rows, weights)


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("correction", CORRECTIONS, ids=["none", "apc", "asc"])
def test_fractional_weights_against_the_reference(fractional, statistic, correction):
    import torch
    rows, weights, ref = fractional
    for thr in (DEFAULTS, EVERY_CELL):
        res = statistics(sequences=rows, weights=weights, statistic=statistic, correction=correction, **thr)
        check_result(res, ref, weights, ref.select(statistic, correction, **thr), "scan", statistic, correction)
    some = [(5, 20), (0, 1), (5, 20), (3, 32)]
    for given in (weights, np.array(weights), torch.tensor(weights, dtype=torch.float64)):
        res = statistics(sequences=rows, weights=given, statistic=statistic, correction=correction, pairs=some)
        check_result(res, ref, weights, [ref.record(statistic, correction, v, w) for v, w in some], "pairs", statistic, correction)


def test_derived_fields_work_on_weighted_tables(fractional):
    rows, weights, ref = fractional
    res = statistics(sequences=rows, weights=weights, statistic="mi", correction="asc")
    exp = ref.select("mi", "asc", **DEFAULTS)
    na, nb = res.marginals()
    assert na.tolist() == [[float(Fraction(sum(n[a * 4:a * 4 + 4]), ONE)) for a in range(4)] for _, _, n, _, _ in exp]
    assert nb.tolist() == [[float(Fraction(sum(n[b::4]), ONE)) for b in range(4)] for _, _, n, _, _ in exp]
    assert res.canonical().tolist() == [[n[res.CELLS.index(t)] / ONE for t in res.TYPES] for _, _, n, _, _ in exp]
    v, w, n, S, C = exp[len(exp) // 2]
    rec = res.of(v, w)
    assert [rec[c] for c in res.CELLS] == [x / ONE for x in n] and rec == res.of(w, v)
    m = res.to_matrix("GC")
    assert str(m.dtype) == "torch.float64" and (m == m.T).all() and float(m[v, w]) == n[res.CELLS.index("GC")] / ONE
    assert float(res.to_matrix("rows")[v, w]) == sum(n) / ONE and float(res.to_matrix()[w, v]) == rec["value"]
    top = res.top(5)
    assert len(top) == 5 and top.value.tolist() == sorted(res.value.tolist(), reverse=True)[:5] and top.weights is res.weights
    assert res.cpu().weights.tolist() == res.weights.tolist()


def test_error_messages():
    import torch
    rows = random_rows(9, 4, 12)
    for bad in ([1.0] * 3, [1.0] * 5, np.ones((2, 4)), torch.ones(0)):
        with pytest.raises(ValueError, match="CovariationStatistics: weights has . entries for 4 rows"):
            statistics(sequences=rows, weights=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.5, 2048.5):
        for form in (list, np.array, torch.tensor):
            with pytest.raises(ValueError, match="CovariationStatistics: weights are finite numbers from 0 to 2048"):
                statistics(sequences=rows, weights=form([1.0, bad, 1.0, 1.0]))
    with pytest.raises(ValueError, match="CovariationStatistics: weights is a sequence"):
        statistics(sequences=rows, weights=["a", "b", "c", "d"])
    for bad in (-1, -0.5, float("nan"), "2", True):
        with pytest.raises(ValueError, match="CovariationStatistics: with weights min_rows"):
            statistics(sequences=rows, weights=[1.0] * 4, min_rows=bad)
    statistics(sequences=rows, weights=[0.0, 2048.0, 0.0, 2048], pairs=[(0, 5)])      # the two ends are weights


def test_a_float_min_rows_selects_by_the_weighted_rows(fractional):
    rows, weights, ref = fractional
    cells = [(v, w) for (v, w) in sorted(ref.n) if w - v >= 4]
    N = sorted(set(ref.rows_of(v, w) for v, w in cells))
    assert len(N) > 20
    gap, low, high = max((b - a, a, b) for a, b in zip(N, N[1:]))            # the threshold: the middle of the widest gap
    for thr in (float((low + high) / 2), 0.0):
        assert all(abs(ref.rows_of(v, w) - Fraction(thr)) > Fraction(1, ONE) for v, w in cells)     # no N within 2^-20 of it
        kept = ref.select("gt", "apc", min_rows=thr)
        res = statistics(sequences=rows, weights=weights, min_rows=thr)
        assert res.pair_cols.tolist() == [list(r[:2]) for r in kept] and (res.rows >= thr).all()
        assert 0 < len(kept) < len(cells) if thr else len(kept) == len(cells)


def test_without_weights_the_dtypes_are_as_before():
    import torch
    rows = random_rows(11030, 11, 30)
    for kw in (dict(), dict(pairs=[(2, 9)])):
        res = statistics(sequences=rows, **kw)
        assert getattr(res, "weights", None) is None
        assert (res.pair_cols.dtype, res.joint.dtype, res.rows.dtype, res.raw.dtype, res.value.dtype) == (
            torch.int32, torch.int32, torch.int32, torch.float64, torch.float64)
        assert all(t.dtype == torch.int32 for t in res.marginals()) and res.canonical().dtype == torch.int32
        assert res.to_matrix("GC").dtype == torch.int64 and res.to_matrix("rows").dtype == torch.int64
        assert getattr(res.cpu(), "weights", None) is None
