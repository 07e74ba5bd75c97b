"""CPU tests of CovariationStatistics() / CovariationStatisticsResult (no GPU): the numpy path under the test-only OracleEngine
against the plain-Python reference of tests/covariation_stat_checks.py.  Counters are compared exactly, floats under the bound
derived there."""
import math

import numpy as np
import pytest

from squarna_amd import engine as E
from tests.covariation_checks import random_rows
from tests.covariation_stat_checks import (CELLS, CORRECTIONS, DEFAULTS, EVERY_CELL, STATISTICS, Reference, canonical, check_means,
                                           check_records)
from tests.oracle_engine import OracleEngine

ALI = "examples/ali_input.afa"


def statistics(**kw):
    from squarna_amd import CovariationStatistics
    with E.use_engine(OracleEngine()):
        return CovariationStatistics(**kw)


@pytest.fixture(scope="module")
def folded():
    from squarna_amd import FoldAlignment
    with E.use_engine(OracleEngine()):
        return FoldAlignment(inputfile=ALI)


def check_result(res, ref, expected, mode, statistic="gt", correction="apc"):
    import torch
    P = len(expected)
    assert (res.mode, res.source, res.device.type, len(res)) == (mode, "host", "cpu", P)
    assert (res.statistic, res.correction) == (statistic, correction)
    for key, shape, dtype in (("pair_cols", (P, 2), torch.int32), ("joint", (P, 16), torch.int32), ("raw", (P,), torch.float64),
                              ("value", (P,), torch.float64)):
        t = getattr(res, key)
        assert tuple(t.shape) == shape and t.dtype == dtype, key
    check_records(ref, statistic, correction, res.pair_cols.tolist(), res.joint.tolist(), res.raw.tolist(), res.value.tolist(), expected, mode)
    if correction is None:
        assert res.col_mean is None and res.mean_all is None and torch.equal(res.raw, res.value)
    else:
        assert res.col_mean.dtype == res.mean_all.dtype == torch.float64 and tuple(res.col_mean.shape) == (ref.L,) and res.mean_all.dim() == 0
        check_means(ref, statistic, res.col_mean.tolist(), float(res.mean_all), mode)


@pytest.fixture(scope="module")
def small():
    rows = random_rows(11030, 11, 30)
    return rows, Reference(rows)


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("correction", CORRECTIONS, ids=["none", "apc", "asc"])
def test_every_statistic_and_correction(small, statistic, correction):
    rows, ref = small
    for thr in (DEFAULTS, EVERY_CELL):
        res = statistics(sequences=rows, statistic=statistic, correction=correction, **({} if thr is DEFAULTS else thr))
        check_result(res, ref, ref.select(statistic, correction, **thr), "scan", statistic, correction)
    assert len(res) == 30 * 29 // 2 and res.R == 11 and res.L == 30 and res.sequences == rows
    some = [(5, 20), (0, 1), (5, 20), (3, 29)]
    check_result(statistics(sequences=rows, pairs=some, statistic=statistic, correction=correction), ref,
                 [ref.record(statistic, correction, v, w) for v, w in some], "pairs", statistic, correction)


def test_the_defaults_are_the_g_test_with_apc(small):
    rows, ref = small
    res = statistics(sequences=rows)
    assert (res.statistic, res.correction) == ("gt", "apc")
    check_result(res, ref, ref.select("gt", "apc", **DEFAULTS), "scan")
    thr = ref.gap_threshold("gt", "apc")[0]
    kept = statistics(sequences=rows, min_stat=thr, min_rows=3)
    assert kept.pair_cols.tolist() == [list(r[:2]) for r in ref.select("gt", "apc", minspan=4, min_rows=3, min_stat=thr)] and 0 < len(kept) < len(res)


def test_a_larger_shape(small):
    rows = random_rows(77, 130, 70)
    ref = Reference(rows)
    for s in STATISTICS:
        check_result(statistics(sequences=rows, pairs="scan", statistic=s, names=["r%d" % k for k in range(130)]), ref,
                     ref.select(s, "apc", **DEFAULTS), "scan", s)


def test_every_pairs_form(folded):
    import torch
    from squarna_amd.dbn import DBNToPairs
    seqs = folded.sequences
    ref = Reference(seqs)
    given = lambda pairs: [ref.record("gt", "apc", v, w) for v, w in pairs]
    steps = sorted(set(p for s in (1, 2, 3) for p in folded.pairs(s)))
    assert steps and len(folded.pair_cols)
    res = statistics(alignment=folded)                                      # the default with an alignment: "steps"
    check_result(res, ref, given(steps), "pairs")
    assert res.names == folded.names and res.sequences == seqs
    check_result(statistics(alignment=folded, pairs="steps"), ref, given(steps), "pairs")
    table = [tuple(p) for p in folded.pair_cols.tolist()]
    check_result(statistics(alignment=folded, pairs="table"), ref, given(table), "pairs")       # in the table's order
    check_result(statistics(alignment=folded, pairs="scan"), ref, ref.select("gt", "apc", **DEFAULTS), "scan")
    line = folded.dbn(3)
    check_result(statistics(sequences=seqs, pairs=line), ref, given(DBNToPairs(line)), "pairs")
    some = [(5, 20), (0, 1), (5, 20), (3, folded.L - 1)]                    # as given: unsorted, a repeat, below minspan
    check_result(statistics(sequences=seqs, pairs=some), ref, given(some), "pairs")
    check_result(statistics(sequences=seqs, pairs=torch.tensor(some, dtype=torch.int64)), ref, given(some), "pairs")
    check_result(statistics(sequences=seqs, pairs=[]), ref, [], "pairs")
    filed = statistics(inputfile=ALI)
    assert filed.names == folded.names and filed.sequences == seqs
    check_result(filed, ref, ref.select("gt", "apc", **DEFAULTS), "scan")


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("correction", CORRECTIONS, ids=["none", "apc", "asc"])
def test_a_conserved_alignment_is_exactly_zero(statistic, correction):
    res = statistics(sequences=["GGGAAAUCCC-N"] * 7, statistic=statistic, correction=correction, **EVERY_CELL)
    assert len(res) == 12 * 11 // 2 and set(res.rows.tolist()) == {0, 7}
    assert res.raw.tolist() == [0.0] * len(res) and res.value.tolist() == [0.0] * len(res)
    if correction is not None:
        assert float(res.mean_all) == 0.0 and res.col_mean.tolist() == [0.0] * 12
    assert not any(math.isnan(x) for x in res.to_matrix().flatten().tolist())


def test_an_all_gap_column():
    rows = [r[:3] + "-" + r[4:9] + "." + r[10:] for r in random_rows(3, 9, 14)]
    ref = Reference(rows)
    for s in STATISTICS:
        for c in CORRECTIONS:
            res = statistics(sequences=rows, statistic=s, correction=c, **EVERY_CELL)
            check_result(res, ref, ref.select(s, c, **EVERY_CELL), "scan", s, c)
            at = [(v, w) for v, w in res.pair_cols.tolist() if 3 in (v, w) or 9 in (v, w)]
            assert len(at) == 13 + 12 and all(res.of(v, w)["rows"] == 0 and res.of(v, w)["raw"] == 0.0 for v, w in at)
            assert not torch_isnan(res.raw) and not torch_isnan(res.value)
            if c is not None:
                assert res.col_mean[3] == 0 and res.col_mean[9] == 0 and not torch_isnan(res.col_mean)
    assert len(statistics(sequences=rows, **dict(EVERY_CELL, min_rows=1))) == 12 * 11 // 2       # the gap columns' cells: N == 0


def torch_isnan(t):
    return bool(t.isnan().any())


def test_a_single_column_is_an_empty_result():
    import torch
    for c in CORRECTIONS:
        res = statistics(sequences=["A", "C", "G"], correction=c, **EVERY_CELL)
        assert len(res) == 0 and res.L == 1 and tuple(res.pair_cols.shape) == (0, 2) and tuple(res.joint.shape) == (0, 16)
        assert res.raw.dtype == res.value.dtype == torch.float64 and tuple(res.to_matrix().shape) == (1, 1)
        if c is not None:
            assert res.col_mean.tolist() == [0.0] and float(res.mean_all) == 0.0
    assert len(statistics(sequences=["A", "C", "G"], pairs=[])) == 0


def test_canonical_is_covariations_counts(folded):
    from squarna_amd import Covariation
    rows = random_rows(5, 12, 33)
    res = statistics(sequences=rows, **EVERY_CELL)
    with E.use_engine(OracleEngine()):
        cov = Covariation(sequences=rows, minspan=1, min_rows=0, min_cov=0)
        cov_steps = Covariation(alignment=folded)
    assert res.pair_cols.tolist() == cov.pair_cols.tolist() and res.canonical().tolist() == cov.counts[:, :6].tolist()
    assert res.TYPES == cov.TYPES and res.canonical().dtype == cov.counts.dtype
    steps = statistics(alignment=folded)
    assert steps.pair_cols.tolist() == cov_steps.pair_cols.tolist() and steps.canonical().tolist() == cov_steps.counts[:, :6].tolist()


def test_derived_fields_matrix_of_and_top(small):
    rows, ref = small
    res = statistics(sequences=rows, statistic="mi", correction="asc")
    exp = ref.select("mi", "asc", **DEFAULTS)
    assert res.CELLS == CELLS and res.LETTERS == "ACGU"
    assert res.rows.tolist() == [sum(n) for _, _, n, _, _ in exp]
    na, nb = res.marginals()
    assert na.tolist() == [[sum(n[a * 4:a * 4 + 4]) for a in range(4)] for _, _, n, _, _ in exp]
    assert nb.tolist() == [[sum(n[b::4]) for b in range(4)] for _, _, n, _, _ in exp]
    assert res.canonical().tolist() == [canonical(n) for _, _, n, _, _ in exp]
    for field, of in (("value", lambda r: r[4]), ("raw", lambda r: r[3]), ("rows", lambda r: sum(r[2])), ("GC", lambda r: r[2][CELLS.index("GC")])):
        m = res.to_matrix(field) if field != "value" else res.to_matrix()
        assert tuple(m.shape) == (30, 30) and (m == m.T).all()
        dense = np.zeros((30, 30))
        for r in exp:
            dense[r[0], r[1]] = dense[r[1], r[0]] = of(r)
        assert np.abs(m.numpy() - dense).max() <= 1e-9, field
    assert str(res.to_matrix("raw").dtype) == "torch.float64" and str(res.to_matrix("UA").dtype) == "torch.int64"
    with pytest.raises(ValueError):
        res.to_matrix("nothing")
    v, w, n, S, C = exp[len(exp) // 2]
    rec = res.of(v, w)
    assert rec == res.of(w, v) and [rec[c] for c in CELLS] == n and rec["rows"] == sum(n)
    assert abs(rec["raw"] - S) <= 1e-9 and abs(rec["value"] - C) <= 1e-9
    with pytest.raises(KeyError):
        res.of(0, 1)                                                        # below minspan: no record
    top = res.top(5)
    order = sorted(range(len(exp)), key=lambda k: -res.value[k].item())[:5]
    assert len(top) == 5 and top.pair_cols.tolist() == [res.pair_cols[k].tolist() for k in order]
    assert top.value.tolist() == sorted(res.value.tolist(), reverse=True)[:5] and top.joint.tolist() == [res.joint[k].tolist() for k in order]
    assert len(res.top(10 ** 6)) == len(res) and len(res.top(0)) == 0
    assert len(res.cpu()) == len(res) and res.cpu().value.tolist() == res.value.tolist()
    assert statistics(sequences=rows, correction=None).cpu().col_mean is None


def test_the_call_prints_nothing(capsys, small):
    statistics(sequences=small[0])
    statistics(inputfile=ALI, pairs=[(0, 9)])
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""


def test_error_messages():
    rows = random_rows(9, 4, 12)
    with pytest.raises(ValueError, match="CovariationStatistics: exactly one of inputfile, sequences and alignment"):
        statistics(sequences=rows, inputfile=ALI)
    with pytest.raises(ValueError, match="exactly one of"):
        statistics()
    with pytest.raises(AssertionError, match="not aligned"):
        statistics(sequences=rows + ["ACGU"])
    for bad in ([(3, 12)], [(5, 5)], [(-1, 4)], [(7, 2)]):                  # outside L, v == w, v < 0, v > w
        with pytest.raises(RuntimeError, match="CovariationStatistics: a pair is not 0 <= v < w < 12 columns"):
            statistics(sequences=rows, pairs=bad)
    with pytest.raises(ValueError, match="CovariationStatistics: pairs is 'scan'"):
        statistics(sequences=rows, pairs="everything")
    with pytest.raises(ValueError, match="pairs='steps' needs alignment="):
        statistics(sequences=rows, pairs="steps")
    with pytest.raises(ValueError, match="CovariationStatistics: minspan"):
        statistics(sequences=rows, minspan=-1)
    with pytest.raises(ValueError, match="CovariationStatistics: minspan"):
        statistics(sequences=rows, min_rows=-1)
    with pytest.raises(ValueError, match="1 names for 4 sequences"):
        statistics(sequences=rows, names=["a"])
    with pytest.raises(ValueError, match="statistic is one of mi, gt, chi: 'GTp'"):
        statistics(sequences=rows, statistic="GTp")
    for bad in ("APC", "none", 1):
        with pytest.raises(ValueError, match="correction is 'apc', 'asc' or None"):
            statistics(sequences=rows, correction=bad)
    for bad in ("3", float("nan"), True, [1.0]):
        with pytest.raises(ValueError, match="min_stat is a number or None"):
            statistics(sequences=rows, min_stat=bad)
