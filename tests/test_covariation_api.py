"""CPU tests of Covariation() / CovariationResult (no GPU): the numpy path under the test-only OracleEngine against the
plain-Python references of tests/covariation_checks.py.  Integer comparisons are exact; score() is compared with the same
formula in numpy float64 at 1e-12 (|score| <= 2 + phi and the formula is four IEEE operations, so the error is below 1e-15:
the margin only absorbs reciprocal-multiply forms)."""
import numpy as np
import pytest

from squarna_amd import engine as E
from tests.covariation_checks import DEFAULTS, EVERY_CELL, check_records, count_cells, naive_cells, random_rows, select
from tests.oracle_engine import OracleEngine

ALI = "examples/ali_input.afa"


def covariation(**kw):
    from squarna_amd import Covariation
    with E.use_engine(OracleEngine()):
        return Covariation(**kw)


@pytest.fixture(scope="module")
def folded():
    from squarna_amd import FoldAlignment
    with E.use_engine(OracleEngine()):
        return FoldAlignment(inputfile=ALI)


def check_result(res, expected, mode):
    import torch
    P = len(expected)
    assert res.mode == mode and res.source == "host" and res.device.type == "cpu" and len(res) == P
    for key, shape, dtype in (("pair_cols", (P, 2), torch.int32), ("counts", (P, 7), torch.int32), ("cov", (P,), torch.int64)):
        t = getattr(res, key)
        assert tuple(t.shape) == shape and t.dtype == dtype, key
    check_records(res.pair_cols.tolist(), res.counts.tolist(), res.cov.tolist(), expected, mode)


@pytest.mark.parametrize("R,L", [(1, 30), (2, 9), (11, 30), (12, 40)])
@pytest.mark.parametrize("thr", [DEFAULTS, EVERY_CELL], ids=["defaults", "every_cell"])
def test_scan_against_the_naive_and_the_count_reference(R, L, thr):
    rows = random_rows(R * 1000 + L, R, L)
    cells = naive_cells(rows)
    assert count_cells(rows) == cells
    res = covariation(sequences=rows, **({} if thr is DEFAULTS else thr))
    check_result(res, select(cells, **thr), "scan")
    assert res.R == R and res.L == L and res.sequences == rows and res.names == [">record%d" % (k + 1) for k in range(R)]
    if thr is EVERY_CELL:
        assert len(res) == L * (L - 1) // 2


def test_scan_at_a_larger_shape_against_the_count_reference():
    rows = random_rows(77, 130, 70)
    check_result(covariation(sequences=rows, pairs="scan", names=["r%d" % k for k in range(130)]), select(count_cells(rows), **DEFAULTS), "scan")


def test_file_input_is_the_sequences_input():
    from squarna_amd import FoldAlignment
    res = covariation(inputfile=ALI)
    with E.use_engine(OracleEngine()):
        ali = FoldAlignment(inputfile=ALI, step3="1")
    assert res.names == ali.names and res.sequences == ali.sequences
    check_result(res, select(count_cells(res.sequences), **DEFAULTS), "scan")


def _given(rows, pairs):
    cells = count_cells(rows)
    return [(v, w) + cells[(v, w)] for v, w in pairs]


def test_every_pairs_form(folded):
    import torch
    seqs = folded.sequences
    steps = sorted(set(p for s in (1, 2, 3) for p in folded.pairs(s)))
    assert steps and len(folded.pair_cols)
    res = covariation(alignment=folded)                                     # the default with an alignment: "steps"
    check_result(res, _given(seqs, steps), "pairs")
    assert res.names == folded.names and res.sequences == seqs
    check_result(covariation(alignment=folded, pairs="steps"), _given(seqs, steps), "pairs")
    table = [tuple(p) for p in folded.pair_cols.tolist()]
    check_result(covariation(alignment=folded, pairs="table"), _given(seqs, table), "pairs")      # in the table's order
    check_result(covariation(alignment=folded, pairs="scan"), select(count_cells(seqs), **DEFAULTS), "scan")
    line = folded.dbn(3)
    from squarna_amd.dbn import DBNToPairs
    check_result(covariation(sequences=seqs, pairs=line), _given(seqs, DBNToPairs(line)), "pairs")
    some = [(5, 20), (0, 1), (5, 20), (3, folded.L - 1)]                    # as given: unsorted, a repeat, below minspan
    check_result(covariation(sequences=seqs, pairs=some), _given(seqs, some), "pairs")
    check_result(covariation(sequences=seqs, pairs=torch.tensor(some, dtype=torch.int64)), _given(seqs, some), "pairs")
    check_result(covariation(sequences=seqs, pairs=[]), [], "pairs")


def test_derived_fields_matrix_and_of():
    rows = random_rows(5, 12, 33)
    cells = naive_cells(rows)
    res = covariation(sequences=rows)
    exp = select(cells, **DEFAULTS)
    assert res.TYPES == ("AU", "UA", "GC", "CG", "GU", "UG")
    assert res.bp_rows.tolist() == [sum(c[:6]) for _, _, c, _ in exp]
    assert res.both_gap.tolist() == [c[6] for _, _, c, _ in exp]
    assert res.incompatible.tolist() == [12 - sum(c) for _, _, c, _ in exp]
    assert res.types.tolist() == [sum(x > 0 for x in c[:6]) for _, _, c, _ in exp]
    assert res.covarying().tolist() == [sum(x > 0 for x in c[:6]) >= 2 for _, _, c, _ in exp]
    assert res.covarying(min_types=3).tolist() == [sum(x > 0 for x in c[:6]) >= 3 for _, _, c, _ in exp]
    assert any(res.covarying().tolist()) and not all(res.covarying(3).tolist())
    for field, of in (("cov", lambda c, cov: cov), ("bp_rows", lambda c, cov: sum(c[:6])), ("GC", lambda c, cov: c[2]),
                      ("incompatible", lambda c, cov: 12 - sum(c))):
        m = res.to_matrix(field)
        assert tuple(m.shape) == (33, 33) and (m == m.T).all()
        dense = np.zeros((33, 33), np.int64)
        for v, w, c, cov in exp:
            dense[v, w] = dense[w, v] = of(c, cov)
        assert np.array_equal(m.numpy(), dense), field
    with pytest.raises(ValueError):
        res.to_matrix("nothing")
    v, w, c, cov = exp[len(exp) // 2]
    rec = res.of(v, w)
    assert rec == res.of(w, v) and rec["cov"] == cov and [rec[t] for t in res.TYPES] == c[:6] and rec["both_gap"] == c[6]
    assert rec["bp_rows"] == sum(c[:6]) and rec["incompatible"] == 12 - sum(c) and rec["types"] == sum(x > 0 for x in c[:6])
    with pytest.raises(KeyError):
        res.of(0, 1)                                                        # below minspan: no record
    assert len(res.cpu()) == len(res) and res.cpu().cov.tolist() == res.cov.tolist()


@pytest.mark.parametrize("R", [1, 2, 11])
@pytest.mark.parametrize("phi", [1.0, 0.25])
def test_score(R, phi):
    res = covariation(sequences=random_rows(40 + R, R, 30), **EVERY_CELL)
    cov, bad = res.cov.numpy().astype(np.float64), res.incompatible.numpy().astype(np.float64)
    first = cov / np.float64(R * (R - 1) // 2) if R > 1 else np.zeros_like(cov)
    exp = first - np.float64(phi) * bad / np.float64(R)
    got = res.score(phi) if phi != 1.0 else res.score()
    assert str(got.dtype) == "torch.float64" and len(got) == len(res) == 30 * 29 // 2
    assert np.abs(got.numpy() - exp).max() <= 1e-12
    assert np.abs(got.numpy()).max() <= 2 + phi and (R > 1 or (got.numpy() <= 0).all())


def test_argument_errors():
    rows = random_rows(9, 4, 12)
    with pytest.raises(ValueError):
        covariation(sequences=rows, inputfile=ALI)                          # two inputs
    with pytest.raises(ValueError):
        covariation()                                                       # none
    with pytest.raises(AssertionError, match="not aligned"):
        covariation(sequences=rows + ["ACGU"])
    for bad in ([(3, 12)], [(5, 5)], [(-1, 4)], [(7, 2)]):                  # outside L, v == w, v < 0, v > w
        with pytest.raises(RuntimeError):
            covariation(sequences=rows, pairs=bad)
    with pytest.raises(ValueError):
        covariation(sequences=rows, pairs="everything")                     # an unknown pairs string
    with pytest.raises(ValueError):
        covariation(sequences=rows, pairs="steps")                          # needs an alignment
    with pytest.raises(ValueError):
        covariation(sequences=rows, minspan=-1)
    with pytest.raises(ValueError):
        covariation(sequences=rows, names=["a"])
