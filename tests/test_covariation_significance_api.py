"""CPU tests of CovariationSignificance() / SignificanceResult (no GPU): the numpy path under the test-only OracleEngine against
the plain-Python restatement of tests/covariation_null_checks.py.  Integer comparisons are exact; evalue(), pvalue() and
pvalue_max() are one IEEE division of two integers below 2^53 each and are compared with the same division in numpy: equal
floats."""
import collections

import numpy as np
import pytest

from squarna_amd import engine as E
from squarna_amd.covariation_significance import scope_cells
from tests.covariation_checks import DEFAULTS, EVERY_CELL, count_cells, normalise, random_rows, select
from tests.covariation_null_checks import MASK, PLANTED, check_significance, null_stats, planted_rows, planted_stats, scope, shuffled
from tests.oracle_engine import OracleEngine

ALI = "examples/ali_input.afa"


def significance(**kw):
    from squarna_amd import CovariationSignificance
    with E.use_engine(OracleEngine()):
        return CovariationSignificance(**kw)


def covariation(**kw):
    from squarna_amd import Covariation
    with E.use_engine(OracleEngine()):
        return Covariation(**kw)


def same_observed(a, b):
    assert (a.names, a.sequences, a.R, a.L, a.mode, a.source) == (b.names, b.sequences, b.R, b.L, b.mode, b.source)
    for key in ("pair_cols", "counts", "cov"):
        assert getattr(a, key).dtype == getattr(b, key).dtype and getattr(a, key).tolist() == getattr(b, key).tolist(), key


def check_shapes(res, samples):
    import torch
    P = len(res.observed)
    assert res.source == "host" and res.device.type == "cpu" and len(res) == P and res.samples == samples
    for key, shape, dtype in (("null_ge", (P,), torch.int64), ("own_ge", (P,), torch.int32), ("null_max", (samples,), torch.int64)):
        assert tuple(getattr(res, key).shape) == shape and getattr(res, key).dtype == dtype, key


@pytest.mark.parametrize("R,L", [(1, 12), (2, 9), (11, 30), (65, 20)])
def test_scan_against_the_restatement(R, L):
    rows = random_rows(R * 1000 + L, R, L)
    for thr, samples, seed in ((DEFAULTS, 5, 0), (EVERY_CELL, 3, MASK)):
        res = significance(sequences=rows, samples=samples, seed=seed, **thr)
        check_shapes(res, samples)
        same_observed(res.observed, covariation(sequences=rows, **thr))
        assert [tuple(p) for p in res.observed.pair_cols.tolist()] == [(v, w) for v, w, _, _ in select(count_cells(rows), **thr)]
        check_significance(res, rows, thr["minspan"], samples, seed)
        assert res.null_cells == samples * len(scope(L, thr["minspan"])) == samples * scope_cells(L, thr["minspan"])
        assert (res.own_ge <= samples).all() and (res.null_ge <= res.null_cells).all()


def test_given_pairs_against_the_restatement():
    rows = random_rows(31, 9, 25)
    some = [(5, 20), (0, 1), (5, 20), (3, 24), (2, 3)]                      # as given: unsorted, a repeat, below minspan
    res = significance(sequences=rows, pairs=some, samples=6, seed=3, min_rows=5, min_cov=10 ** 6)       # thresholds: not for given pairs
    check_shapes(res, 6)
    same_observed(res.observed, covariation(sequences=rows, pairs=some))
    assert res.observed.mode == "pairs" and [tuple(p) for p in res.observed.pair_cols.tolist()] == some
    check_significance(res, rows, 4, 6, 3)
    assert res.null_ge[0] == res.null_ge[2] and res.own_ge[0] == res.own_ge[2]
    empty = significance(sequences=rows, pairs=[], samples=2)
    check_shapes(empty, 2)
    assert len(empty) == 0 and empty.null_max.tolist() == null_stats(rows, [], [], 4, 2, 0)[2] and empty.evalue().numel() == 0


def test_alignment_and_file_inputs():
    from squarna_amd import FoldAlignment
    with E.use_engine(OracleEngine()):
        folded = FoldAlignment(inputfile=ALI)
    res = significance(alignment=folded, samples=3, seed=11)                # the default with an alignment: "steps"
    same_observed(res.observed, covariation(alignment=folded))
    check_significance(res, folded.sequences, 4, 3, 11)
    scan = significance(inputfile=ALI, samples=2, min_rows=20)
    same_observed(scan.observed, covariation(inputfile=ALI, min_rows=20))
    check_significance(scan, folded.sequences, 4, 2, 0)


def test_every_shuffled_column_keeps_its_class_counts():
    from squarna_amd.covariation import _classes
    from squarna_amd.covariation_significance import _shuffled_classes
    rows = random_rows(8, 70, 33)
    byte_rows = np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(70, 33)
    cls = _classes(byte_rows)
    for k, seed in ((0, 0), (4, MASK)):
        got = _shuffled_classes(cls, k, seed)
        assert got.shape == cls.shape and not np.array_equal(got, cls)
        assert all(collections.Counter(got[:, c].tolist()) == collections.Counter(cls[:, c].tolist()) for c in range(33))
        # the numpy shuffle is the restatement's: the same classes row by row
        again = _classes(np.frombuffer("".join(shuffled(rows, k, seed)).encode("latin-1"), np.uint8).reshape(70, 33))
        assert np.array_equal(got, again)
        assert all(sorted(normalise("".join(r[c] for r in shuffled(rows, k, seed)))) == sorted(normalise("".join(r[c] for r in rows)))
                   for c in range(33))


def test_seeds_repeat_and_differ():
    rows = random_rows(77, 12, 30)
    a, b, c = (significance(sequences=rows, samples=8, seed=s) for s in (5, 5, 6))
    for key in ("null_ge", "own_ge", "null_max"):
        assert getattr(a, key).tolist() == getattr(b, key).tolist(), key
    pairs, covs = [tuple(p) for p in a.observed.pair_cols.tolist()], a.observed.cov.tolist()
    assert null_stats(rows, pairs, covs, 4, 8, 5)[:3] != null_stats(rows, pairs, covs, 4, 8, 6)[:3]       # the restatement says they differ
    assert (a.null_ge.tolist(), a.own_ge.tolist(), a.null_max.tolist()) != (c.null_ge.tolist(), c.own_ge.tolist(), c.null_max.tolist())
    assert a.null_max.tolist() != c.null_max.tolist()


def test_null_ge_falls_with_cov_and_the_helpers():
    import torch
    rows = random_rows(5, 12, 33)
    res = significance(sequences=rows, samples=9, seed=1)
    cov, ge = res.observed.cov.tolist(), res.null_ge.tolist()
    by_cov = sorted(zip(cov, ge))
    assert all(g0 >= g1 for (_, g0), (_, g1) in zip(by_cov, by_cov[1:])) and len(set(ge)) > 3
    assert all(g0 == g1 for (c0, g0), (c1, g1) in zip(by_cov, by_cov[1:]) if c0 == c1)
    K = 9
    null_ge, own_ge, null_max = res.null_ge.numpy(), res.own_ge.numpy(), res.null_max.numpy()
    max_ge = (null_max[None, :] >= np.array(cov)[:, None]).sum(1)
    for got, exp in ((res.evalue(), null_ge.astype(np.float64) / np.float64(K)), (res.pvalue(), (1 + own_ge).astype(np.float64) / np.float64(K + 1)),
                     (res.pvalue_max(), (1 + max_ge).astype(np.float64) / np.float64(K + 1))):
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), exp)
    assert res.max_ge().tolist() == max_ge.tolist()
    assert res.significant().tolist() == (null_ge / K <= 0.05).tolist() and res.significant(evalue=2.0).tolist() == (null_ge / K <= 2.0).tolist()
    assert 0 < (res.pvalue() <= 1).sum() == len(res) and (res.pvalue_max() >= 1 / (K + 1)).all()
    v, w = res.observed.pair_cols[len(res) // 2].tolist()
    k = len(res) // 2
    rec = res.of(w, v)
    assert rec["cov"] == cov[k] and rec["null_ge"] == ge[k] and rec["own_ge"] == int(own_ge[k]) and rec["evalue"] == ge[k] / K
    assert rec["pvalue"] == (1 + int(own_ge[k])) / (K + 1) and rec["pvalue_max"] == (1 + int(max_ge[k])) / (K + 1) and rec["bp_rows"] >= 1
    with pytest.raises(KeyError):
        res.of(0, 1)
    for field, exp in (("null_ge", null_ge), ("own_ge", own_ge), ("evalue", res.evalue().numpy()), ("pvalue", res.pvalue().numpy()),
                       ("pvalue_max", res.pvalue_max().numpy()), ("cov", np.array(cov))):
        m = res.to_matrix(field)
        dense = np.zeros((33, 33), exp.dtype if exp.dtype.kind == "f" else np.int64)
        for (a, b), x in zip(res.observed.pair_cols.tolist(), exp.tolist()):
            dense[a, b] = dense[b, a] = x
        assert tuple(m.shape) == (33, 33) and np.array_equal(m.numpy(), dense), field
    assert torch.equal(res.to_matrix(), res.to_matrix("evalue"))
    with pytest.raises(ValueError):
        res.to_matrix("nothing")
    host = res.cpu()
    assert host.null_ge.tolist() == ge and host.observed.cov.tolist() == cov and host.null_cells == res.null_cells and len(host) == len(res)


def test_no_cell_in_scope():
    rows = random_rows(3, 6, 10)
    res = significance(sequences=rows, pairs=[(1, 7)], minspan=10, samples=4)
    assert res.null_cells == 0 and res.null_max.tolist() == [0] * 4 and res.null_ge.tolist() == [0]
    check_significance(res, rows, 10, 4, 0)


def test_the_planted_helices_stand_out():
    """40 rows x 60 columns, two planted helices of five pairs, 50 samples: first equality with the restatement, then what
    the restatement shows for this seed -- no sample reaches a planted pair's cov at its own cell, and the planted pairs have
    the smallest evalue of the table."""
    rows, planted = planted_rows()
    pairs, covs, null_ge, own_ge, null_max, null_cells = planted_stats()
    res = significance(sequences=rows, samples=PLANTED["samples"], seed=PLANTED["seed"])
    assert [tuple(p) for p in res.observed.pair_cols.tolist()] == pairs and res.observed.cov.tolist() == covs
    assert (res.null_ge.tolist(), res.own_ge.tolist(), res.null_max.tolist(), res.null_cells) == (null_ge, own_ge, null_max, null_cells)
    at = [pairs.index(p) for p in planted]
    evalue = res.evalue().tolist()
    assert all(res.own_ge[k] == 0 for k in at) and all(evalue[k] == min(evalue) for k in at)
    assert sum(e == min(evalue) for e in evalue) < len(evalue) // 10 and res.significant()[at].all() and not res.significant().all()


def test_argument_errors():
    rows = random_rows(9, 4, 12)
    for bad in (0, -3, 2.0, "7", None, True):
        with pytest.raises(ValueError, match="samples"):
            significance(sequences=rows, samples=bad)
    for bad in (-1, MASK + 1, 0.5, "1", None, False):
        with pytest.raises(ValueError, match="seed"):
            significance(sequences=rows, seed=bad)
    assert significance(sequences=rows, samples=np.int64(2), seed=MASK).samples == 2
    with pytest.raises(ValueError, match="CovariationSignificance"):
        significance(sequences=rows, inputfile=ALI)                         # two inputs
    with pytest.raises(ValueError):
        significance()                                                      # none
    with pytest.raises(AssertionError, match="not aligned"):
        significance(sequences=rows + ["ACGU"])
    with pytest.raises(RuntimeError, match="CovariationSignificance"):
        significance(sequences=rows, pairs=[(3, 12)])
    for kw in (dict(pairs="everything"), dict(pairs="steps"), dict(minspan=-1), dict(names=["a"])):
        with pytest.raises(ValueError, match="CovariationSignificance"):
            significance(sequences=rows, **kw)
    with pytest.raises(ValueError, match="65,535"):
        significance(sequences=["A"] * 65536, samples=1)


def test_covariation_is_unchanged():
    """The shared opening left Covariation what it was: its table on the inputs above, and its messages."""
    from tests.covariation_checks import check_records
    rows = random_rows(77, 12, 30)
    res = covariation(sequences=rows)
    check_records(res.pair_cols.tolist(), res.counts.tolist(), res.cov.tolist(), select(count_cells(rows), **DEFAULTS))
    with pytest.raises(ValueError, match="^Covariation: exactly one of inputfile, sequences and alignment is needed$"):
        covariation()
    with pytest.raises(ValueError, match="^Covariation: pairs='steps' needs alignment=$"):
        covariation(sequences=rows, pairs="steps")
    with pytest.raises(ValueError, match="^Covariation: minspan, min_rows and min_cov are non-negative integers$"):
        covariation(sequences=rows, min_cov=-1)
    with pytest.raises(RuntimeError, match="^Covariation: a pair is not 0 <= v < w < 30 columns$"):
        covariation(sequences=rows, pairs=[(3, 30)])
    with pytest.raises(ValueError, match="^Covariation: 1 names for 12 sequences$"):
        covariation(sequences=rows, names=["a"])
