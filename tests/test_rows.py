"""The host helpers on partner rows (squarna_amd/rows.py) on hand-made cases, and what the result classes share
(results.TensorResult): ``device`` and ``cpu()`` of all eight, each built through the test-only CPU engines."""
import os

import numpy as np
import pytest
import torch

from squarna_amd import engine as E, rows as R
from squarna_amd import Covariation, Entropy, Fold, FoldAlignment, FoldDuplex, FoldMutants, FoldWindows, Score
from tests import entropy_checks as EC
from tests.oracle_engine import OracleEngine


def test_offsets():
    assert R.offsets([]).tolist() == [0] and R.offsets([]).dtype == np.int64
    for counts in ([3], [2, 0, 4], np.array([1, 5], np.int32), np.array([], np.int64)):
        got = R.offsets(counts)
        assert got.dtype == np.int64 and got.tolist() == [0] + np.cumsum(np.asarray(counts, np.int64)).tolist()


def test_position_axis():
    pos_off, total = R.position_axis(["ACG", "", "UU"])
    assert pos_off.tolist() == [0, 3, 3, 5] and total == 5 and isinstance(total, int)

    class Long(str):                                                 # (a record of 2^31 positions, without the memory)
        def __len__(self):
            return 2 ** 31 - 3
    with pytest.raises(ValueError, match=r"^2147483648 positions in all records: fewer than 2\^31 are needed$"):
        R.position_axis(["ACG", Long()])
    assert R.position_axis(["AC", Long()])[1] == 2 ** 31 - 1


@pytest.mark.parametrize("pairs,n", [([], 0), ([], 4), ([(0, 1)], 2), ([(0, 5), (1, 4)], 6), ([(1, 3), (2, 5)], 6)])
def test_partner_row_and_row_pairs_round_trip(pairs, n):
    row = R.partner_row(pairs, n)
    assert row.dtype == np.int32 and len(row) == n
    assert R.row_pairs(row) == pairs
    want = [-1] * n
    for v, w in pairs:
        want[v], want[w] = w, v
    assert row.tolist() == want
    assert R.partner_row(reversed(pairs), n).tolist() == want        # (row_pairs sorts: the order given does not matter)


def test_first_fit_keeps_the_order_taken():
    # six candidates in rank order; (2, 5) is blocked by its 3' end, (0, 3) by its 5' end, (1, 4) by both
    cands = [(1, 5), (0, 4), (2, 5), (0, 3), (1, 4), (2, 3)]
    taken = R.first_fit(cands)
    assert taken == [(1, 5), (0, 4), (2, 3)]                         # (not sorted: PairsToDBN sees this order)
    assert R.partner_row(taken, 6).tolist() == [4, 5, 3, 2, 0, 1]
    assert R.first_fit(iter(cands)) == taken and R.first_fit([]) == []
    assert R.first_fit([[0, 1], [1, 2]]) == [(0, 1)]                 # (rows of a table's tolist())


def test_checked_fit():
    text = r"^sq_first_fit_dev: %d candidates still live after %d rounds$"
    rounds = []
    R.checked_fit(torch.tensor([0, 3, 2, 0], dtype=torch.int32), rounds)
    R.checked_fit(np.array([0, 1, 0, 0], np.int32), rounds)
    R.checked_fit(torch.tensor([0, 9, 2, 0], dtype=torch.int32), None)
    assert rounds == [3, 1]
    with pytest.raises(RuntimeError, match=text % (0, 7)):           # a status
        R.checked_fit(torch.tensor([1, 7, 2, 0], dtype=torch.int32), rounds)
    with pytest.raises(RuntimeError, match=text % (5, 64)):          # candidates still live
        R.checked_fit(torch.tensor([0, 64, 2, 5], dtype=torch.int32), rounds)
    assert rounds == [3, 1]


def test_pair_table():
    # three records of 4, 0 and 5 entries: rows 0 and 2 hold (0, 3); the table's second rows are not consensus rows
    partner = np.array([3, 2, 1, 0, 9, 9, 9, 9, 3, -1, 4, 0, 2], np.int32)
    cell_off, lengths = np.array([0, 8, 8]), np.array([4, 0, 5])
    flat, count, first = R.pair_table(partner, cell_off, lengths, 6)
    assert all(a.dtype == np.int64 for a in (flat, count, first))
    assert flat.tolist() == [3, 8, 16] and count.tolist() == [2, 1, 1] and first.tolist() == [0, 0, 2]
    flat, count, first = R.pair_table(partner, cell_off, lengths, 100, base=np.array([10, 0, 20]))
    assert flat.tolist() == [1013, 1112, 2023, 2224] and count.tolist() == [1, 1, 1, 1] and first.tolist() == [0, 0, 2, 2]
    empty = R.pair_table(np.full(3, -1, np.int32), np.array([0]), np.array([3]), 3)
    assert [a.tolist() for a in empty] == [[], [], []] and empty[2].dtype == np.int64


# ---------------------------------------------------------------- results.TensorResult
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONF = "greedynobpp"
SEQS = ["GGGGCUAAAAGCCCCAAAAAAUCAGGUCAUCG", "GGGAAACCCAAAGGGAAACCC"]
RESULTS = {
    "FoldResult": lambda: Fold(records=SEQS, configfile=CONF),
    "AlignmentResult": lambda: FoldAlignment(os.path.join(GOLDEN, "align_synth", "u.afa")),
    "WindowResult": lambda: FoldWindows(records=SEQS, window=16, configfile=CONF),
    "MutantResult": lambda: FoldMutants(records=SEQS[1:], positions=[0, 4], configfile=CONF),
    "DuplexResult": lambda: FoldDuplex(targets=SEQS[:1], queries=SEQS[1:], configfile=CONF),
    "CovariationResult": lambda: Covariation(sequences=["GGGAAACCC", "GCGAAAUGC", "AGGA-ACCU"], minspan=2),
    "ScoreResult": lambda: Score(records=[("r", SEQS[1], None, None, "(((...)))...(((...)))")]),
    "EntropyResult": lambda: Entropy(records=SEQS, configfile=CONF),
}


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return a is b or a == b


def _equal(a, b):
    """Equal tensors, NaN equal to NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


def _check_cpu(res, got):
    assert type(got) is type(res) and got is not res
    assert list(vars(got)) == list(vars(res))
    assert res.device == getattr(res, res._TENSORS[0]).device and got.device.type == "cpu"
    for k, v in vars(res).items():
        w = getattr(got, k)
        if k in res._TENSORS:
            assert isinstance(v, torch.Tensor) and w.device.type == "cpu" and _equal(w, v.cpu()), k
        elif k in res._NESTED:
            assert (v is None and w is None) or _check_cpu(v, w) is None
        else:                                                        # host attributes and host caches: carried over unchanged
            assert not isinstance(v, torch.Tensor), "%s.%s is a tensor outside _TENSORS" % (type(res).__name__, k)
            assert _same(v, w), k


@pytest.mark.parametrize("name", sorted(RESULTS))
def test_cpu_moves_the_tensors_and_carries_the_rest(name):
    with E.use_engine(EC.EntropyOracleEngine() if name == "EntropyResult" else OracleEngine()):
        res = RESULTS[name]()
    assert type(res).__name__ == name and len(res._TENSORS) > 0
    _check_cpu(res, res.cpu())
    len(res.cpu())                                                   # (every class still counts what it counted)
    if name == "WindowResult":
        res.pairs(0)                                                 # fills the host cache of the pair offsets
        assert res._pair_off is not None and res.cpu()._pair_off is res._pair_off
        _check_cpu(res, res.cpu())
    if name in ("AlignmentResult", "WindowResult", "MutantResult", "DuplexResult"):
        assert any(getattr(res, k) is not None for k in res._NESTED)
