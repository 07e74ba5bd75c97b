"""The records and helpers of tests/bits_checks.py on the CPU: that AnnotateStems(minlen = 1, minscore = -1e9) of the empty
structure spells the oracle's bool matrix out cell for cell on the visited diagonals (what the GPU tests of the bit-matrix
kernels rest on), and that the record list has the properties it is there for."""
import numpy as np
import pytest

from tests import bits_checks as B


def test_visited_and_cells_of():
    v = B.visited(7)
    assert v.sum() == sum(1 for i in range(7) for j in range(i + 1, 7) if 4 <= i + j <= 8) and not v[0, 3] and v[0, 4] and not v[5, 6]
    m = B.cells_of([(0, 6, 2), (2, 4, 1)], 7)
    assert sorted(zip(*np.nonzero(m))) == [(0, 6), (1, 5), (2, 4)]
    with pytest.raises(AssertionError):
        B.cells_of([(0, 6, 2), (1, 5, 1)], 7)
    with pytest.raises(AssertionError):
        B.cells_of([(2, 4, 2)], 7)


@pytest.mark.parametrize("interchainonly", [False, True], ids=["all", "chain_test"])
def test_stems_of_the_empty_structure_are_the_matrix(interchainonly):
    """Every record under both pair tables: the stems list every true visited cell exactly once (cells_of asserts the
    "once"), as maximal runs -- no stem continues another on its diagonal."""
    outside = 0
    for name, rec in zip(B.NAMES, B.RECORDS):
        for which in (0, 1):
            m, stems = B.expected(rec, which, interchainonly)
            n = m.shape[0]
            assert n == len(rec[0])
            assert np.array_equal(B.cells_of(stems, n), m & B.visited(n)), (name, which)
            ends = {(i + ln, j - ln) for i, j, ln, _ in stems}
            assert not ends & {(i, j) for i, j, _, _ in stems}, (name, which, "a run was cut")
            outside += int((m & ~B.visited(n)).sum())
    if not interchainonly:
        assert outside > 0                     # true cells off the visited diagonals exist: the comparison must be masked


def test_the_record_list_has_what_it_is_there_for():
    lengths = [len(r[0]) for r in B.RECORDS[:15]]
    assert lengths == [5, 6, 31, 32, 33, 64, 65, 127, 128, 129, 160, 255, 256, 257, 300]
    used = [p for p, _ in B.PLACEMENTS]
    assert len(set(used)) == 7 and all(used.count(p) >= 2 for p in used), used
    for (seq, _, _), (place, at) in zip(B.RECORDS, B.PLACEMENTS):
        assert [p for p, ch in enumerate(seq) if ch in "&;"] == at, (place, at)
    n = lambda name: len(B.RECORDS[B.NAMES.index(name)][0])      # noqa: E731
    # more than one 256-diagonal tile per word-row (2n > 256) and several word-rows, on every kind of record
    multi = [name for name, r in zip(B.NAMES, B.RECORDS) if 2 * len(r[0]) > 256]
    assert {"129-31|32|33", "160-63+64", "255-first+last", "256-doubled", "257-none", "300-31|32|33", "129-restraints",
            "257-restraints", "300-restraints", "160-reacts", "300-reacts", "200-letters"} == set(multi)
    assert all(B.tiles_of(n(name))[1] > 1 and B.tiles_of(n(name))[0] > 4 for name in multi)
    # a separator on a word boundary: rows 31 | 32 and 63 | 64
    seps = {p for seq, _, _ in B.RECORDS for p, ch in enumerate(seq) if ch in "&;"}
    assert {31, 32, 63, 64} <= seps
    # restraint lines with every symbol, reactivities that are not all 0.5, all 26 letters
    for name in ("129-restraints", "257-restraints", "300-restraints"):
        line = B.RECORDS[B.NAMES.index(name)][2]
        assert set("_+/\\()[]") <= set(line) and len(line) == n(name)
    for name in ("65-reacts", "160-reacts", "300-reacts"):
        reacts = B.RECORDS[B.NAMES.index(name)][1]
        assert len(reacts) == n(name) and len(set(reacts)) > 10
    letters = B.RECORDS[B.NAMES.index("200-letters")][0]
    assert len(letters) == 200 and set("ABCDEFGHIJKLMNOPQRSTUVWXYZ") <= set(letters) and sum(letters.count(c) for c in "&;") == 2
    # the two pair tables give different matrices: a record owns two of them
    assert all(not np.array_equal(B.expected(r, 0, False)[0], B.expected(r, 1, False)[0]) for r in B.RECORDS if len(r[0]) > 30)
    assert set(B.GOLDEN_RECORDS) <= set(B.NAMES)


def test_the_long_record():
    """4,097 nt, three chains: one more than sq_fill_kernel's LDS paths hold (SQ_FILL_LDS_N = 4096), and more tiles than the
    2,048 blocks sq_bits_direct_kernel is launched with, so that its stride loop runs."""
    seq = B.BIG[0]
    assert len(seq) == 4097 and sum(seq.count(c) for c in "&;") == 2
    nw, ntile = B.tiles_of(4097)
    assert (nw, ntile) == (129, 33) and nw * ntile > 2048
    for ico in (False, True):
        for which in (0, 1):
            m, stems = B.expected(B.BIG, which, ico, **B.BIG_SETTINGS)
            assert len(stems) > 1000 and all(ln >= 3 and sc >= 4.5 for _, _, ln, sc in stems)
            assert all(m[i + k, j - k] for i, j, ln, _ in stems[::97] for k in range(ln))
