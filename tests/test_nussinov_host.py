"""The product's Nussinov restatement (squarna_amd/csrc/sq_nussinov.h), compiled for the host with a plain C++ compiler, against
the oracle's Nussinov: the same pair list, with and without separators in the sequence, and the column lists inside the region
of scratch the layout lends them.  (One thread: the rows of a column on many threads are what the GPU tests of
tests/test_hip_matching_many.py add.)"""
import os
import subprocess

import pytest

from tests import matching_checks as M
from tests.test_matching_reference import LARGE, SMALL

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "nussinov_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "nussinov_host")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EXE, SRC])
    return EXE


def _run(exe, problems):
    """problems: [(seq, cells)] -> [(bytes of the column lists, bytes they may take, sorted pairs)]"""
    from squarna_amd.dbn import encode_seq
    lines = [str(len(problems))]
    for seq, cells in problems:
        cells = [(v, w, x) for (v, w), x in M.dedup_cells(cells).items()]        # as sq_graph.hip's build_cells
        lines.append("%d %d" % (len(seq), len(cells)))
        lines.append(" ".join(str(c) for c in encode_seq(seq)))
        lines += ["%d %d %r" % c for c in cells]
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = [[int(x) for x in r.split()] for r in res.stdout.strip().split("\n")]
    assert len(rows) == len(problems)
    out = []
    for r in rows:
        assert len(r) == 3 + 2 * r[2]
        out.append((r[0], r[1], sorted(zip(r[3::2], r[4::2]))))
    return out


@pytest.mark.parametrize("seps", [False, True], ids=["plain", "separators"])
def test_pairs_equal_the_oracles(exe, seps):
    problems = [M.nussinov_case(seed, n, ncells, family, seps=seps) for seed, n, ncells, family in SMALL + LARGE]
    if seps:
        assert any(c in seq for seq, _ in problems for c in ";&") and any(w - v in (2, 3) for _, cells in problems for v, w, _ in cells)
    got = _run(exe, problems)
    assert any(len(pairs) > 20 for _, _, pairs in got)
    for (seq, cells), (used, room, pairs) in zip(problems, got):
        assert pairs == M.oracle_nussinov(seq, cells), (len(seq), len(cells))
        assert used <= room or len(seq) < 2
        if not seps:
            M.check_nussinov_pairs(len(seq), cells, pairs)


def test_shortest_sequences(exe):
    problems = [("", []), ("A", []), ("AU", []), ("AU", [(0, 1, 1.0)]), ("A;U", [(0, 2, 1.0)])]
    got = _run(exe, problems)
    assert [p for _, _, p in got] == [M.oracle_nussinov(seq, cells) for seq, cells in problems]


def test_column_lists_of_all_cells_end_inside_their_region(exe):
    """Every cell v < w of the matrix: the most a job of distinct cells can have.  12 m + 4 (2 n + 1) <= 8 n^2 from n = 2 on,
    with equality at n = 2."""
    problems = [("ACGU" * 18)[:n] for n in range(2, 71)]
    problems = [(seq, [(v, w, (0.5, 1.5, 3.5, 4.0)[(3 * v + w) % 4]) for v in range(len(seq)) for w in range(v + 1, len(seq))])
                for seq in problems]
    got = _run(exe, problems)
    for (seq, cells), (used, room, pairs) in zip(problems, got):
        n, m = len(seq), len(cells)
        assert m == n * (n - 1) // 2 and used == 12 * m + 4 * (2 * n + 1) and room == 8 * n * n and used <= room
        assert pairs == M.oracle_nussinov(seq, cells)
    assert got[0][0] == got[0][1]
