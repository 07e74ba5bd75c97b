"""The covariation logic (squarna_amd/csrc/sq_covar.h, the logic of sq_covariation_scan), compiled for the host and run as one
thread -- planes from the rows, then every cell of every tile -- against the plain-Python references of
tests/covariation_checks.py: the naive one (row pairs, string Hamming distance) at tiny shapes, the count one at every row
count around the 64-row word and around the kernel's chunk of words.  All comparisons are exact."""
import os
import subprocess

import pytest

from tests.covariation_checks import (ALPHABET, D, DEFAULTS, EVERY_CELL, TYPES, count_cells, hamming, naive_cells, random_rows, select)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "covar_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "covar_host")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def run(exe, cases):
    """((TILE, WORD_CHUNK, MAX_BLOCKS), per case [(v, w, counts, cov)] sorted by (v, w)) for cases (rows, thresholds)."""
    lines = [str(len(cases))]
    for rows, thr in cases:
        L = len(rows[0])
        assert all(len(r) == L for r in rows) and not any(ch.isspace() for r in rows for ch in r)
        lines.append("%d %d %d %d %d" % (len(rows), L, thr["minspan"], thr["min_rows"], thr["min_cov"]))
        lines += rows
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = res.stdout.strip().split("\n")
    assert len(out) == len(cases) + 1
    got = []
    for line, (rows, _) in zip(out[1:], cases):
        nums, L = list(map(int, line.split())), len(rows[0])
        assert len(nums) == 1 + 9 * nums[0]
        recs = [nums[1 + 9 * k:10 + 9 * k] for k in range(nums[0])]
        assert len({r[0] for r in recs}) == len(recs)                        # no cell twice
        got.append(sorted((r[0] // L, r[0] % L, r[1:8], r[8]) for r in recs))
    return tuple(map(int, out[0].split())), got


def constants(exe):
    return run(exe, [])[0]


def check(exe, rows_list, cells_of):
    cases = [(rows, thr) for rows in rows_list for thr in (DEFAULTS, EVERY_CELL)]
    got = run(exe, cases)[1]
    for (rows, thr), g in zip(cases, got):
        assert g == select(cells_of(rows), **thr), (len(rows), len(rows[0]), thr)


def test_the_distance_table_is_the_hamming_distance():
    assert all(D[s][t] == hamming(TYPES[s], TYPES[t]) for s in range(6) for t in range(6))
    assert sum(D[s][t] for s in range(6) for t in range(s + 1, 6)) == 26


def test_constants_are_the_python_mirrors(exe):
    from squarna_amd import device_calls as dc
    assert constants(exe) == (dc.COVAR_TILE, dc.COVAR_WORD_CHUNK, dc.COVAR_MAX_BLOCKS) and dc.COVAR_MAX_BLOCKS == 2048


@pytest.mark.parametrize("R", [1, 2, 11])
def test_against_the_naive_reference(exe, R):
    rows_list = [random_rows(100 * R + L, R, L) for L in (1, 2, 5, 33, 40)]
    for rows in rows_list:
        assert count_cells(rows) == naive_cells(rows)                        # (the count reference itself, first)
    check(exe, rows_list, naive_cells)


@pytest.mark.parametrize("R", [63, 64, 65, 129])
def test_against_the_count_reference_around_the_word(exe, R):
    check(exe, [random_rows(R, R, L) for L in (31, 32, 33, 70)], count_cells)


def test_against_the_count_reference_around_the_chunk(exe):
    chunk = constants(exe)[1]
    check(exe, [random_rows(R, R, 20) for R in (64 * chunk - 1, 64 * chunk, 64 * chunk + 1)], count_cells)


def test_more_tiles_than_a_row_of_them(exe):
    """L = 3 tiles + 1: ten tiles in four rows, walked by tile_of (the harness checks its order)."""
    tile = constants(exe)[0]
    check(exe, [random_rows(7, 5, 3 * tile + 1, "ACGU-")], count_cells)


def test_special_alignments(exe):
    gap_col = [r[:3] + "-" + r[4:9] + "." + r[10:] for r in random_rows(3, 9, 14)]          # columns 3 and 9: all gaps
    same = ["GGGAAAUCCC-N"] * 7
    six = [t[0] + "NNNN" + t[1] for t in TYPES]
    got = run(exe, [(gap_col, EVERY_CELL), (same, EVERY_CELL), (six, EVERY_CELL), (six, DEFAULTS)])[1]
    assert got[0] == select(naive_cells(gap_col), **EVERY_CELL)
    cell = {(v, w): (c, cov) for v, w, c, cov in got[0]}
    assert cell[(3, 9)] == ([0, 0, 0, 0, 0, 0, 9], 0)
    assert all(sum(c[:6]) == 0 for (v, w), (c, _) in cell.items() if 3 in (v, w) or 9 in (v, w))
    assert got[1] == select(naive_cells(same), **EVERY_CELL)
    assert all(cov == 0 and sum(x > 0 for x in c[:6]) <= 1 for _, _, c, cov in got[1])
    cell = {(v, w): (c, cov) for v, w, c, cov in got[2]}
    assert cell[(0, 5)] == ([1, 1, 1, 1, 1, 1, 0], 26)                                      # the sum of d over t < t'
    assert got[3] == [(0, 5, [1, 1, 1, 1, 1, 1, 0], 26)]


def test_alphabet_classes(exe):
    """Every character of the alphabet against every other, one row each way: case, T, the three gaps, N and the separator."""
    rows = [a + "NNN" + b for a in ALPHABET for b in ALPHABET]
    got = run(exe, [(rows, EVERY_CELL)])[1][0]
    assert got == select(count_cells(rows), **EVERY_CELL)
    c, cov = {(v, w): (c, cov) for v, w, c, cov in got}[(0, 4)]
    assert c == [8, 8, 4, 4, 8, 8, 9]                                        # A, C, G: 2 spellings each, U: 4, gaps: 3
