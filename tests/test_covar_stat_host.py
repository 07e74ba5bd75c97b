"""The covariation-statistics logic (squarna_amd/csrc/sq_covar_stat.h, the logic of sq_covariation_stat_scan), compiled for
the host and run as one thread -- planes from the rows, pass 1 with the kernels' order of sums, pass 2 -- against the
plain-Python reference of tests/covariation_stat_checks.py.  Counters are compared exactly, S, C and the means under the float
bound derived there."""
import os
import subprocess

import pytest

from tests.covariation_checks import ALPHABET, random_rows
from tests.covariation_stat_checks import (BOUND, CORRECTIONS, DEFAULTS, EVERY_CELL, STATISTICS, Reference, check_means, check_records)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "covar_stat_host.cpp")


def _build(name, flags):
    exe = os.path.join(HERE, "native", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("covar_stat_host", ["-O2"])


@pytest.fixture(scope="module")
def exe_san():
    return _build("covar_stat_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def text_of(cases):
    lines = [str(len(cases))]
    for rows, statistic, correction, thr in cases:
        L = len(rows[0])
        assert all(len(r) == L for r in rows) and not any(ch.isspace() for r in rows for ch in r)
        floor = "-inf" if thr["min_stat"] is None else float(thr["min_stat"]).hex()
        lines.append("%d %d %d %d %d %d %s" % (len(rows), L, STATISTICS.index(statistic), CORRECTIONS.index(correction), thr["minspan"],
                                               thr["min_rows"], floor))
        lines += rows
    return "\n".join(lines) + "\n"


def run(exe, cases):
    """((TILE, WORD_CHUNK, MAX_BLOCKS), per case (means, [(v, w, n, S, C)] sorted by (v, w)))."""
    res = subprocess.run([exe], input=text_of(cases), capture_output=True, text=True, check=True)
    out = res.stdout.strip("\n").split("\n")
    assert len(out) == 2 * len(cases) + 1
    got = []
    for k, (rows, _, _, _) in enumerate(cases):
        L = len(rows[0])
        means = [float.fromhex(x) for x in out[1 + 2 * k].split()]
        words = out[2 + 2 * k].split()
        count = int(words[0])
        assert len(means) == L + 1 and len(words) == 1 + 19 * count
        recs = [words[1 + 19 * j:20 + 19 * j] for j in range(count)]
        assert len({r[0] for r in recs}) == count                            # no cell twice
        got.append((means, sorted((int(r[0]) // L, int(r[0]) % L, [int(x) for x in r[1:17]], float.fromhex(r[17]), float.fromhex(r[18]))
                                  for r in recs)))
    return tuple(map(int, out[0].split())), got


def constants(exe):
    return run(exe, [])[0]


def check(exe, rows_list, thresholds=(DEFAULTS, EVERY_CELL)):
    refs = [Reference(rows) for rows in rows_list]
    cases = [(rows, s, c, thr) for rows in rows_list for s in STATISTICS for c in CORRECTIONS for thr in thresholds]
    got = run(exe, cases)[1]
    for (rows, s, c, thr), (means, recs) in zip(cases, got):
        ref = refs[rows_list.index(rows)]
        what = (len(rows), len(rows[0]), s, c, thr)
        check_records(ref, s, c, [r[:2] for r in recs], [r[2] for r in recs], [r[3] for r in recs], [r[4] for r in recs],
                      ref.select(s, c, **thr), what)
        if c is None:
            assert means == [0.0] * (ref.L + 1) and all(r[3] == r[4] for r in recs)
        else:
            check_means(ref, s, means[:-1], means[-1], what)


def test_constants_are_the_python_mirrors(exe):
    from squarna_amd import device_calls as dc
    assert constants(exe) == (dc.COVAR_STAT_TILE, dc.COVAR_STAT_WORD_CHUNK, dc.COVAR_STAT_MAX_BLOCKS)
    assert dc.COVAR_STATISTICS == STATISTICS and dc.COVAR_CORRECTIONS == CORRECTIONS


@pytest.mark.parametrize("R", [1, 63, 64, 65])
def test_against_the_reference_around_the_word_and_the_tile(exe, R):
    tile = constants(exe)[0]
    check(exe, [random_rows(1000 * R + L, R, L) for L in (1, 2, tile - 1, tile, tile + 1, 3 * tile + 1)])


def test_around_the_chunk_of_words(exe):
    chunk = constants(exe)[1]
    check(exe, [random_rows(R, R, 20, "ACGU-") for R in (64 * chunk - 1, 64 * chunk, 64 * chunk + 1)])


def test_a_conserved_alignment_is_exactly_zero(exe):
    rows = ["GGGAAAUCCC-N"] * 7
    cases = [(rows, s, c, EVERY_CELL) for s in STATISTICS for c in CORRECTIONS]
    for means, recs in run(exe, cases)[1]:
        assert means == [0.0] * 13 and len(recs) == 12 * 11 // 2
        assert all(S == 0.0 and C == 0.0 for _, _, _, S, C in recs)           # ln 1 == 0; APC with mean_all == 0 leaves S
        assert {sum(n) for _, _, n, _, _ in recs} == {0, 7}


def test_an_all_gap_column_gives_zero_and_no_nan(exe):
    rows = [r[:3] + "-" + r[4:9] + "." + r[10:] for r in random_rows(3, 9, 14)]
    check(exe, [rows], thresholds=(EVERY_CELL,))
    for s in STATISTICS:
        (means, recs), = run(exe, [(rows, s, "apc", EVERY_CELL)])[1]
        assert means[3] == 0.0 and means[9] == 0.0
        assert all(n == [0] * 16 and S == 0.0 and C == 0.0 for v, w, n, S, C in recs if 3 in (v, w) or 9 in (v, w))


def test_selection_under_min_stat(exe):
    """The threshold lies in the widest gap of the reference's sorted values, and no reference value within the float bound
    of it: the record set is compared exactly."""
    rows = random_rows(21, 40, 45, "ACGU-", helices=3)
    ref = Reference(rows)
    cases, expected = [], []
    for s in STATISTICS:
        for c in CORRECTIONS:
            thr, half_gap = ref.gap_threshold(s, c)
            kept = ref.select(s, c, min_stat=thr)
            scope = ref.select(s, c)
            assert 0 < len(kept) < len(scope)
            assert all(abs(r[4] - thr) > BOUND * (abs(r[3]) + abs(ref.term(s, c, r[0], r[1]))) for r in scope)
            cases.append((rows, s, c, dict(DEFAULTS, min_stat=thr)))
            expected.append(kept)
    for (means, recs), exp in zip(run(exe, cases)[1], expected):
        assert [r[:3] for r in recs] == [r[:3] for r in exp]


def test_alphabet_classes(exe):
    """Every character of the alphabet against every other, one row each way: case, T, the three gaps, N and the separator."""
    rows = [a + "NNN" + b for a in ALPHABET for b in ALPHABET]
    (_, recs), = run(exe, [(rows, "gt", None, EVERY_CELL)])[1]
    n = {(v, w): n for v, w, n, _, _ in recs}[(0, 4)]
    per = {"A": 2, "C": 2, "G": 2, "U": 4}                                      # spellings of each residue in the alphabet
    assert n == [per[a] * per[b] for a in "ACGU" for b in "ACGU"]
    check(exe, [rows], thresholds=(EVERY_CELL,))


def test_the_harness_is_clean_under_the_sanitizers(exe, exe_san):
    """The same cases through a build with -fsanitize=address,undefined, run as a stand-alone program: the same output, bit
    for bit, and no report."""
    tile = constants(exe)[0]
    rows_list = [random_rows(65000 + L, 65, L) for L in (1, 2, tile + 1, 3 * tile + 1)]
    text = text_of([(rows, s, c, thr) for rows in rows_list for s in STATISTICS for c in CORRECTIONS for thr in (DEFAULTS, EVERY_CELL)])
    plain = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    checked = subprocess.run([exe_san], input=text, capture_output=True, text=True)
    assert checked.returncode == 0 and not checked.stderr, checked.stderr[-2000:]
    assert checked.stdout == plain.stdout and len(plain.stdout) > 10000
