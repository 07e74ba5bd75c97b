"""The projection logic (squarna_amd/csrc/sq_project.h, the logic of sq_project_rows and sq_lift_rows), compiled for the host
and run as one thread -- the chunk walk with its ballot words and exclusive bases, col_of / pos_of, the validity pass, the
judgement of every paired column with the counts, and the lift through the search over the bases and the select within a
word -- against the naive reference of tests/project_checks.py (plain loops over characters).  The harness checks by itself
that every output cell is written exactly where it belongs, that col(pos(c)) == c, and select64.  It is built a second time
as a stand-alone program with the address and undefined-behaviour sanitizers and run on the same cases.  All comparisons
are exact."""
import os
import subprocess

import pytest

from squarna_amd import device_calls as dc
from squarna_amd.device_calls import PROJECT_COUNTS
from tests.project_checks import (WIDTHS, aligned_rows, class_line, naive, naive_lift, short_lines, special_rows, structure_line)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "project_host.cpp")
BUILD = os.path.join(HERE, "native", "_build")


def _build(name, flags):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("project_host", ["-O2"])


@pytest.fixture(scope="module")
def exe_san():
    return _build("project_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _take(nums, at, shape):
    """(the nested lists of `shape` from nums[at:], the position after them)."""
    n = 1
    for s in shape:
        n *= s
    flat = nums[at:at + n]
    for s in reversed(shape[1:]):
        flat = [flat[k:k + s] for k in range(0, len(flat), s)]
    return flat, at + n


def run(exe, cases):
    """(the constants, per case a dict of lists in the form of naive() / naive_lift()).  A case is ("project", rows, lines,
    canonical_only, min_loop) with lines = K partner lists (shared) or per row K lists, or ("lift", rows, short, width) with
    short[r] = the lines of row r over `width` >= its residues entries (None: the row's own length)."""
    text = [str(len(cases))]
    for case in cases:
        rows = case[1]
        R, L = len(rows), len(rows[0])
        if case[0] == "project":
            lines, canonical_only, min_loop = case[2:]
            shared = not isinstance(lines[0][0], (list, tuple))
            K = len(lines) if shared else len(lines[0])
            text.append("0 %d %d %d %d %d %d" % (R, L, K, shared, canonical_only, min_loop))
            text += rows
            text += [" ".join(map(str, p)) for p in (lines if shared else [p for mine in lines for p in mine])]
        else:
            short, width = case[2:]
            K = max(max(len(mine) for mine in short), 1)
            text.append("1 %d %d %d 0 0 0" % (R, L, K))
            text += rows
            for row, mine in zip(rows, short):
                n = sum(ch not in "-.~" for ch in row)
                w = n if width is None else width
                text.append("%d %d" % (len(mine), w))
                text += [" ".join(map(str, list(p) + [-1] * (w - len(p)))) for p in mine]
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout.strip().split("\n")
    assert len(out) == len(cases) + 1
    got = []
    for line, case in zip(out[1:], cases):
        nums = list(map(int, line.split()))
        rows = case[1]
        R, L, Lmax = len(rows), len(rows[0]), nums[0]
        length, at = _take(nums, 1, (R,))
        assert Lmax == max(max(length), 1)
        col_of, at = _take(nums, at, (R, Lmax))
        pos_of, at = _take(nums, at, (R, L))
        assert all(x == -1 for row, n in zip(col_of, length) for x in row[n:])
        rec = dict(length=length, col_of=[row[:n] for row, n in zip(col_of, length)], pos_of=pos_of)
        if case[0] == "project":
            K = len(case[2]) if not isinstance(case[2][0][0], (list, tuple)) else len(case[2][0])
            partner, at = _take(nums, at, (R, K, Lmax))
            rec["cls"], at = _take(nums, at, (R, K, L))
            rec["counts"], at = _take(nums, at, (R, K, 12))
            rec["status"], at = _take(nums, at, (R, K))
            assert all(x == -1 for lines, n in zip(partner, length) for p in lines for x in p[n:])
            rec["partner"] = [[p[:n] for p in lines] for lines, n in zip(partner, length)]
        else:
            K = max(max(len(mine) for mine in case[2]), 1)
            partner, at = _take(nums, at, (R, K, L))
            status, at = _take(nums, at, (R, K))
            for lines, st, mine in zip(partner, status, case[2]):
                assert all(x == -1 for p in lines[len(mine):] for x in p) and not any(st[len(mine):])
            rec["partner"] = [lines[:len(mine)] for lines, mine in zip(partner, case[2])]
            rec["status"] = [st[:len(mine)] for st, mine in zip(status, case[2])]
        assert at == len(nums)
        got.append(rec)
    return tuple(map(int, out[0].split())), got


def check(exe, cases):
    for case, got in zip(cases, run(exe, cases)[1]):
        exp = naive(case[1], *case[2:]) if case[0] == "project" else naive_lift(case[1], case[2])
        for key in exp:
            assert got[key] == exp[key], (key, case[0], len(case[1]), len(case[1][0]), case[3:])


def shape_cases():
    """Every width of the issue: random rows beside the rows that are all gaps, have no gap, or have gaps only in the first
    or the last chunk; K = 1 and 3, shared and per-row lines, both directions."""
    cases = []
    for j, L in enumerate(WIDTHS):
        rows = aligned_rows(100 + L, 5, L) + special_rows(L)
        for K in (1, 3):
            shared = [structure_line(10 * L + k, L, knots=k == 1) for k in range(K)]
            per_row = [[structure_line(1000 * L + 10 * r + k, L, knots=(r + k) % 2 == 1) for k in range(K)] for r in range(len(rows))]
            cases.append(("project", rows, shared, (j + K) % 2 == 1, (0, 3)[j % 2]))
            cases.append(("project", rows, per_row, (j + K) % 2 == 0, (3, 0)[j % 2]))
            cases.append(("lift", rows, short_lines(L + K, rows, K, knots=K == 3), None))
        cases.append(("lift", rows, short_lines(L, rows, 2), L + 3))                              # padded lines
        cases.append(("lift", rows, [short_lines(L, [row], r % 3)[0] for r, row in enumerate(rows)], None))   # 0, 1 or 2 lines a row
    return cases


def rule_cases():
    """min_loop 0, 3 and a value that drops every pair, canonical_only both ways, on lines in which every class occurs."""
    rows = aligned_rows(7, 12, 130, gap_share=0.25)
    lines = [class_line(rows[0]), structure_line(3, 130, knots=True)]
    return [("project", rows, lines, co, ml) for co in (0, 1) for ml in (0, 3, 130)]


INVALID = [[1, 0, 6] + [-1] * 3, [0] + [-1] * 5, [2, 2, 0] + [-1] * 3, [-2] + [-1] * 5, [1, 2, 0] + [-1] * 3]   # outside, self, not mutual, below -1, a cycle


def invalid_cases():
    rows = ["GC-AUN", "-.~-.~", "gcaugc"]
    good = [5, 4, -1, -1, 1, 0]
    per_row = [[good, bad] for bad in INVALID[:3]]
    short_bad = [[[1, 0, 5, -1, -1], [0, -1, -1, -1, -1]], [[]], [[2, 2, 0, -1, -1, -1], [5, 4, -1, -1, 1, 0]]]
    return [("project", rows, [good] + INVALID, 0, 0), ("project", rows, per_row, 0, 0), ("lift", rows, short_bad, None)]


def test_constants_are_the_python_mirrors(exe):
    assert PROJECT_COUNTS == 12 and run(exe, [])[0] == (dc.PROJECT_THREADS, dc.PROJECT_MAX_BLOCKS, dc.PROJECT_MAX_COLS, dc.PROJECT_MAX_ROWS, dc.PROJECT_MAX_WORDS,
                               dc.PROJECT_COUNTS)
    assert dc.PROJECT_MAX_COLS == 32768 and dc.PROJECT_MAX_ROWS == 2 ** 20 and dc.PROJECT_MAX_WORDS * 64 == dc.PROJECT_MAX_COLS
    # static LDS of a block: the ballot words, the bases, the class bytes, the table, the counters and the flag
    assert 8 * dc.PROJECT_MAX_WORDS + 4 * (dc.PROJECT_MAX_WORDS + 1) + dc.PROJECT_MAX_COLS + 256 + 4 * dc.PROJECT_COUNTS + 4 <= 65536


def test_shapes_against_the_naive_reference(exe):
    check(exe, shape_cases())


def test_the_kept_rule_and_every_class(exe):
    cases = rule_cases()
    check(exe, cases)
    got = run(exe, cases)[1]
    total = [sum(c[0][q] for c in got[0]["counts"]) for q in range(12)]
    assert all(total[q] > 0 for q in range(1, 10)), total          # every class occurs on the first line
    for rec, (_, _, _, co, ml) in zip(got, cases):
        for row in rec["counts"]:
            for c in row:
                assert c[0] == sum(c[1:10]) and c[11] == sum(c[1:7]) + (0 if co else c[7]) - c[10]
                assert ml < 130 or c[11] == 0


def test_invalid_lines(exe):
    cases = invalid_cases()
    check(exe, cases)
    got = run(exe, cases)[1]
    assert got[0]["status"] == [[0, 1, 1, 1, 1, 1]] * 3 and got[1]["status"] == [[0, 1]] * 3
    assert got[0]["counts"][0][1] == [0] * 12 and got[0]["partner"][0][1] == [-1] * 5 and got[0]["cls"][0][1] == [0] * 6
    assert got[2]["status"] == [[1, 1], [0], [1, 0]] and got[2]["partner"][2][1] == [5, 4, -1, -1, 1, 0]


def test_one_long_row(exe):
    """The longest row the kernels take: 512 chunk words, a pair across the whole row."""
    L = 32768
    row = ("GA-CU." * (L // 6 + 1))[:L]
    line = [-1] * L
    line[0], line[L - 2] = L - 2, 0
    line[1], line[3] = 3, 1
    got = run(exe, [("project", [row], [line], 0, 0)])[1][0]
    exp = naive([row], [line])
    assert got == {k: exp[k] for k in got} and got["counts"][0][0][0] == 2


def test_the_sanitized_harness_on_the_same_cases(exe, exe_san):
    cases = shape_cases() + rule_cases() + invalid_cases()
    assert run(exe_san, cases) == run(exe, cases)
