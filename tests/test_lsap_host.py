"""The product's Hungarian restatement (squarna_amd/csrc/sq_lsap.h), compiled for the host with a plain C++ compiler, against
scipy.optimize.linear_sum_assignment: the assignment scipy returns, in each of the three storage forms of a job.  The same
program prints the layout of a job's state and the decisions of a launch; tests/matching_checks.py states both a second time,
independently, and the two must agree.  (One lane: the cross-lane combine of the column scan is what the GPU tests of
tests/test_hip_matching_many.py add.)"""
import json
import os
import subprocess

import pytest

from tests import matching_checks as M
from tests.test_matching_reference import LARGE, SMALL

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "lsap_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "lsap_host")
AMPLE = 64 << 20

#: (seed, n, cells, weight family): n = 0 and 1, the grid of the references' test with its dyadic families (ties everywhere) and
#: again without ties, two sizes beyond 256 (several mask words per row, 16-bit prefix counts past 255)
CASES = ([(900, 0, 0, M.DYADIC[0]), (901, 1, 0, M.DYADIC[0])] + SMALL + [(s + 500, n, c, M.CONTINUOUS) for s, n, c, _ in SMALL] +
         [(s, n, 3 * n, f) for s, n, _, f in LARGE])


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EXE, SRC])
    return EXE


def _run(exe, problems):
    """problems: [(n, distinct cells, lds_bytes)] -> [(form, col4row)]"""
    lines = [str(len(problems))]
    for n, cells, lds in problems:
        lines.append("%d %d %d" % (n, len(cells), lds))
        lines += ["%d %d %r" % c for c in cells]
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip("\n").split("\n")
    assert len(rows) == len(problems)
    return [(r.split()[0], [int(x) for x in r.split()[1:]]) for r in rows]


def _distinct(cells):
    """What sq_graph.hip's build_cells hands the kernel: v < w, a repeated cell at its first place with its last weight."""
    return [(v, w, x) for (v, w), x in M.dedup_cells(cells).items()]


def test_assignments_equal_scipys_in_all_three_forms(exe):
    problems, expected = [], []
    for seed, n, ncells, family in CASES:
        n, cells = M.lsap_case(seed, n, ncells, family)
        exp, cells = M.scipy_col_ind(n, cells), _distinct(cells)
        m = len(cells)
        for form, lds in (("a", M.lsap_lds_bytes(n, m)), ("b", M.lsap_vec_bytes(n) + 64), ("c", 0)):
            problems.append((n, cells, lds))
            expected.append((form, exp, (seed, n, m)))
    assert {n for n, _, _ in problems} >= {0, 1, 2, 70, 257, 300}
    assert any(len(c) == 0 for n, c, _ in problems if n > 1) and max(len(c) / n for n, c, _ in problems if n) > 2.5
    got = _run(exe, problems)
    for (form, col4row), (eform, exp, what) in zip(got, expected):
        assert form == eform, what
        assert col4row == exp, (what, form)


def test_too_many_cells_for_16_bit_ids_take_the_dense_form(exe):
    """m = 32,767 distinct cells: form a would fit the LDS offered, but 2 m cells no longer count in 16 bits."""
    n, cells = M.lsap_case(4400, 260, 32767, M.DYADIC[2], flips=0.0, repeats=0.0)
    assert len(cells) == 32767 == len(M.dedup_cells(cells))
    assert M.lsap_lds_bytes(260, 32767) < AMPLE and M.lsap_form(260, 32767, [(260, 32767)]) == "b"
    (form, col4row), = _run(exe, [(n, cells, AMPLE)])
    assert form == "b" and col4row == M.scipy_col_ind(n, cells)
    (form, _), = _run(exe, [(260, cells[:32766], AMPLE)])
    assert form == "a"


DIMS = [(385, 3080), (800, 3000), (3655, 6000), (3656, 6000)]
MIXED = [(3656, 6000), (100, 200), (800, 3000)]


def test_layout_is_ordered_aligned_and_ends_at_the_size_functions(exe):
    dims = sorted({(n, (c * n) // 7) for _, n, _, _ in SMALL for c in (0, 1, 20)} | {(0, 0), (1, 0), (257, 700), (300, 900)} |
                  set(DIMS + MIXED))
    res = subprocess.run([exe, "layout"], input="".join("%d %d\n" % d for d in dims), capture_output=True, text=True, check=True)
    rows = [json.loads(x) for x in res.stdout.strip().split("\n")]
    assert len(rows) == len(dims)
    vectors = ("u", "v", "spc", "path", "col4row", "row4col", "remaining", "SR", "SC")
    sparse = ("wts", "mask", "rowstart", "pre", "cids")
    for (n, m), r in zip(dims, rows):
        def chain(names, at):
            """the arrays lie in this order from `at` on, each on a multiple of its element size; where the last one ends"""
            for name in names:
                off, size, count = r[name]
                assert off >= at and off % size == 0 and off - at < 16, (n, m, name)
                at = off + size * count
            return at
        nw = (n + 31) // 32
        assert [r[k][2] for k in vectors] == [n] * 9 and [r[k][2] for k in sparse] == [m, n * nw, n + 1, n * nw, 2 * m]
        assert [r[k][1] for k in vectors + sparse] == [8, 8, 8, 4, 4, 4, 4, 1, 1, 8, 4, 2, 2, 2]
        vec_end = chain(vectors, 0)
        assert r["u"][0] == 0 and r["vec_bytes"] == (vec_end + 15) // 16 * 16 == M.lsap_vec_bytes(n)
        assert r["wts"][0] == r["vec_bytes"]
        lds_end = chain(sparse, r["vec_bytes"])
        assert r["sparse_bytes"] == lds_end - r["vec_bytes"] + 16
        assert r["lds_bytes"] == r["vec_bytes"] + r["sparse_bytes"] + 64 == M.lsap_lds_bytes(n, m)
        # form c: the dense matrix, then the same vectors, in global scratch
        assert r["c_cost"] == [0, 8, n * n] and r["c_u"][0] == 8 * n * n and r["c_SC"][0] - r["c_u"][0] == r["SC"][0]
        assert r["scratch_bytes"] == r["c_SC"][0] + n + 64 == 8 * n * n + 42 * n + 64


def test_forms_of_a_launch_equal_the_python_statement(exe):
    launches = [[d] for d in DIMS] + [MIXED]
    res = subprocess.run([exe, "launch"], input="".join("%d %s\n" % (len(js), " ".join("%d %d" % j for j in js)) for js in launches),
                         capture_output=True, text=True, check=True)
    rows = [x.split() for x in res.stdout.strip().split("\n")]
    assert len(rows) == len(launches)
    for js, row in zip(launches, rows):
        need, lds, forms = int(row[0]), int(row[1]), row[2:]
        assert need == max(M.lsap_lds_bytes(n, m) for n, m in js)
        assert lds == (need if need <= M.LSAP_LDS_CAP else min(M.lsap_vec_bytes(max(n for n, _ in js)) + 64, M.LSAP_LDS_CAP))
        assert forms == [M.lsap_form(n, m, js) for n, m in js], js
    assert [r[2:] for r in rows] == [["a"], ["b"], ["b"], ["c"], ["c", "a", "b"]]
