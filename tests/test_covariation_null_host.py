"""The definition of the shuffled-column null (squarna_amd/csrc/sq_covar_null.h), compiled for the host and run as one thread --
sort keys, the padded bitonic sort, bins, the closed form of the cells -- against the plain-Python restatement of
tests/covariation_null_checks.py.  All comparisons are exact.  The harness is also built with the address and
undefined-behaviour sanitizers and run once as the stand-alone program it is."""
import os
import random
import subprocess

import pytest

from squarna_amd.covariation_significance import scope_cells
from tests.covariation_null_checks import MASK, SEEDS, bin_of, order, scope, sortkey

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "covar_null_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "covar_null_host")
ROWS = (1, 2, 64, 65, 300)


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def run(exe, commands):
    """(the header's constants, one list of ints per command)."""
    text = "\n".join([str(len(commands))] + [" ".join(str(x) for x in cmd) for cmd in commands]) + "\n"
    res = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    out = res.stdout.split("\n")
    assert len(out) == len(commands) + 2 and out[-1] == ""
    return tuple(map(int, out[0].split())), [list(map(int, line.split())) for line in out[1:-1]]


def shuffle_cases():
    """(R, L, k, c, seed): every row count and seed, first and last column, sample 0 and samples whose index product wraps."""
    return [(R, L, k, c, seed) for R in ROWS for seed in SEEDS for L, k, c in ((1, 0, 0), (70, 3, 69), (5000, 99, 4321), (17, 2 ** 62 + 5, 16))]


def bin_cases():
    rng = random.Random(5)
    thr = sorted(rng.sample(range(1, 5000), 300))
    covs = [0, thr[0] - 1, thr[0], thr[0] + 1, thr[150], thr[150] - 1, thr[-1], thr[-1] + 1, 10 ** 12] + [rng.randrange(6000) for _ in range(200)]
    return [([], [0, 5, 10 ** 9]), ([7], [0, 6, 7, 8]), ([0], [0, 1]), (thr, covs), ([2 ** 40, 2 ** 62], [0, 2 ** 40, 2 ** 50, 2 ** 62, 2 ** 62 + 1])]


def commands():
    cmds = [("keys",) + case for case in shuffle_cases()] + [("order",) + case for case in shuffle_cases()]
    cmds += [("bins", len(t), *t, len(q), *q) for t, q in bin_cases()]
    cmds += [("cells", L, m) for L in (1, 2, 5, 33) for m in (0, 1, 4, 32, 33, 40)]
    return cmds


def test_constants_are_the_python_mirrors(exe):
    from squarna_amd import device_calls as dc
    max_rows, key_rows, lds_bins = run(exe, [])[0]
    assert (max_rows, lds_bins) == (dc.COVAR_NULL_MAX_ROWS, dc.COVAR_NULL_LDS_BINS) and max_rows >= 4096 and key_rows == 65535


def test_sort_keys_and_order_against_the_restatement(exe):
    cases = shuffle_cases()
    got = run(exe, [("keys",) + case for case in cases] + [("order",) + case for case in cases])[1]
    for (R, L, k, c, seed), keys, rows in zip(cases, got[:len(cases)], got[len(cases):]):
        assert keys == [sortkey(seed, k, c, r, R, L) for r in range(R)], (R, L, k, c, seed)
        assert len(set(keys)) == R and all(key & 0xFFFF == r and key < MASK for r, key in enumerate(keys))
        assert rows == order(seed, k, c, R, L) and sorted(rows) == list(range(R)), (R, L, k, c, seed)
    orders = {(R, seed): rows for (R, L, k, c, seed), rows in zip(cases, got[len(cases):]) if L == 70}
    assert orders[(300, SEEDS[0])] != orders[(300, SEEDS[1])] != list(range(300))      # the seeds shuffle, and differently


def test_bins_and_cells_against_the_restatement(exe):
    cases = bin_cases()
    cells = [(L, m) for L in (1, 2, 5, 33) for m in (0, 1, 4, 32, 33, 40)]
    got = run(exe, [("bins", len(t), *t, len(q), *q) for t, q in cases] + [("cells",) + c for c in cells])[1]
    for (thr, covs), bins in zip(cases, got):
        assert bins == [bin_of(thr, x) for x in covs], thr[:3]
    assert got[0] == [0, 0, 0] and got[1] == [0, 0, 1, 1] and got[2] == [1, 1]          # U = 0; below, equal, above one threshold
    assert [g[0] for g in got[len(cases):]] == [len(scope(L, m)) for L, m in cells] == [scope_cells(L, m) for L, m in cells]


def test_the_harness_is_clean_under_the_sanitizers(exe, tmp_path):
    """The same commands through a build with -fsanitize=address,undefined, run as a stand-alone program: the same output and
    no report."""
    san = str(tmp_path / "covar_null_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, SRC])
    cmds = commands()
    text = "\n".join([str(len(cmds))] + [" ".join(str(x) for x in cmd) for cmd in cmds]) + "\n"
    plain = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    checked = subprocess.run([san], input=text, capture_output=True, text=True)
    assert checked.returncode == 0 and not checked.stderr, checked.stderr[-2000:]
    assert checked.stdout == plain.stdout and len(plain.stdout.split("\n")) == len(cmds) + 2
