"""The first fit in rounds (squarna_amd/csrc/sq_firstfit.h, the logic of sq_first_fit_dev), compiled for the host and run as
one thread, against the sequential pass sq_align_first_fit: the same pairs for every ranked list, within L / 2 + 1 rounds."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "firstfit_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "firstfit_host")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", EXE, SRC])
    return EXE


def sequential(flat, L, minspan):
    """The pairs sq_align_first_fit takes, as a partner list."""
    from squarna_amd import _lib
    arr = np.ascontiguousarray(flat, np.int64)
    out = np.empty(2 * (L // 2 + 1), np.int32)
    n = int(_lib.load().sq_align_first_fit(ctypes.c_void_p(arr.ctypes.data), ctypes.c_int64(len(arr)), int(L), int(minspan),
                                           ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(len(out) // 2)))
    assert 0 <= n <= len(out) // 2
    partner = [-1] * L
    for v, w in out[:2 * n].reshape(-1, 2).tolist():
        assert partner[v] == -1 and partner[w] == -1
        partner[v], partner[w] = w, v
    return partner, n


def in_rounds(exe, cases):
    """[(status, rounds, pairs, live, partner)] of the host-compiled header for cases (flat list, L, minspan)."""
    lines = [str(len(cases))]
    for flat, L, minspan in cases:
        lines.append("%d %d %d" % (L, minspan, len(flat)))
        lines.append(" ".join(map(str, flat)))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip().split("\n")
    assert len(rows) == len(cases)
    out = []
    for row in rows:
        nums = list(map(int, row.split()))
        out.append((nums[0], nums[1], nums[2], nums[3], nums[4:]))
    return out


def check(exe, cases):
    got = in_rounds(exe, cases)
    for (flat, L, minspan), (status, rounds, pairs, live, partner) in zip(cases, got):
        exp, n = sequential(flat, L, minspan)
        assert status == 0 and live == 0, (L, minspan, flat[:20])
        assert partner == exp, (L, minspan, flat[:20])
        assert pairs == n
        assert rounds <= L // 2 + 1
        assert (rounds == 0) == (not any(0 <= f < L * L and f % L > f // L and f % L - f // L >= minspan for f in flat))
    return got


def random_cases(seed, count):
    rng = random.Random(seed)
    cases = []
    for _ in range(count):
        L = rng.randint(2, 90)
        n = rng.randint(0, 4 * L)
        flat = []
        for _ in range(n):
            v, w = sorted(rng.sample(range(L), 2))
            flat.append(v * L + w)
            if rng.random() < 0.15:
                flat.append(flat[rng.randrange(len(flat))])            # the same pair again, at a worse rank
        rng.shuffle(flat)
        cases.append((flat, L, rng.choice((0, 4))))
    return cases


def test_random_ranked_lists(exe):
    got = check(exe, random_cases(101, 400))
    assert max(g[1] for g in got) >= 3                                   # (some lists need several rounds)


@pytest.mark.parametrize("minspan", [0, 4])
def test_chain_needs_a_round_per_pair(exe, minspan):
    """(0,10), (10,20), ...: every candidate shares a column with the one ranked before it, so a round takes the best live one
    and its neighbour dies -- about one round per accepted pair, the worst case of the bound."""
    L = 2001
    flat = [v * L + v + 10 for v in range(0, L - 10, 10)]
    (status, rounds, pairs, live, partner), = check(exe, [(flat, L, minspan)])
    assert pairs == (len(flat) + 1) // 2
    assert pairs - 1 <= rounds <= pairs + 1 <= L // 2 + 1


def test_dense_chain_at_the_bound(exe):
    """(0,1), (1,2), ..., minspan 0: L / 2 pairs in L / 2 rounds -- the bound L / 2 + 1 holds with one to spare."""
    for L in (2, 3, 10, 11, 64):
        flat = [v * L + v + 1 for v in range(L - 1)]
        (status, rounds, pairs, live, partner), = check(exe, [(flat, L, 0)])
        assert pairs == L // 2 and rounds <= L // 2 + 1


def test_duplicate_columns(exe):
    """Many candidates on few columns, every pair several times."""
    rng = random.Random(5)
    cases = []
    for L in (6, 9, 16):
        for _ in range(30):
            flat = []
            for _ in range(rng.randint(1, 60)):
                v, w = sorted(rng.sample(range(min(L, 7)), 2))
                flat += [v * L + w] * rng.randint(1, 3)
            rng.shuffle(flat)
            cases.append((flat, L, rng.choice((0, 4))))
    check(exe, cases)


def test_empty_single_and_invalid_candidates(exe):
    L = 12
    cases = [([], L, 0), ([], L, 4), ([2 * L + 9], L, 4), ([2 * L + 9], L, 0), ([2 * L + 4], L, 4),      # (span 2 < 4: no candidate)
             ([9 * L + 2, 2 * L + 9], L, 0),                                                                 # (w < v: no candidate)
             ([-5, L * L, L * L + 3, 1 * L + 7], L, 4)]                                                     # (outside the matrix)
    got = check(exe, cases)
    assert [g[2] for g in got] == [0, 0, 1, 1, 0, 1, 1]
    assert got[0][4] == [-1] * L and got[2][4][2] == 9 and got[2][4][9] == 2
