"""The window pair count (squarna_amd/csrc/sq_windows.h, the logic of sq_window_pair_count), compiled for the host and run as
one thread, against a dict count with the coverage by enumeration: every distinct pair exactly once, with its count, cover
and first holder, on random multi-record tables -- step 1, step = window, records shorter than the window, invalid entries."""
import os
import random
import subprocess

import pytest

from tests.fold_windows_checks import expected_global, pack_tables, synthetic_windows

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "windows_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "windows_host")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def run(exe, cases):
    """[(status, n, {(gi, gj): (count, cover, first)}, records stored)] for cases (Ltot, rec0, cap, partner, cell_off, starts, lens)."""
    lines = [str(len(cases))]
    for Ltot, rec0, cap, partner, cell_off, starts, lens in cases:
        lines.append("%d %d %d %d %d" % (Ltot, rec0, len(starts), cap, len(partner)))
        for arr in (cell_off, partner, starts, lens):
            lines.append(" ".join(map(str, arr)))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip().split("\n")
    assert len(rows) == len(cases)
    out = []
    for row, case in zip(rows, cases):
        nums = list(map(int, row.split()))
        recs = [nums[2 + 4 * k:6 + 4 * k] for k in range((len(nums) - 2) // 4)]
        table = {divmod(f, case[0]): (c, cov, first) for f, c, cov, first in recs}
        assert len(table) == len(recs), "a pair was given twice"
        out.append((nums[0], nums[1], table, len(recs)))
    return out


def random_case(rng, window=None, step=None, Ns=None):
    window = window or rng.randint(2, 40)
    step = step or rng.randint(1, window)
    Ns = Ns or [rng.randint(1, 120) for _ in range(rng.randint(1, 4))]
    gstart, lens, rows, per_rec = synthetic_windows(rng, Ns, window, step)
    return Ns, gstart, lens, rows, per_rec


def test_random_multi_record_tables(exe):
    rng = random.Random(5)
    shapes = [dict() for _ in range(300)]
    shapes += [dict(step=1) for _ in range(20)] + [dict(window=w, step=w) for w in (2, 7, 30)]
    shapes += [dict(window=50, Ns=[10, 50, 51, 3, 120]), dict(window=64, step=5, Ns=[1, 2, 63, 64, 65, 300])]
    cases, expected = [], []
    for shape in shapes:
        Ns, gstart, lens, rows, per_rec = random_case(rng, **shape)
        rec0 = rng.randint(0, 2)
        partner, cell_off = pack_tables(rows, rng, rec0)
        cases.append((sum(Ns), rec0, 1 << 20, partner, cell_off, gstart, lens))
        expected.append(expected_global(per_rec, Ns))
    got = run(exe, cases)
    assert max(c for exp in expected for c, _, _ in exp.values()) >= 5
    assert sum(len(exp) for exp in expected) > 5000
    for k, ((status, n, table, stored), exp) in enumerate(zip(got, expected)):
        assert status == 0 and n == stored == len(exp), k
        assert table == exp, k


def test_cap_below_the_count(exe):
    rng = random.Random(6)
    Ns, gstart, lens, rows, per_rec = random_case(rng, window=30, step=4, Ns=[100, 80])
    partner, cell_off = pack_tables(rows, rng)
    exp = expected_global(per_rec, Ns)
    assert len(exp) > 20
    for cap in (0, 1, 20, len(exp) - 1):
        (status, n, table, stored), = run(exe, [(sum(Ns), 0, cap, partner, cell_off, gstart, lens)])
        assert status == 0 and n == len(exp) and stored == cap
        assert all(exp[bp] == v for bp, v in table.items())


def _blank_invalid(per_rec, Ns, bad_windows):
    """per_rec with the rows of the windows in bad_windows (indices over all records) holding nothing."""
    out, k = [], 0
    for s, wlen, mine in per_rec:
        out.append((s, wlen, [[-1] * wlen if k + q in bad_windows else row for q, row in enumerate(mine)]))
        k += len(s)
    return out


def test_invalid_entries_give_status_2_and_the_rest_is_counted(exe):
    rng = random.Random(7)
    cases, expected, seen = [], [], set()
    for trial in range(60):
        Ns, gstart, lens, rows, per_rec = random_case(rng, window=rng.randint(6, 30), Ns=[rng.randint(20, 90) for _ in range(rng.randint(1, 3))])
        kind = ("outside", "below", "self", "asymmetric", "past_the_axis", "longer_than_its_table")[trial % 6]
        Ltot, bad_windows = sum(Ns), set()
        k = rng.randrange(len(rows))
        row = rows[k]                                                     # (the very list inside per_rec: edited in place)
        free = [t for t, p in enumerate(row) if p == -1]
        partner = cell_off = None
        if kind in ("outside", "below", "self"):
            if not free:
                continue
            t = rng.choice(free)
            row[t] = {"outside": len(row) + rng.randint(0, 3), "below": -2 - rng.randint(0, 3), "self": t}[kind]
        elif kind == "asymmetric":
            if len(free) < 1 or len(row) < 2:
                continue
            t = rng.choice(free)
            row[t] = rng.choice([p for p in range(len(row)) if p != t])   # (does not point back: row[p] is -1 or another)
        elif kind == "past_the_axis":
            Ltot -= rng.randint(1, 3)
            bad_windows = {q for q in range(len(rows)) if gstart[q] + lens[q] > Ltot}
            if not any(p > t for q in bad_windows for t, p in enumerate(rows[q])):
                continue
        else:
            partner, cell_off = pack_tables(rows, rng)
            cut = len(row) - rng.randint(1, len(row))                   # window k's table ends early: the rows move up
            lo = cell_off[k]
            width = cell_off[k + 1] - lo
            del partner[lo + cut:lo + width]
            cell_off = cell_off[:k + 1] + [c - (width - cut) for c in cell_off[k + 1:]]
            bad_windows = {k}
        if partner is None:
            partner, cell_off = pack_tables(rows, rng)
        exp = expected_global(_blank_invalid(per_rec, Ns, bad_windows), Ns)
        exp = {bp: v for bp, v in exp.items()}
        cases.append((Ltot, 0, 1 << 20, partner, cell_off, gstart, lens))
        expected.append((exp, sum(Ns)))
        seen.add(kind)
    assert len(seen) == 6
    got = run(exe, cases)
    for k, ((status, n, table, stored), (exp, full), case) in enumerate(zip(got, expected, cases)):
        assert status == 2, k
        # (pairs are reported on the axis the call named: gi * Ltot + gj)
        assert table == exp and n == len(exp), k
    assert sum(len(exp) for exp, _ in expected) > 300


def test_no_window_and_all_unpaired(exe):
    got = run(exe, [(10, 0, 4, [], [0], [], []), (30, 1, 4, [-1, 2, 1] + [-1] * 30, [0, 3, 13, 23, 33], [0, 10, 20], [10, 10, 10])])
    assert [(g[0], g[1], g[2]) for g in got] == [(0, 0, {}), (0, 0, {})]
