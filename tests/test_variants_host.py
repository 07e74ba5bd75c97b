"""The variant comparison (squarna_amd/csrc/sq_variants.h, the logic of sq_variant_diff), compiled for the host and run as one
thread, against set differences of the rows' sets of pairs: random symmetric rows, all-unpaired rows, identical rows, lengths
around the 64-position chunk, and one planted invalid entry or record of every kind."""
import os
import random
import re
import subprocess

import pytest

from tests.fold_mutants_checks import expected_flat, nested_row, pack_records, perturbed, plant_invalid, random_row

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "variants_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "variants_host")
HEADER = os.path.join(os.path.dirname(HERE), "squarna_amd", "csrc", "sq_variants.h")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def run(exe, cases):
    """[(status, [valid per variant], [diff row per variant], pos_changed)] for cases (partner, cell_off, lengths, rec0, pos_off,
    Ltot, wt_of)."""
    lines = [str(len(cases))]
    for partner, cell_off, lengths, rec0, pos_off, Ltot, wt_of in cases:
        lines.append("%d %d %d %d" % (Ltot, rec0, len(wt_of), len(partner)))
        for arr in (cell_off, lengths, partner, wt_of, pos_off):
            lines.append(" ".join(map(str, arr)))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip().split("\n")
    assert len(rows) == len(cases)
    out = []
    for row, case in zip(rows, cases):
        nums = list(map(int, row.split()))
        V, Ltot = len(case[6]), case[5]
        assert len(nums) == 1 + 7 * V + Ltot
        recs = [nums[1 + 7 * m:8 + 7 * m] for m in range(V)]
        out.append((nums[0], [r[0] for r in recs], [r[1:] for r in recs], nums[1 + 7 * V:]))
    return out


def random_case(rng, lens, kinds=("random",)):
    """Wild types of the given lengths with 1-5 variants each, interleaved: (wt_rows, var_rows, wt_of)."""
    wt_rows, pairs = [], []
    for r, n in enumerate(lens):
        kind = rng.choice(kinds)
        w = {"random": lambda: random_row(rng, n), "unpaired": lambda: [-1] * n, "nested": lambda: nested_row(n)}[kind]()
        wt_rows.append(w)
        for _ in range(rng.randint(1, 5)):
            how = rng.random()
            v = list(w) if how < 0.2 else [-1] * n if how < 0.3 else random_row(rng, n) if how < 0.5 else perturbed(rng, w)
            pairs.append((rng.random(), v, r))
    pairs.sort(key=lambda e: e[0])                                          # (the wild types' variants interleaved)
    return wt_rows, [e[1] for e in pairs], [e[2] for e in pairs]


def test_random_rows(exe):
    rng = random.Random(5)
    cases, expected = [], []
    for trial in range(120):
        lens = [1, 2, 63, 64, 65, 129] if trial % 10 == 0 else [rng.randint(1, 300) for _ in range(rng.randint(1, 5))]
        wt_rows, var_rows, wt_of = random_case(rng, lens, ("random", "random", "unpaired", "nested"))
        cases.append(pack_records(rng, wt_rows, var_rows, wt_of, extra=rng.randint(0, 2)) + (wt_of,))
        expected.append(expected_flat(wt_rows, var_rows, wt_of))
    got = run(exe, cases)
    for k, ((status, valid, diff, pos_changed), (exp_diff, exp_pos)) in enumerate(zip(got, expected)):
        assert status == 0 and all(valid), k
        assert diff == exp_diff and pos_changed == exp_pos, k
    every = [d for exp, _ in expected for d in exp]
    assert sum(d[3] == 0 for d in every) > 50 and sum(d[0] > 0 and d[1] > 0 for d in every) > 100 and max(d[5] for d in every) > 250
    assert any(d == [0, 0, 0, 0, -1, -1] for d in every) and any(d[2] > 0 and d[3] == 0 for d in every)


ENTRY_KINDS = ("outside", "below", "self", "asymmetric")
RECORD_KINDS = ("lengths_differ", "longer_than_its_table", "past_the_axis", "wild_type_not_before_rec0", "wild_type_negative")


def test_invalid_entries_and_records_give_status_2_and_the_rest_is_right(exe):
    rng = random.Random(7)
    cases, expected, seen = [], [], set()
    kinds = [(k, where) for k in ENTRY_KINDS for where in ("variant", "wild type")] + [(k, None) for k in RECORD_KINDS]
    for trial in range(90):
        kind, where = kinds[trial % len(kinds)]
        lens = [rng.randint(2, 150) for _ in range(rng.randint(2, 4))]
        wt_rows, var_rows, wt_of = random_case(rng, lens)
        exp_diff, exp_pos = expected_flat(wt_rows, var_rows, wt_of)
        m = rng.randrange(len(var_rows))
        bad = {m}
        if where == "variant":
            planted = plant_invalid(rng, var_rows[m], kind)
            if planted is None:
                continue
            var_rows = var_rows[:m] + [planted] + var_rows[m + 1:]
        elif where == "wild type":
            planted = plant_invalid(rng, wt_rows[wt_of[m]], kind)
            if planted is None:
                continue
            wt_rows = wt_rows[:wt_of[m]] + [planted] + wt_rows[wt_of[m] + 1:]
            bad = {q for q, r in enumerate(wt_of) if r == wt_of[m]}
        partner, cell_off, lengths, rec0, pos_off, Ltot = pack_records(rng, wt_rows, var_rows, wt_of, extra=rng.randint(0, 1))
        sent = list(wt_of)
        if kind == "lengths_differ":
            lengths[rec0 + m] -= 1
        elif kind == "longer_than_its_table":                                # variant m's table ends early: the rows behind move up
            cut = rng.randint(1, lengths[rec0 + m])
            lo, width = cell_off[rec0 + m], cell_off[rec0 + m + 1] - cell_off[rec0 + m]
            del partner[lo + lengths[rec0 + m] - cut:lo + width]
            shift = width - (lengths[rec0 + m] - cut)
            cell_off = cell_off[:rec0 + m + 1] + [c - shift for c in cell_off[rec0 + m + 1:]]
        elif kind == "past_the_axis":
            Ltot -= 1
            bad = {q for q, r in enumerate(wt_of) if r == len(wt_rows) - 1}
            exp_pos = exp_pos[:-1]
        elif kind == "wild_type_not_before_rec0":
            sent[m] = rec0 + rng.randint(0, 1)
        elif kind == "wild_type_negative":
            sent[m] = -1 - rng.randint(0, 2)
        cases.append((partner, cell_off, lengths, rec0, pos_off, Ltot, sent))
        expected.append((exp_diff, exp_pos, bad, {wt_of[q] for q in bad}, pos_off))
        seen.add((kind, where))
    assert seen == set(kinds)
    for k, ((status, valid, diff, pos_changed), (exp_diff, exp_pos, bad, bad_wt, pos_off)) in enumerate(zip(run(exe, cases), expected)):
        assert status == 2, k                                               # every planted kind is reported
        assert [q for q, ok in enumerate(valid) if not ok] == sorted(bad), k
        assert all(diff[q] == exp_diff[q] for q in range(len(diff)) if q not in bad), k
        for r in range(len(pos_off) - 1):                                   # (the other wild types' counts are whole)
            if r not in bad_wt and pos_off[r + 1] <= len(pos_changed):
                assert pos_changed[pos_off[r]:pos_off[r + 1]] == exp_pos[pos_off[r]:pos_off[r + 1]], k


def test_no_variant(exe):
    got = run(exe, [([-1, 2, 1], [0, 3], [3], 1, [0, 3], 3, [])])
    assert got == [(0, [], [], [0, 0, 0])]


def test_the_grid_cap_is_the_one_python_sees():
    from squarna_amd import device_calls
    with open(HEADER) as fh:
        cap, = re.findall(r"#define SQ_VARIANT_MAX_BLOCKS (\d+)", fh.read())
    assert int(cap) == device_calls.VARIANT_DIFF_MAX_BLOCKS
