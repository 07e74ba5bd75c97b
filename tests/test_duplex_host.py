"""The duplex summary (squarna_amd/csrc/sq_duplex.h, the logic of sq_duplex_summary), compiled for the host and run as one
thread, against sets of pairs: chains of every length around the 64-position chunk on either side of the separator,
homodimers, duplexes without an inter pair and with nothing else, and one planted violation of every kind of the validity
list on every row it applies to."""
import os
import random
import re
import subprocess

import pytest

from tests.fold_duplex_checks import BOUNDARY_LENGTHS, ROW_KINDS, duplex_row, expected_summary, pack_tables, plant_invalid, random_row

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "duplex_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "duplex_host")
HEADER = os.path.join(os.path.dirname(HERE), "squarna_amd", "csrc", "sq_duplex.h")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def run(exe, cases):
    """[(status, [valid per duplex], [nine numbers per duplex], bound)] for cases (tables of pack_tables, a_of, b_of)."""
    lines = [str(len(cases))]
    for t, a_of, b_of in cases:
        nsolo, ndup = len(t["lengths_s"]), len(a_of)
        assert len(t["cell_off_s"]) == nsolo + 1 and len(t["cell_off_d"]) == ndup + 1 and len(t["lengths_d"]) == ndup == len(b_of)
        assert len(t["pos_off"]) == nsolo + 1
        lines.append("%d %d %d %d %d %d" % (t["Ltot"], nsolo, ndup, len(t["partner_s"]), len(t["partner_d"]), t["same"]))
        for arr in (t["cell_off_s"], t["lengths_s"], t["partner_s"], t["cell_off_d"], t["lengths_d"], [] if t["same"] else t["partner_d"],
                    a_of, b_of, t["pos_off"]):
            lines.append(" ".join(map(str, arr)))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip().split("\n")
    assert len(rows) == len(cases)
    out = []
    for row, (t, a_of, _) in zip(rows, cases):
        nums = list(map(int, row.split()))
        P = len(a_of)
        assert len(nums) == 1 + 10 * P + t["Ltot"]
        recs = [nums[1 + 10 * k:11 + 10 * k] for k in range(P)]
        out.append((nums[0], [r[0] for r in recs], [r[1:] for r in recs], nums[1 + 10 * P:]))
    return out


def random_case(rng, lens, forced=(), kinds=ROW_KINDS):
    """Solo rows of the given lengths and 3-8 duplexes of them in any order, those of `forced` ((a, b) pairs) among them:
    (solo_rows, dup_rows, a_of, b_of, kinds of the duplex rows)."""
    solo_rows = [rng.choice([lambda n: random_row(rng, n), lambda n: random_row(rng, n, 0.95), lambda n: [-1] * n])(n) for n in lens]
    pairs = list(forced) + [(rng.randrange(len(lens)), rng.randrange(len(lens))) for _ in range(rng.randint(3, 8) - len(forced))]
    rng.shuffle(pairs)
    how = [rng.choice(kinds) for _ in pairs]
    dup_rows = [duplex_row(rng, kind, solo_rows[a], solo_rows[b]) for kind, (a, b) in zip(how, pairs)]
    return solo_rows, dup_rows, [a for a, _ in pairs], [b for _, b in pairs], how


def test_random_rows(exe):
    rng = random.Random(5)
    cases, expected, shapes, homodimers = [], [], set(), 0
    for trial in range(132):
        # the two chains of a forced duplex go through all pairs of boundary lengths' residues: every length on each side
        nA, nB = BOUNDARY_LENGTHS[trial % 11], BOUNDARY_LENGTHS[(trial // 11 + trial) % 11]
        lens = [nA, nB] + [rng.randint(0, 300) for _ in range(rng.randint(0, 3))]
        forced = [(0, 1)] + ([(rng.randrange(len(lens)),) * 2] if trial % 3 == 0 else [])
        solo_rows, dup_rows, a_of, b_of, how = random_case(rng, lens, forced)
        cases.append((pack_tables(rng, solo_rows, dup_rows, one_table=trial % 2 == 0, unrelated=rng.randint(0, 2)), a_of, b_of))
        expected.append(expected_summary(solo_rows, dup_rows, a_of, b_of) + (how,))
        shapes |= {("A", len(solo_rows[a])) for a in a_of} | {("B", len(solo_rows[b])) for b in b_of}
        homodimers += sum(a == b for a, b in zip(a_of, b_of))
    assert shapes >= {(side, n) for side in "AB" for n in BOUNDARY_LENGTHS} and homodimers >= 40
    got = run(exe, cases)
    for k, ((status, valid, summary, bound), (exp_summary, exp_bound, _)) in enumerate(zip(got, expected)):
        assert status == 0 and all(valid), k
        assert summary == exp_summary and bound == exp_bound, k
    every = [(row, kind) for exp, _, how in expected for row, kind in zip(exp, how)]
    rows = [row for row, _ in every]
    # the data cannot hide a dead column: every count is positive somewhere and zero somewhere, every site is set and unset
    assert all(any(r[c] > 0 for r in rows) and any(r[c] == 0 for r in rows) for c in range(5))
    assert all(any(r[c] >= 0 for r in rows) and any(r[c] == -1 for r in rows) for c in range(5, 9))
    assert any(r[5] != r[6] for r in rows) and any(r[7] != r[8] for r in rows) and any(r[5] > 0 for r in rows) and any(r[7] > 0 for r in rows)
    assert max(r[6] for r in rows) > 128 and max(r[7] for r in rows) > 64
    assert any(r[3] > 0 and r[0] == 0 for r in rows) and any(r[4] > 0 and r[0] == 0 for r in rows)
    assert sum(r[0] == 0 and r[1] + r[2] > 0 for r in rows) > 20                  # no inter pair
    assert sum(r[0] > 0 and r[1] + r[2] == 0 for r, kind in every if kind == "inter_only") > 20   # nothing but inter pairs
    assert any(r[:5] == [0, 0, 0, 0, 0] for r in rows) and any(r[0] > 0 and r[3] > 0 and r[4] > 0 for r in rows)


ENTRY_KINDS = ("outside", "below", "self", "asymmetric")
RECORD_KINDS = (("duplex_length_differs", None), ("negative_length", "A"), ("negative_length", "B"),
                ("longer_than_its_table", "D"), ("longer_than_its_table", "A"), ("longer_than_its_table", "B"),
                ("before_the_axis", "A"), ("before_the_axis", "B"), ("past_the_axis", "A"), ("past_the_axis", "B"),
                ("chain_not_a_solo", "A"), ("chain_not_a_solo", "B"), ("chain_negative", "A"), ("chain_negative", "B"),
                ("separator_paired", None), ("separator_paired_both_ways", None))


def _cut_table(partner, cell_off, lengths, r, cut):
    """The table with record r's cells ending `cut` entries inside its row 0: the rows behind move up."""
    lo, width = cell_off[r], cell_off[r + 1] - cell_off[r]
    keep = lengths[r] - cut
    partner = partner[:lo + keep] + partner[lo + width:]
    return partner, cell_off[:r + 1] + [c - (width - keep) for c in cell_off[r + 1:]]


def test_invalid_entries_and_records_give_status_2_and_the_rest_is_right(exe):
    rng = random.Random(7)
    cases, expected, seen = [], [], set()
    kinds = [(k, where) for k in ENTRY_KINDS for where in "ABD"] + list(RECORD_KINDS)
    for trial in range(6 * len(kinds)):
        kind, where = kinds[trial % len(kinds)]
        lens = [rng.randint(2, 150) for _ in range(rng.randint(3, 5))]
        solo_rows, dup_rows, a_of, b_of, _ = random_case(rng, lens, kinds=("dropped", "bind", "random", "inter_only"))
        exp_summary, exp_bound = expected_summary(solo_rows, dup_rows, a_of, b_of)
        k = rng.randrange(len(dup_rows))
        solo = a_of[k] if where == "A" else b_of[k] if where == "B" else None
        uses = lambda r: {q for q in range(len(a_of)) if r in (a_of[q], b_of[q])}
        bad = {k} if solo is None else uses(solo)
        sent_a, sent_b = list(a_of), list(b_of)
        if kind in ENTRY_KINDS:
            if where == "D":
                planted = plant_invalid(rng, dup_rows[k], kind)
                if planted is None:
                    continue
                dup_rows = dup_rows[:k] + [planted] + dup_rows[k + 1:]
            else:
                planted = plant_invalid(rng, solo_rows[solo], kind)
                if planted is None:
                    continue
                solo_rows = solo_rows[:solo] + [planted] + solo_rows[solo + 1:]
        elif kind.startswith("separator_paired"):
            D, nA = list(dup_rows[k]), lens[a_of[k]]
            free = [t for t, q in enumerate(D) if q == -1 and t != nA]
            if not free:
                continue
            D[nA] = rng.choice(free)
            if kind == "separator_paired_both_ways":                        # (a symmetric pair: only the separator's own check sees it)
                D[D[nA]] = nA
            dup_rows = dup_rows[:k] + [D] + dup_rows[k + 1:]
        t = pack_tables(rng, solo_rows, dup_rows, one_table=False, unrelated=rng.randint(0, 1))
        if kind == "duplex_length_differs":
            t["lengths_d"][k] += rng.choice((-1, 1))
        elif kind == "negative_length":
            t["lengths_s"][solo] = -1 - rng.randint(0, 2)
        elif kind == "longer_than_its_table" and where == "D":
            t["partner_d"], t["cell_off_d"] = _cut_table(t["partner_d"], t["cell_off_d"], t["lengths_d"], k, rng.randint(1, t["lengths_d"][k]))
        elif kind == "longer_than_its_table":
            t["partner_s"], t["cell_off_s"] = _cut_table(t["partner_s"], t["cell_off_s"], t["lengths_s"], solo, rng.randint(1, lens[solo]))
        elif kind == "before_the_axis":
            t["pos_off"][solo] = -1 - rng.randint(0, 2)
        elif kind == "past_the_axis":                                           # (the record's last positions lie behind the axis)
            t["pos_off"][solo] = t["Ltot"] - lens[solo] + rng.randint(1, 3)
        elif kind == "chain_not_a_solo":
            (sent_a if where == "A" else sent_b)[k] = len(lens) + rng.randint(0, 1)
            bad = {k}
        elif kind == "chain_negative":
            (sent_a if where == "A" else sent_b)[k] = -1 - rng.randint(0, 2)
            bad = {k}
        cases.append((t, sent_a, sent_b))
        touched = {r for q in bad for r in (a_of[q], b_of[q])}
        expected.append((exp_summary, exp_bound, bad, touched, t["pos_off"], lens))
        seen.add((kind, where))
    assert seen == set(kinds)
    for n, ((status, valid, summary, bound), (exp_summary, exp_bound, bad, touched, pos_off, lens)) in enumerate(zip(run(exe, cases), expected)):
        assert status == 2, n                                                   # every planted kind is reported
        assert [q for q, ok in enumerate(valid) if not ok] == sorted(bad), n    # ... for exactly the duplexes it affects
        assert all(summary[q] == exp_summary[q] for q in range(len(summary)) if q not in bad), n
        start = 0
        for r, length in enumerate(lens):                                       # (the untouched solo records' counts are whole)
            if r not in touched and start + length <= len(bound):
                assert bound[start:start + length] == exp_bound[start:start + length], n
            start += length


def test_invalid_solo_entry_in_one_table(exe):
    """Solos and duplexes in ONE table: a solo's entry planted there reaches its duplexes only."""
    rng = random.Random(9)
    solo_rows, dup_rows, a_of, b_of, _ = random_case(rng, [40, 70, 90], forced=[(0, 1), (2, 2)])
    exp_summary, _ = expected_summary(solo_rows, dup_rows, a_of, b_of)
    solo_rows[0] = plant_invalid(rng, random_row(rng, 40, 0.5), "self")
    (status, valid, summary, _), = run(exe, [(pack_tables(rng, solo_rows, dup_rows, one_table=True, unrelated=1), a_of, b_of)])
    bad = {q for q in range(len(a_of)) if 0 in (a_of[q], b_of[q])}
    assert status == 2 and [q for q, ok in enumerate(valid) if not ok] == sorted(bad)
    assert all(summary[q] == exp_summary[q] for q in range(len(summary)) if q not in bad)


def test_no_duplex(exe):
    t = pack_tables(random.Random(1), [[-1, 2, 1]], [], one_table=False)
    assert run(exe, [(t, [], [])]) == [(0, [], [], [0, 0, 0])]


def test_homodimer_of_a_hairpin_that_opens(exe):
    """One 8-nt hairpin against itself, fully paired across: 8 inter pairs, both copies' 3 pairs lost, every position bound
    twice -- once in either role."""
    A = [7, 6, 5, -1, -1, 2, 1, 0]
    D = [16 - t for t in range(8)] + [-1] + [7 - u for u in range(8)]
    assert expected_summary([A], [D], [0], [0]) == ([[8, 0, 0, 3, 3, 0, 7, 0, 7]], [2] * 8)
    (status, valid, summary, bound), = run(exe, [(pack_tables(random.Random(2), [A], [D]), [0], [0])])
    assert (status, valid, summary, bound) == (0, [1], [[8, 0, 0, 3, 3, 0, 7, 0, 7]], [2] * 8)


def test_the_grid_cap_is_the_one_python_sees():
    from squarna_amd import device_calls
    with open(HEADER) as fh:
        cap, = re.findall(r"#define SQ_DUPLEX_MAX_BLOCKS (\d+)", fh.read())
    assert int(cap) == device_calls.DUPLEX_SUMMARY_MAX_BLOCKS
