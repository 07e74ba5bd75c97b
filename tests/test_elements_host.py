"""The loop annotation of Elements (squarna_amd/csrc/sq_elements.h, the logic of the kernels of sq_elements_dev.hip), compiled
for the host and run as one thread -- the per-column test of a listed opener, then that opener's walk -- with the levels fed
in from Python, against the naive reference of tests/elements_checks.py on the literal table and on random rows.  All
comparisons are exact."""
import os
import re
import subprocess

import pytest

from tests import elements_checks as EC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "elements_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "elements_host")
CSRC = os.path.join(os.path.dirname(HERE), "squarna_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def run(exe, cases):
    """(the constants, per case (element, loop_of, loops) in input columns) for cases (seq, partner row); a case whose row is
    invalid is not sent."""
    lines, sent = [], []
    for seq, row in cases:
        status, _, level, _, _, _, _ = EC.naive(seq, row)
        assert status == 0
        cols = [c for c, ch in enumerate(seq) if ch not in "-.~"]
        pos = {c: g for g, c in enumerate(cols)}
        part = [pos.get(int(row[c]), -1) if row[c] >= 0 else -1 for c in cols]
        lines += ["%d %d" % (len(cols), len(seq))] + [" ".join(map(str, v)) for v in
                                                     (part, [level[c] for c in cols], [int(seq[c] in ";&") for c in cols], cols)]
        sent.append((seq, level, cols))
    res = subprocess.run([exe], input="\n".join([str(len(sent))] + lines) + "\n", capture_output=True, text=True, check=True)
    out = res.stdout.split("\n")
    consts = tuple(map(int, out[0].split()))
    got = []
    for k, (seq, level, cols) in enumerate(sent):
        nums = list(map(int, out[1 + 3 * k].split()))
        loops = [tuple(nums[1 + 6 * t:7 + 6 * t]) for t in range(nums[0])]
        assert len(nums) == 1 + 6 * nums[0]
        lo, what = (list(map(int, out[2 + 3 * k + t].split())) for t in (0, 1))
        # what the levels kernel writes (GAP, BREAK, STEM, PK by the level) under what the walks wrote
        element = [8 if ch in "-.~" else 7 if ch in ";&" else 0 if not level[c] else 1 if abs(level[c]) == 1 else 6 for c, ch in enumerate(seq)]
        loop_of = [-1] * len(seq)
        for g, c in enumerate(cols):
            loop_of[c] = lo[g]
            if what[g] >= 0:
                element[c] = what[g]
        got.append((element, loop_of, loops))
    return consts, got


def check(exe, cases):
    for (seq, row), (element, loop_of, loops) in zip(cases, run(exe, cases)[1]):
        want = EC.naive(seq, row)
        assert (element, loop_of, loops) == (want[1], want[3], want[4]), (seq, list(row))


def test_constants_are_the_python_mirrors(exe):
    from squarna_amd import device_calls as dc
    from squarna_amd import elements as el
    consts = run(exe, [])[0]
    assert consts[:9] == (el.EXTERIOR, el.STEM, el.HAIRPIN, el.BULGE, el.INTERNAL, el.MULTI, el.PK, el.BREAK, el.GAP) == tuple(range(9))
    assert consts[9:] == (el.CODES, -1, dc.ELEMENTS_WAVES) and len(el.LETTERS) == el.CODES and el.LETTERS == EC.LETTERS
    define = lambda name, header: int(re.search(r"#define %s (\d+)" % name, open(os.path.join(CSRC, header)).read()).group(1))
    assert define("SQ_CHAIN_TMAX", "sq_device.h") == dc.ELEMENTS_MAX_STEMS and define("SQ_MAXLEVELS", "sq_internal.h") == dc.ELEMENTS_MAX_LEVELS


def test_the_literal_table(exe):
    cases = [(seq, EC.partner_row(dbn)) for seq, dbn, _, _ in EC.TABLE]
    for (seq, dbn, text, loops), (element, _, got) in zip(EC.TABLE, run(exe, cases)[1]):
        assert ''.join(EC.LETTERS[c] for c in element) == text and got == loops, (seq, dbn)
    check(exe, cases)


@pytest.mark.parametrize("gaps,sep", [(False, False), (True, False), (False, True), (True, True)])
def test_random_rows(exe, gaps, sep):
    check(exe, [EC.random_row(11 * w + k, w, k=k, gaps=gaps, sep=sep) for w in (0, 1, 5, 30, 64, 65, 150, 263) for k in range(7)])


def test_many_branches_and_deep_nesting(exe):
    """An exterior loop of 70 branches, 70 bulges inside one another, a multiloop of 66 hairpins."""
    wide, deep = "(...)" * 70, "(." * 70 + "..." + ")" * 70
    multi = "(" + "(...)" * 66 + ")"
    check(exe, [("A" * len(d), EC.partner_row(d)) for d in (wide, deep, multi)])
