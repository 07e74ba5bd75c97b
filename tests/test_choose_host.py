"""The product's ChooseStems (squarna_amd/csrc/sq_choose.h), compiled for the host with a plain C++ compiler, against the
oracle's pinned restatement (oracle.sqrn_pyform._choose_stems): the stopper's pick and the full choice with its two overflows,
on lists in which nearly every comparison is a tie.  The oracle gets the stems in ascending key order -- the order they are
emitted in --, so its stable sort gives the tie rule; the harness gets them shuffled.  (One lane: the cross-lane gather and
conflict test are what the GPU parity tests of tests/test_hip_lowcomplex.py add.)"""
import glob
import os
import random
import re
import subprocess

import pytest

from oracle.sqrn_pyform import _choose_stems

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "choose_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "choose_host")
CSRC = os.path.join(os.path.dirname(HERE), "squarna_amd", "csrc")
INF = float("inf")
CMAX = 64                       # SQ_POOL_CMAX (test_one_define_and_one_conflict_test reads it back)


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def key_of(st):
    return ((st[0] + st[1]) << 16) | st[0]


def expect(stems, subopt, cap, cmax):
    """(pick, choice) the harness must print for stems [(i, j, len, bps, fin)]: the oracle's list, or the overflow that comes first"""
    ordered = sorted(stems, key=key_of)
    res = _choose_stems(ordered, subopt)
    best = max(s[4] for s in stems)
    rng = subopt * best
    in_range = sum(1 for s in stems if not s[4] < rng)
    if in_range > cap:
        choice = "ovf range"
    elif len(res) > min(CMAX, cmax):
        choice = "ovf picks"
    else:
        choice = (in_range, [(key_of(s), s[2], s[3], s[4]) for s in res])
    return key_of(res[0]), rng, choice


def run(exe, cases, width="32", seed=1):
    """cases: [(stems, subopt, cap, cmax)] -> [(pick, choice)], the stems handed over in shuffled order"""
    rnd = random.Random(seed)
    lines = [str(len(cases))]
    for stems, subopt, cap, cmax in cases:
        rng = subopt * max(s[4] for s in stems)
        mixed = list(stems)
        rnd.shuffle(mixed)
        lines.append("%r %d %d %d" % (rng, cap, cmax, len(mixed)))
        lines += ["%d %d %r %r" % (key_of(s), s[2], s[3], s[4]) for s in mixed]
    res = subprocess.run([exe, width], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip("\n").split("\n")
    assert len(rows) == 2 * len(cases)
    got = []
    for p, c in zip(rows[0::2], rows[1::2]):
        pick = None if p == "pick none" else int(p.split()[1])
        if c.startswith("ovf"):
            got.append((pick, c))
            continue
        f = c.split()
        taken, in_range, rest = int(f[0]), int(f[1]), f[2:]
        assert len(rest) == 4 * taken
        got.append((pick, (in_range, [(int(rest[4 * k]), int(rest[4 * k + 1]), float(rest[4 * k + 2]), float(rest[4 * k + 3]))
                                      for k in range(taken)])))
    return got


def check(exe, cases, width="32"):
    got = run(exe, cases, width)
    for k, ((stems, subopt, cap, cmax), (pick, choice)) in enumerate(zip(cases, got)):
        epick, _, echoice = expect(stems, subopt, cap, cmax)
        assert pick == epick, (k, subopt, cap, cmax)                 # the stopper's pick == _choose_stems(...)[0]
        assert choice == echoice, (k, subopt, cap, cmax, stems)
    return got


def random_case(rnd):
    """1-200 stems of 1-6 pairs with distinct (i, j) on 12-80 positions, finalscores from at most three values, some at -inf; in
    half of the cases most stems hold one common position, so that long results occur"""
    n = rnd.randint(12, 80)
    want = rnd.randint(1, 200)
    values = [rnd.choice([1.5, 2.0, 2.25, 7.0, 10.0]) for _ in range(rnd.randint(1, 3))]
    hub = rnd.randrange(n) if rnd.random() < 0.5 else None
    stems, seen = [], set()
    for _ in range(20 * want):
        if len(stems) == want:
            break
        ln = rnd.randint(1, 6)
        if hub is not None and rnd.random() < 0.8:                   # the hub on the 5' or the 3' strand
            if rnd.random() < 0.5:
                i = hub - rnd.randrange(ln)
                j = rnd.randint(i + 2 * ln - 1, n - 1) if i >= 0 and i + 2 * ln - 1 <= n - 1 else -1
            else:
                j = hub + rnd.randrange(ln)
                i = rnd.randint(0, j - 2 * ln + 1) if j <= n - 1 and j - 2 * ln + 1 >= 0 else -1
        else:
            i = rnd.randint(0, n - 1)
            j = rnd.randint(i, n - 1)
        if i < 0 or j < 0 or j - i + 1 < 2 * ln or (i, j) in seen:
            continue
        seen.add((i, j))
        fin = -INF if rnd.random() < 0.15 else rnd.choice(values)
        stems.append((i, j, ln, float(rnd.randint(6, 40)) / 2, fin))
    if not stems or all(s[4] == -INF for s in stems):
        stems.append((0, n - 1, 1, 3.0, values[0]))
    return stems


def refused_between_accepted(stems, subopt):
    """does the conflict filter refuse a candidate that stands between two accepted ones?"""
    ordered = sorted(stems, key=key_of)
    res = _choose_stems(ordered, subopt)
    rng = subopt * res[0][4]
    ranked = [s for s in sorted(ordered, key=lambda s: s[4], reverse=True) if not s[4] < rng]
    flags = [s in res for s in ranked]
    return any(not f and any(flags[t + 1:]) for t, f in enumerate(flags))


@pytest.mark.parametrize("width", ["32", "16"])
def test_random_tie_heavy_lists_equal_the_oracle(exe, width):
    rnd = random.Random(20240)
    cases = []
    for k in range(320):
        stems = random_case(rnd)
        cases.append((stems, [1.0, 0.9, 0.5, 0.0][k % 4], 256, CMAX))
    got = check(exe, cases, width)
    sizes = {len(c[1]) for _, c in got if not isinstance(c, str)}
    assert 1 in sizes and 2 in sizes and max(sizes) >= 5
    assert any(refused_between_accepted(stems, subopt) for stems, subopt, _, _ in cases)
    assert max(len(s) for s, _, _, _ in cases) >= 150 and min(len(s) for s, _, _, _ in cases) <= 5
    assert any(s[4] == -INF for stems, _, _, _ in cases for s in stems)


def test_all_equal_one_stem_and_single_shared_bases(exe):
    a = (10, 40, 3, 9.0, 4.0)
    shares = [(12, 30, 3, 8.0, 4.0),        # 5' strand with 5' strand: position 12
              (2, 10, 3, 8.0, 4.0),         # its 3' strand with a's 5' strand: position 10
              (40, 50, 3, 8.0, 4.0),        # its 5' strand with a's 3' strand: position 40
              (20, 38, 3, 8.0, 4.0)]        # 3' strand with 3' strand: position 38
    beside = (13, 37, 3, 8.0, 4.0)          # adjacent on both strands, no base in common
    rnd = random.Random(7)
    equal = [(s[0], s[1], s[2], s[3], 5.0) for s in random_case(rnd) if s[4] != -INF]
    cases = [(equal, 1.0, 256, CMAX), ([a], 1.0, 256, CMAX), ([a], 0.0, 1, 1)]
    cases += [([a, b], 1.0, 256, CMAX) for b in shares] + [([a, beside], 1.0, 256, CMAX)]
    got = check(exe, cases)
    assert [len(c[1]) for _, c in got[1:]] == [1, 1, 2, 2, 2, 2, 1]
    assert got[0][1][0] == len(equal)                                # all of them within range


def hub_stems(count, fin=3.0):
    """`count` stems that all hold position 30 on their 5' strand: any two share a base"""
    return [(30, 40 + k, 1, 6.0 + k, fin) for k in range(count)]


def test_capacity_edge(exe):
    got = check(exe, [(hub_stems(7), 1.0, 7, CMAX), (hub_stems(8), 1.0, 7, CMAX),
                      (hub_stems(7) + [(0, 5, 1, 6.0, -INF)], 1.0, 7, CMAX)])         # (-inf never passes the range)
    assert len(got[0][1][1]) == 7 and got[1][1] == "ovf range" and len(got[2][1][1]) == 7


def test_picks_edge(exe):
    three = hub_stems(3)
    fourth_all = (30, 50, 1, 6.0, 3.0)                               # position 30 again: shares a base with all three
    fourth_not = (41, 60, 1, 6.0, 3.0)                               # position 41: the second stem's 3' end only
    got = check(exe, [(three, 1.0, 256, 3), (three + [fourth_all], 1.0, 256, 3), (three + [fourth_not], 1.0, 256, 3),
                      (hub_stems(CMAX), 1.0, 256, 1000), (hub_stems(CMAX + 1), 1.0, 256, 1000)])
    assert len(got[0][1][1]) == 3 and got[1][1] == "ovf picks" and len(got[2][1][1]) == 3
    assert len(got[3][1][1]) == CMAX and got[4][1] == "ovf picks"


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))


def test_one_define_and_one_conflict_test():
    """SQ_POOL_CMAX is defined once and the base-sharing test of :783-786 is written once, both in sq_choose.h"""
    defines, bodies = [], []
    for path in _sources():
        with open(path) as fh:
            text = fh.read()
        for m in re.finditer(r"#\s*define\s+SQ_POOL_CMAX\s+(\d+)", text):
            defines.append((os.path.basename(path), int(m.group(1))))
        # a definition: a name that ends in shares_base, its parameter list, then a body
        bodies += [os.path.basename(path) for _ in re.finditer(r"\w*shares_base\s*\([^(){};]*\)\s*(?://[^\n]*)?\s*\{", text)]
    assert defines == [("sq_choose.h", CMAX)]
    assert bodies == ["sq_choose.h"]
