"""The structure-distance logic (squarna_amd/csrc/sq_distances.h, the logic of sq_structure_distances), compiled for the host
and run as one thread -- planes from the partner rows, then every cell of every planned tile with its mirror, then the greedy
filter with the leaders group by group -- against the naive reference of tests/distances_checks.py (sets of pairs, a loop
over a list of kept rows).  The harness checks by itself that the plan covers every same-group cell exactly once and plans
no other tile, that the filter reads only words a tile wrote, and the matrix addresses.  It is built a second time as a
stand-alone program with the address and undefined-behaviour sanitizers and run on the same cases.  All comparisons are
exact."""
import os
import subprocess

import pytest

from tests.distances_checks import MODES, chain_rows, family_rows, naive, partners_of

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "distances_host.cpp")
BUILD = os.path.join(HERE, "native", "_build")
GROUP_SIZES = [0, 1, 3, 64, 65, 2, 0, 130]


def _build(name, flags):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("distances_host", ["-O2"])


@pytest.fixture(scope="module")
def exe_san():
    return _build("distances_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def as_partners(groups):
    """The groups' rows as partner lists: a dot-bracket string is parsed, a list is taken as it is."""
    return [[partners_of(r) if isinstance(r, str) else list(r) for r in rows] for rows in groups]


def run(exe, cases):
    """(the constants, per case the dict of host lists with `planes` and `tiles`) for cases (groups, mode, threshold): groups =
    a list per group of rows, each a dot-bracket string or a list of partners."""
    lines = [str(len(cases))]
    for groups, mode, threshold in cases:
        rows = [r for g in as_partners(groups) for r in g]
        lines.append("%d %d %d %d %d" % (len(rows), max(len(r) for r in rows), len(groups), MODES.index(mode), threshold))
        lines.append(" ".join(str(len(g)) for g in groups))
        lines += ["%d %s" % (len(r), " ".join(map(str, r))) for r in rows]
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout.strip().split("\n")
    assert len(out) == len(cases) + 1
    got = []
    for line, (groups, _, _) in zip(out[1:], cases):
        nums, S = list(map(int, line.split())), sum(len(g) for g in groups)
        planes, T = nums[:2]
        tiles, rest = nums[2:2 + 2 * T], nums[2 + 2 * T:]
        cells = rest[5 * S]
        assert len(rest) == 5 * S + 1 + cells and cells == sum(len(g) ** 2 for g in groups)
        got.append(dict(planes=planes, tiles=[tuple(tiles[2 * k:2 * k + 2]) for k in range(T)], status=rest[:S], npairs=rest[S:2 * S],
                        neighbours=rest[2 * S:3 * S], keep=[bool(x) for x in rest[3 * S:4 * S]], leader=rest[4 * S:5 * S],
                        common=rest[5 * S + 1:]))
    return tuple(map(int, out[0].split())), got


def constants(exe):
    return run(exe, [])[0]


def check(exe, cases):
    for (groups, mode, threshold), got in zip(cases, run(exe, cases)[1]):
        exp = naive([[r if isinstance(r, str) else None for r in g] for g in groups], mode, threshold)
        for key in exp:
            assert got[key] == exp[key], (key, [len(g) for g in groups], mode, threshold)


def shape_cases(chunk):
    """One group of S rows around the 64-row tile and word of the kept mask, widths around the 64-column word and the chunk."""
    cases = []
    for k, S in enumerate((1, 2, 63, 64, 65, 129)):
        for j, W in enumerate((1, 2, 63, 64, 65, 64 * chunk + 1)):
            rows = family_rows(1000 * S + W, S, W, families=max(S // 16, 2), knots=(k + j) % 2 == 1)
            cases.append(([rows], MODES[(k + j) % 2], ((0, 1, 2, 5), (0, 2500, 5000, 10000))[(k + j) % 2][(k + 2 * j) % 4]))
    return cases


def group_cases():
    sizes = GROUP_SIZES
    rows = family_rows(5, sum(sizes), 40, families=4, knots=True)
    cut = [sum(sizes[:k]) for k in range(len(sizes) + 1)]
    groups = [rows[a:b] for a, b in zip(cut, cut[1:])]
    mixed = [family_rows(7 + k, n, 20 + 9 * k, families=2) for k, n in enumerate([5, 0, 70, 3])]   # widths differ between groups
    return [(groups, "radius", 2), (groups, "relative", 2000), ([rows], "radius", 1), (mixed, "radius", 0), (mixed, "relative", 3000)]


def special_cases():
    bad = [[1, 0, 5], [1, 1], [2, 2, 0], [3, -1, -1], [-2, -1], "()()"]   # outside, self, not mutual, outside, below -1; the last is valid
    rows = ["(())..", "(())..", "(..)..", "......", "......", "((()))"]
    return [([rows + bad], "radius", 0), ([rows, bad], "relative", 5000), ([bad[:5]], "radius", 9), ([chain_rows(70)], "radius", 2),
            ([chain_rows(70)], "relative", 5000), ([chain_rows(130)], "radius", 2), ([["(((...)))"] * 70], "radius", 0)]


def test_constants_are_the_python_mirrors(exe):
    from squarna_amd import device_calls as dc
    assert constants(exe) == (dc.DISTANCES_TILE, dc.DISTANCES_WORD_CHUNK, dc.DISTANCES_MAX_BLOCKS, dc.DISTANCES_MAX_ROWS, dc.DISTANCES_MAX_COLS,
                              dc.DISTANCES_MAX_PLANES, dc.DISTANCES_FILTER_WORDS)
    assert dc.DISTANCES_TILE == 64 and dc.DISTANCES_MAX_ROWS == 65535 and dc.DISTANCES_MAX_COLS == 32768 and dc.DISTANCES_MODES == MODES
    # static LDS of the pairs kernel: both row ranges at 16 planes, and the mirror pieces
    assert 2 * dc.DISTANCES_MAX_PLANES * dc.DISTANCES_WORD_CHUNK * 64 * 8 + 512 <= 65536


def test_shapes_against_the_naive_reference(exe):
    check(exe, shape_cases(constants(exe)[1]))


def test_groups_against_the_naive_reference(exe):
    check(exe, group_cases())


def test_the_tile_plan_is_the_python_plan(exe):
    """The harness has checked that the plan covers every same-group cell once and holds no other tile; the plan Python
    uploads is the same list."""
    import numpy as np
    from squarna_amd.distances import plan_tiles
    for sizes in (GROUP_SIZES, [130], [64, 64], [63, 1, 64], [1] * 70, [0, 0, 5], [200, 0, 1], [64, 0, 0, 64, 1]):
        groups = [["()"] * n for n in sizes]
        got = run(exe, [(groups, "radius", 0)])[1][0]
        off = np.concatenate(([0], np.cumsum(sizes)))
        assert got["tiles"] == [tuple(t) for t in plan_tiles(off).tolist()], sizes
    one = run(exe, [([["()"] * 130], "radius", 0)])[1][0]["tiles"]
    assert one == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    split = run(exe, [([["()"] * 64, ["()"] * 66], "radius", 0)])[1][0]["tiles"]
    assert split == [(0, 0), (1, 1), (1, 2), (2, 2)]


def test_the_plane_count_at_the_powers_of_two(exe):
    """1 + the bits of Wmax - 1: width 2^k has k span planes, widths 2^k + 1 and 2^k + 2 have k + 1.  Two rows whose only
    pairs are (0, 1) and (0, W - 1) share nothing; at width 2^k + 2 their spans 1 and 2^k + 1 differ in the top bit alone."""
    for k in range(2, 10):
        for W, bits in ((2 ** k, k), (2 ** k + 1, k + 1), (2 ** k + 2, k + 1)):
            near_row, far_row = "()" + "." * (W - 2), "(" + "." * (W - 2) + ")"
            got = run(exe, [([[near_row, far_row, far_row]], "radius", 0)])[1][0]
            assert got["planes"] == 1 + bits, W
            assert got["common"] == [1, 0, 0, 0, 1, 1, 0, 1, 1] and got["keep"] == [True, True, False] and got["leader"] == [0, 1, 1], W
    assert run(exe, [([["."]], "radius", 0)])[1][0]["planes"] == 1 and run(exe, [([["()"]], "radius", 0)])[1][0]["planes"] == 2
    assert run(exe, [([["(" + "." * 32766 + ")"]], "radius", 0)])[1][0]["planes"] == 16


def test_special_rows(exe):
    cases = special_cases()
    check(exe, cases)
    got = run(exe, cases)[1]
    assert got[0]["status"] == [0] * 6 + [1] * 5 + [0] and got[0]["keep"] == [True, False, True, True, False, True] + [False] * 5 + [True]
    assert got[0]["leader"] == [0, 0, 2, 3, 3, 5, -1, -1, -1, -1, -1, 11] and got[0]["neighbours"] == [2, 2, 1, 2, 2, 1, 0, 0, 0, 0, 0, 1]
    assert got[2]["keep"] == [False] * 5 and got[2]["common"] == [0] * 25
    for chain in got[3:6]:
        n = len(chain["keep"])
        assert chain["neighbours"] == [2] + [3] * (n - 2) + [2] and chain["keep"] == [k % 2 == 0 for k in range(n)]
        assert chain["leader"] == [k - k % 2 for k in range(n)]
    assert got[6]["neighbours"] == [70] * 70 and got[6]["leader"] == [0] * 70


def test_the_filter_is_sequential(exe):
    """a ~ b, b ~ c, a !~ c at rows 63, 64, 65: b is dropped and protects nobody, so c is kept.  The 63 rows before them are
    invalid rows of the same group, or a group of their own (then the three's group begins in the middle of a word)."""
    three = ["()()....", "()()()..", "..()()()"]                                 # distances a-b 1, b-c 2, a-c 3
    for groups, ref in (([[[0]] * 63 + three], [[None] * 63 + three]), ([["." * 8] * 63, three], None)):
        got = run(exe, [(groups, "radius", 2)])[1][0]
        exp = naive(ref or groups, "radius", 2)
        assert {k: got[k] for k in exp} == exp
        assert got["keep"][63:] == [True, False, True] and got["leader"][63:] == [63, 63, 65] and got["neighbours"][63:] == [2, 3, 2]


def test_the_exact_thresholds(exe):
    rows = ["(((())))", "(((..)))", "(......)", "........", "........"]          # npairs 4 3 1 0 0
    for a, b, d in ((0, 1, 1), (0, 2, 3), (1, 2, 2), (0, 3, 4)):
        for radius, near in ((d, True), (d - 1, False)):
            got = run(exe, [([[rows[a], rows[b]]], "radius", radius)])[1][0]
            assert got["neighbours"] == [1 + near] * 2 and got["keep"] == [True, not near], (a, b, radius)
    # relative: d * 10000 <= T * (na + nb); rows 0 and 1: d = 1 of 7 pairs: the smallest T that admits them is 1429
    for T, near in ((1429, True), (1428, False)):
        assert run(exe, [([[rows[0], rows[1]]], "relative", T)])[1][0]["neighbours"] == [1 + near] * 2
    assert run(exe, [([[rows[3], rows[4]]], "relative", 0)])[1][0]["neighbours"] == [2, 2]      # two empty structures
    assert run(exe, [([[rows[2], rows[3]]], "relative", 9999)])[1][0]["neighbours"] == [1, 1]   # d = 1 of 1: only T = 10000 admits
    assert run(exe, [([[rows[2], rows[3]]], "relative", 10000)])[1][0]["neighbours"] == [2, 2]


def test_the_sanitized_harness_on_the_same_cases(exe, exe_san):
    cases = shape_cases(constants(exe)[1]) + group_cases() + special_cases()
    assert run(exe_san, cases) == run(exe, cases)
