"""The shared logic of the statistics' shuffled-column null (squarna_amd/csrc/sq_covar_stat_null.h), compiled for the host and
run as one thread -- the bin search on doubles, the ordered integer key and the scratch layout -- against bisect, sorted and
max on Python floats.  Doubles travel as their 64 bits; all comparisons are exact.  The harness is also built with the
address and undefined-behaviour sanitizers and run once as the stand-alone program it is."""
import bisect
import math
import os
import random
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "covar_stat_null_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "covar_stat_null_host")
INF = float("inf")
TINY = 5e-324                                                               # the smallest denormal


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def unbits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def neighbours(x):
    return [math.nextafter(x, -INF), x, math.nextafter(x, INF)]


#: the doubles the checks care about: both zeros, both infinities, denormals, the largest and smallest normals and equal
#: neighbours of ordinary values
SPECIAL = [0.0, -0.0, INF, -INF, TINY, -TINY, 2.0 ** -1060, -2.0 ** -1060, 2.2250738585072014e-308, -2.2250738585072014e-308,
           1.7976931348623157e308, -1.7976931348623157e308] + neighbours(1.0) + neighbours(-1.0) + neighbours(37.125) + neighbours(-1e-9)


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def text_of(commands):
    return "\n".join([str(len(commands))] + [" ".join(str(x) for x in cmd) for cmd in commands]) + "\n"


def run(exe, commands):
    """(the header's constant, one list of ints per command)."""
    res = subprocess.run([exe], input=text_of(commands), capture_output=True, text=True, check=True)
    out = res.stdout.split("\n")
    assert len(out) == len(commands) + 2 and out[-1] == ""
    return int(out[0]), [list(map(int, line.split())) for line in out[1:-1]]


def doubles(values):
    return (len(values),) + tuple(bits(x) for x in values)


def thresholds_of(values):
    """Sorted distinct values as the engine forms them (torch.unique): -0.0 and 0.0 are one value."""
    out = []
    for x in sorted(values):
        if not out or x != out[-1]:
            out.append(x)
    return out


def bin_cases():
    rng = random.Random(11)
    wide = [rng.uniform(-50, 200) for _ in range(300)]
    queries = SPECIAL + wide[:40] + [x for t in wide[40:60] for x in neighbours(t)] + [rng.uniform(-60, 210) for _ in range(200)]
    return [([], SPECIAL), ([0.0], SPECIAL), ([-0.0], [0.0, -0.0, TINY, -TINY]), ([7.5], [7.4, 7.5, 7.6] + neighbours(7.5)),
            (thresholds_of(SPECIAL), SPECIAL + [3.0, -3.0, 1e-320, -1e-320]), (thresholds_of(wide), queries),
            ([-INF, INF], SPECIAL)]


def commands():
    cmds = [("bins",) + doubles(t) + doubles(q) for t, q in bin_cases()]
    cmds += [("keys",) + doubles(SPECIAL), ("back",) + doubles(SPECIAL), ("max",) + doubles([]), ("max",) + doubles(SPECIAL),
             ("max",) + doubles([-INF]), ("max",) + doubles([-0.0, 0.0, -0.0]), ("max",) + doubles([-3.5, -TINY, -7.0])]
    cmds += [("words", R, L, b) for R, L, b in ((1, 1, 1), (9, 20, 2), (65, 97, 3), (512, 5000, 7))]
    return cmds


def test_the_constant_is_the_python_mirror(exe):
    from squarna_amd import device_calls as dc
    assert run(exe, [])[0] == dc.COVAR_STAT_NULL_LDS_BINS >= 2


def test_bins_against_bisect(exe):
    cases = bin_cases()
    got = run(exe, [("bins",) + doubles(t) + doubles(q) for t, q in cases])[1]
    for (thr, queries), bins in zip(cases, got):
        assert thr == sorted(thr) and all(a < b for a, b in zip(thr, thr[1:]))
        assert bins == [bisect.bisect_right(thr, x) for x in queries] == [sum(t <= x for t in thr) for x in queries], thr[:3]
    assert got[0] == [0] * len(SPECIAL)                                      # U = 0
    assert got[2] == [1, 1, 1, 0]                                            # the zeros are one value: IEEE <=, not the keys' order
    assert got[3][:3] == [0, 1, 1] and got[3][3:] == [0, 1, 1]               # below, equal, above; and the equal neighbours
    assert got[6][SPECIAL.index(-INF)] == 1 and got[6][SPECIAL.index(INF)] == 2 and got[6][SPECIAL.index(0.0)] == 1


def test_keys_have_the_order_of_the_doubles_and_max_is_max(exe):
    rng = random.Random(3)
    more = SPECIAL + [rng.uniform(-1e3, 1e3) for _ in range(100)] + [rng.uniform(-1e-300, 1e-300) for _ in range(20)]
    lists = [[], SPECIAL, [-INF], [-0.0, 0.0, -0.0], [-3.5, -TINY, -7.0], more, [x for x in more if x < 0]]
    got = run(exe, [("keys",) + doubles(more), ("back",) + doubles(more)] + [("max",) + doubles(v) for v in lists])[1]
    keys = got[0]
    assert all(0 < k < 1 << 64 for k in keys)                                # key 0 stands for "no cell"
    for (x, kx) in zip(more, keys):
        for (y, ky) in zip(more, keys):
            assert (kx < ky) == (x < y or (bits(x), bits(y)) == (bits(-0.0), bits(0.0))), (x, y)
            assert (kx == ky) == (bits(x) == bits(y))
    assert got[1] == [bits(x) for x in more]                                 # unkey(key(x)) is x, bit for bit
    for values, (word,) in zip(lists, got[2:]):
        exp = max(values, default=-INF)
        assert unbits(word) == exp and (exp != 0 or word == bits(0.0 if any(bits(x) == 0 for x in values) else -0.0)), values[:3]
    assert got[2] == [bits(-INF)] and got[5] == [bits(0.0)]


def test_scratch_words(exe):
    shapes = ((1, 1, 1), (9, 20, 2), (65, 97, 3), (512, 5000, 7))
    got = run(exe, [("words",) + s for s in shapes])[1]
    for (R, L, batch), (words,) in zip(shapes, got):
        W, lpad, tiles = (R + 63) // 64, (L + 63) // 64 * 64, (L + 31) // 32
        assert words == batch * (5 * W * lpad + tiles * lpad + L + 1) + (R * L + 7) // 8


def test_the_harness_is_clean_under_the_sanitizers(exe, tmp_path):
    """The same commands through a build with -fsanitize=address,undefined, run as a stand-alone program: the same output and
    no report."""
    san = str(tmp_path / "covar_stat_null_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, SRC])
    cmds = commands()
    plain = subprocess.run([exe], input=text_of(cmds), capture_output=True, text=True, check=True)
    checked = subprocess.run([san], input=text_of(cmds), capture_output=True, text=True)
    assert checked.returncode == 0 and not checked.stderr, checked.stderr[-2000:]
    assert checked.stdout == plain.stdout and len(plain.stdout.split("\n")) == len(cmds) + 2
