"""The logic of the weighted statistics' shuffled-column null (squarna_amd/csrc/sq_covar_wstat_null.h and the headers it
joins), compiled for the host and run as one thread -- the shuffle, the weighted counters of the shuffled planes, raw_w(), the
bin search and the key of the maximum -- against WeightedReference of tests/covariation_wstat_checks.py on shuffled() rows of
tests/covariation_null_checks.py.  The counters are compared exactly, S under the float bound derived there, the histogram and
the maximum exactly against bisect and max on the harness's own S.  The LDS layout of the null's scan kernel and the scratch
offsets are checked here too, and the harness runs once more under the address and undefined-behaviour sanitizers as the
stand-alone program it is."""
import bisect
import os
import struct
import subprocess

import pytest

from tests.covariation_checks import random_rows
from tests.covariation_null_checks import SEEDS, scope, shuffled
from tests.covariation_stat_checks import BOUND, STATISTICS
from tests.covariation_wstat_checks import WeightedReference, random_weights

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "covar_wstat_null_host.cpp")
REGIONS = ("planes", "q", "bins", "S", "row", "col", "flat", "raw", "em", "thresholds", "hist", "top")
KERNELS = ("sums", "scan", "pairs", "null")
SHAPES = ((1, 1, 1), (9, 20, 2), (65, 97, 3), (257, 33, 1), (512, 5000, 7))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def unbits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def _build(name, flags):
    exe = os.path.join(HERE, "native", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("covar_wstat_null_host", ["-O2"])


def text_of(commands):
    lines = [str(len(commands))]
    for cmd in commands:
        if cmd[0] == "words":
            lines.append(" ".join(str(x) for x in cmd))
            continue
        _, rows, weights, statistic, minspan, K, seed, thresholds = cmd
        L = len(rows[0])
        assert all(len(r) == L for r in rows) and not any(ch.isspace() for r in rows for ch in r) and len(weights) == len(rows)
        assert list(thresholds) == sorted(set(thresholds))
        lines.append("null %d %d %d %d %d %d %d %s" % (len(rows), L, STATISTICS.index(statistic), minspan, K, seed, len(thresholds),
                                                       " ".join(str(bits(t)) for t in thresholds)))
        lines.append(" ".join(float(w).hex() if w == w and abs(w) != float("inf") else repr(float(w)) for w in weights))
        lines += rows
    return "\n".join(lines) + "\n"


def run(exe, commands):
    """((LDS_BINS, TILE, WORD_CHUNK, MAX_ROWS), {kernel: (total, {region: (offset, size)})}, per command: the six offsets of
    `words`, or (status, per sample ([(v, w, Q, S)], hist, max)) of `null`)."""
    res = subprocess.run([exe], input=text_of(commands), capture_output=True, text=True, check=True)
    out = res.stdout.strip("\n").split("\n")
    assert len(out) == len(commands) + 5
    layouts = {}
    for kernel, line in zip(KERNELS, out[1:5]):
        words = [int(x) for x in line.split()]
        assert len(words) == 1 + 2 * len(REGIONS)
        layouts[kernel] = (words[0], {name: (words[1 + 2 * k], words[2 + 2 * k]) for k, name in enumerate(REGIONS)})
    got = []
    for cmd, line in zip(commands, out[5:]):
        words = line.split()
        if cmd[0] == "words":
            got.append([int(x) for x in words])
            continue
        K, U = cmd[5], len(cmd[7])
        at, samples = 1, []
        for _ in range(K):
            cells = int(words[at])
            recs = [words[at + 1 + 19 * j:at + 20 + 19 * j] for j in range(cells)]
            at += 1 + 19 * cells
            hist, most = [int(x) for x in words[at:at + U + 1]], unbits(int(words[at + U + 1]))
            at += U + 2
            samples.append(([(int(r[0]), int(r[1]), [int(x) for x in r[2:18]], float.fromhex(r[18])) for r in recs], hist, most))
        assert at == len(words)
        got.append((int(words[0]), samples))
    return tuple(map(int, out[0].split())), layouts, got


def test_the_constants_are_the_python_mirrors(exe):
    from squarna_amd import device_calls as dc
    assert run(exe, [])[0] == (dc.COVAR_WSTAT_NULL_LDS_BINS, dc.COVAR_STAT_TILE, dc.COVAR_STAT_WORD_CHUNK, dc.COVAR_NULL_MAX_ROWS)
    assert dc.COVAR_WSTAT_NULL_LDS_BINS >= 2 and dc.COVAR_NULL_MAX_ROWS < 65535 < dc.COVAR_WSTAT_MAX_ROWS


def test_the_null_kind_places_disjoint_aligned_regions_and_the_old_kinds_are_what_they_were(exe):
    (lds_bins, tile, chunk, _), layouts, _ = run(exe, [])
    total, regions = layouts["null"]
    assert {name for name, (_, size) in regions.items() if size} == {"planes", "q", "bins", "thresholds", "hist", "top"}
    spans = sorted((at, at + size, name) for name, (at, size) in regions.items() if size)
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans                      # disjoint
    assert all(at % 16 == 0 for at, _, _ in spans), spans
    assert all(0 <= at <= total for at, _ in regions.values()) and spans[-1][1] <= total < 64 * 1024, total
    assert regions["thresholds"][1] == 8 * lds_bins and regions["hist"][1] == 4 * lds_bins and regions["top"][1] == 8
    assert regions["bins"][1] == 16 * 256 * 8 and regions["planes"][1] == 2 * 4 * chunk * tile * 8 and regions["q"][1] == 64 * chunk * 4
    assert 3 * total <= 160 * 1024                                           # three blocks per CU, as the unweighted null's scan
    # the three kinds of before, as the numbers they were: planes 8 KB, q 1 KB, bins 32 KB, then the kernel's own regions
    old = {"sums": (50944, dict(planes=0, q=8192, bins=9216, S=41984, row=50432, col=50688)),
           "scan": (58384, dict(planes=0, q=8192, bins=9216, flat=41984, raw=50176, em=58368)),
           "pairs": (32768, dict(bins=0))}
    for kernel, (was_total, was) in old.items():
        now_total, now = layouts[kernel]
        assert now_total == was_total, kernel
        assert {name: at for name, (at, size) in now.items() if size} == was, kernel
        assert all(now[name][1] == 0 for name in ("thresholds", "hist", "top")), kernel
        # an empty region lies at the offset of the one after it: the new ones at the total
        assert all(now[name][0] == now_total for name in ("thresholds", "hist", "top")), kernel


def test_the_scratch_offsets(exe):
    got = run(exe, [("words",) + s for s in SHAPES])[2]
    for (R, L, batch), (planes, partial, mean, cls, q, words) in zip(SHAPES, got):
        W, lpad, tiles = (R + 63) // 64, (L + 63) // 64 * 64, (L + 31) // 32
        assert planes == 0 and partial == batch * 5 * W * lpad and mean == partial + batch * tiles * lpad
        assert cls == mean + batch * (L + 1) and q == cls + (R * L + 7) // 8 and words == q + (R + 255) // 256 * 256 // 2
        assert q == batch * (5 * W * lpad + tiles * lpad + L + 1) + (R * L + 7) // 8       # what the unweighted null's scratch is


def cases():
    """(rows, weights, statistic, minspan, K, seed): around the word, the chunk and the tile, every statistic, every seed."""
    out = []
    for n, (R, L) in enumerate(((1, 5), (63, 2), (64, 9), (65, 33), (257, 12), (9, 1), (30, 40))):
        rows = random_rows(100 * R + L, R, L, "ACGU-" if n % 2 else "ACGUacgutT-.~N&")
        out.append((rows, random_weights(100 * R + L, R), STATISTICS[n % 3], (4, 1, 0)[n % 3], 2 if R > 100 else 3, SEEDS[n % len(SEEDS)]))
    return out


def thresholds_for(rows, weights, statistic, minspan):
    """Sorted distinct observed S of the reference (what the entry bins against), with both ends and a zero among them."""
    ref = WeightedReference(rows, weights)
    values = {ref.S[statistic][vw] for vw in scope(len(rows[0]), minspan)} | {0.0, -1.0, 1e300}
    return sorted(values)


def commands():
    return [("null", rows, weights, s, minspan, K, seed, thresholds_for(rows, weights, s, minspan)) for rows, weights, s, minspan, K, seed in cases()]


def test_the_shuffled_weighted_cells_against_the_reference(exe):
    cmds = commands()
    got = run(exe, cmds)[2]
    seen = 0
    for (_, rows, weights, statistic, minspan, K, seed, thr), (status, samples) in zip(cmds, got):
        R, L = len(rows), len(rows[0])
        cells = scope(L, minspan)
        assert status == 0 and len(samples) == K
        for k, (recs, hist, most) in enumerate(samples):
            ref = WeightedReference(shuffled(rows, k, seed), weights)       # row r of the shuffled rows keeps weights[r]
            assert [(v, w) for v, w, _, _ in recs] == cells, (R, L, k)
            for v, w, Q, S in recs:
                assert Q == ref.n[(v, w)], (R, L, k, v, w)
                assert abs(S - ref.S[statistic][(v, w)]) <= BOUND * ref.scale[statistic][(v, w)], (R, L, k, v, w)
            values = [S for _, _, _, S in recs]
            exp = [0] * (len(thr) + 1)
            for S in values:
                exp[bisect.bisect_right(thr, S)] += 1
            assert hist == exp and sum(hist) == len(cells), (R, L, k)
            assert most == max(values, default=float("-inf")), (R, L, k)
            seen += len(recs)
        if R > 1 and L > 1:                                                   # the samples differ: the shuffle moved something
            assert samples[0][0] != samples[1][0], (R, L)
    assert seen > 3000


def test_a_bad_weight_is_status_3_and_counts_as_nothing(exe):
    rows = random_rows(5, 6, 8, "ACGU")
    for bad in (float("nan"), float("inf"), -2.0 ** -30, 2048.0000000000005):
        weights = [1.0, bad, 0.5, 1.0, 1.0, 1.0]
        (status, samples), = run(exe, [("null", rows, weights, "gt", 1, 1, 3, [])])[2]
        assert status == 3 and all(sum(Q) == (4 << 20) + (1 << 19) for _, _, Q, _ in samples[0][0]), bad


def test_the_harness_is_clean_under_the_sanitizers(exe):
    """The same commands through a build with -fsanitize=address,undefined, run as a stand-alone program: the same output, bit
    for bit, and no report."""
    san = _build("covar_wstat_null_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    text = text_of(commands() + [("words",) + s for s in SHAPES])
    plain = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    checked = subprocess.run([san], input=text, capture_output=True, text=True)
    assert checked.returncode == 0 and not checked.stderr, checked.stderr[-2000:]
    assert checked.stdout == plain.stdout and len(plain.stdout) > 10000
