"""The weighted covariation-statistics logic (squarna_amd/csrc/sq_covar_wstat.h, the logic of sq_covariation_wstat_scan and
sq_covariation_wstat_pairs), compiled for the host and run as one thread -- the weights quantised, the counters of a cell
chunk by chunk and word by word, pass 1 with the kernels' order of sums, pass 2 -- against the plain-Python reference of
tests/covariation_wstat_checks.py, and against the unweighted header's harness for integer weights.  Q is compared exactly, S,
C and the means under the float bound derived there.  The LDS layout function is checked here too."""
import os
import random
import subprocess

import pytest

from tests.covariation_checks import random_rows
from tests.covariation_stat_checks import BOUND, CORRECTIONS, DEFAULTS, EVERY_CELL, STATISTICS, check_means, check_records
from tests.covariation_wstat_checks import ONE, WEIGHTS, quantise, random_weights, reference

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "covar_wstat_host.cpp")
REGIONS = ("planes", "q", "bins", "S", "row", "col", "flat", "raw", "em")
KERNELS = ("sums", "scan", "pairs")


def _build(name, flags, src=SRC):
    exe = os.path.join(HERE, "native", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("covar_wstat_host", ["-O2"])


@pytest.fixture(scope="module")
def exe_san():
    return _build("covar_wstat_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def text_of(cases):
    lines = [str(len(cases))]
    for rows, weights, statistic, correction, thr in cases:
        L = len(rows[0])
        assert all(len(r) == L for r in rows) and not any(ch.isspace() for r in rows for ch in r) and len(weights) == len(rows)
        floor = "-inf" if thr["min_stat"] is None else float(thr["min_stat"]).hex()
        lines.append("%d %d %d %d %d %s %s" % (len(rows), L, STATISTICS.index(statistic), CORRECTIONS.index(correction), thr["minspan"],
                                               float(thr["min_rows"]).hex(), floor))
        lines.append(" ".join(float(w).hex() if w == w and abs(w) != float("inf") else repr(float(w)) for w in weights))
        lines += rows
    return "\n".join(lines) + "\n"


def run(exe, cases):
    """((TILE, WORD_CHUNK, MAX_BLOCKS, ONE, MAX_ROWS), {kernel: (total, {region: (offset, size)})}, per case (status, q, means,
    [(v, w, Q, S, C)] sorted by (v, w)))."""
    res = subprocess.run([exe], input=text_of(cases), capture_output=True, text=True, check=True)
    out = res.stdout.strip("\n").split("\n")
    assert len(out) == 3 * len(cases) + 4
    layouts = {}
    for kernel, line in zip(KERNELS, out[1:4]):
        words = [int(x) for x in line.split()]
        assert len(words) == 1 + 2 * len(REGIONS)
        layouts[kernel] = (words[0], {name: (words[1 + 2 * k], words[2 + 2 * k]) for k, name in enumerate(REGIONS)})
    got = []
    for k, (rows, _, _, _, _) in enumerate(cases):
        L = len(rows[0])
        first = [int(x) for x in out[4 + 3 * k].split()]
        means = [float.fromhex(x) for x in out[5 + 3 * k].split()]
        words = out[6 + 3 * k].split()
        count = int(words[0])
        assert len(first) == 1 + len(rows) and len(means) == L + 1 and len(words) == 1 + 19 * count
        recs = [words[1 + 19 * j:20 + 19 * j] for j in range(count)]
        assert len({r[0] for r in recs}) == count                            # no cell twice
        got.append((first[0], first[1:], means,
                    sorted((int(r[0]) // L, int(r[0]) % L, [int(x) for x in r[1:17]], float.fromhex(r[17]), float.fromhex(r[18])) for r in recs)))
    return tuple(map(int, out[0].split())), layouts, got


def constants(exe):
    return run(exe, [])[0]


def check(exe, inputs, thresholds=(DEFAULTS, EVERY_CELL)):
    """Every statistic and correction with nothing thresholded, and the defaults, for every (rows, weights)."""
    cases = [(rows, weights, s, c, thr) for rows, weights in inputs for s in STATISTICS for c in CORRECTIONS for thr in thresholds
             if thr is EVERY_CELL or (s, c) == ("gt", "apc")]
    got = run(exe, cases)[2]
    for (rows, weights, s, c, thr), (status, q, means, recs) in zip(cases, got):
        ref = reference(rows, weights)
        what = (len(rows), len(rows[0]), s, c, thr)
        assert status == 0 and q == ref.q, what
        check_records(ref, s, c, [r[:2] for r in recs], [r[2] for r in recs], [r[3] for r in recs], [r[4] for r in recs],
                      ref.select(s, c, **thr), what)
        if c is None:
            assert means == [0.0] * (ref.L + 1) and all(r[3] == r[4] for r in recs)
        else:
            check_means(ref, s, means[:-1], means[-1], what)


def test_constants_are_the_python_mirrors(exe):
    from squarna_amd import covariation_statistics as cs, device_calls as dc
    assert constants(exe) == (dc.COVAR_STAT_TILE, dc.COVAR_STAT_WORD_CHUNK, dc.COVAR_STAT_MAX_BLOCKS, dc.COVAR_WSTAT_ONE, dc.COVAR_WSTAT_MAX_ROWS)
    assert (cs.WEIGHT_ONE, cs.MAX_WEIGHT, cs.MAX_WEIGHTED_ROWS) == (dc.COVAR_WSTAT_ONE, dc.COVAR_WSTAT_MAX_WEIGHT, dc.COVAR_WSTAT_MAX_ROWS)
    assert dc.COVAR_WSTAT_ONE == ONE == 1 << 20 and max(WEIGHTS) == dc.COVAR_WSTAT_MAX_WEIGHT and dc.COVAR_WSTAT_MAX_ROWS == 1 << 22


def test_the_lds_layout_places_disjoint_aligned_regions_inside_the_total(exe):
    layouts = run(exe, [])[1]
    have = {"sums": {"planes", "q", "bins", "S", "row", "col"}, "scan": {"planes", "q", "bins", "flat", "raw", "em"}, "pairs": {"bins"}}
    for kernel, (total, regions) in layouts.items():
        assert {name for name, (_, size) in regions.items() if size} == have[kernel], kernel
        spans = sorted((at, at + size, name) for name, (at, size) in regions.items() if size)
        assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (kernel, spans)      # disjoint
        assert all(at % 8 == 0 and at % 16 == 0 for at, _, _ in spans), (kernel, spans)
        assert all(0 <= at <= total for at, _ in regions.values()) and spans[-1][1] <= total <= 64 * 1024, (kernel, total)
    assert layouts["scan"][1]["bins"][1] == 16 * 256 * 8 and layouts["sums"][1]["q"][1] == 64 * constants(exe)[1] * 4


@pytest.mark.parametrize("R", [1, 63, 64, 65, 257])
def test_against_the_reference_around_the_word_the_chunk_and_the_tile(exe, R):
    check(exe, [(random_rows(1000 * R + L, R, L), random_weights(1000 * R + L, R)) for L in (1, 2, 31, 32, 33, 97)])


def test_quantise_rounds_ties_to_even_and_flags_what_is_no_weight(exe):
    ties = [(2 * k + 1) / (2 * ONE) for k in (0, 1, 2, 3, 1000)] + [1 / 3, 1 / 7, 2 ** -21 * 0.999, 2048 - 2 ** -21, 2048.0, 0.0, -0.0]
    rows = ["ACGU"] * len(ties)
    (status, q, _, _), = run(exe, [(rows, ties, "gt", None, EVERY_CELL)])[2]
    assert status == 0 and q == quantise(ties) and q[:5] == [0, 2, 2, 4, 1000] and q[-3:] == [1 << 31, 0, 0]
    for bad in (float("nan"), float("inf"), -float("inf"), -2.0 ** -30, 2048.0000000000005):
        weights = [1.0, bad, 0.5]
        (status, q, _, recs), = run(exe, [(["ACGU", "ACGU", "ACGU"], weights, "gt", None, EVERY_CELL)])[2]
        assert status == 3 and q == [ONE, 0, ONE // 2], bad                  # the bad weight counts as 0
        assert all(sum(Q) == ONE + ONE // 2 for _, _, Q, _, _ in recs) and len(recs) == 6


def test_integer_weights_give_the_bits_of_the_unweighted_header_on_the_repeated_rows(exe):
    """raw_w() on integer weights against SqCovarStat::raw() on the integer counts (the harness of test_covar_stat_host.py on the
    alignment with row r repeated k[r] times): the same records and means, bit for bit."""
    from tests import test_covar_stat_host as plain
    plain_exe = plain._build("covar_stat_host", ["-O2"])
    rng = random.Random(77)
    rows = random_rows(77, 65, 70)
    k = [rng.randrange(4) for _ in rows]
    repeated = [r for r, times in zip(rows, k) for _ in range(times)]
    for s in STATISTICS:
        for c in CORRECTIONS:
            for thr in (DEFAULTS, EVERY_CELL):
                (_, _, means, recs), = run(exe, [(rows, k, s, c, thr)])[2]
                (p_means, p_recs), = plain.run(plain_exe, [(repeated, s, c, thr)])[1]
                assert means == p_means and len(recs) == len(p_recs) > 0, (s, c)
                for (v, w, Q, S, C), (pv, pw, n, pS, pC) in zip(recs, p_recs):
                    assert (v, w, Q, S, C) == (pv, pw, [x * ONE for x in n], pS, pC), (s, c, v, w)


def test_a_float_min_rows_and_min_stat_select(exe):
    """min_rows lies in the middle of the widest gap of the cells' weighted rows, min_stat in the widest gap of the values of the
    cells that are left; the test first asserts, on the reference alone, that neither has a cell within reach (2^-20 of the
    rows, the float bound of the value).  Then the record set is compared exactly."""
    rows, weights = random_rows(21, 40, 45, "ACGU-", helices=3), random_weights(21, 40)
    ref = reference(rows, weights)
    N = sorted(set(ref.rows_of(v, w) for v, w in ref.n if w - v >= 4))
    _, low, high = max((b - a, a, b) for a, b in zip(N, N[1:]))
    min_rows = float((low + high) / 2)
    for s, c in (("gt", "apc"), ("mi", "asc"), ("chi", None)):
        thr, _ = ref.gap_threshold(s, c, min_rows=min_rows)
        scope, enough = ref.select(s, c, min_rows=0), ref.select(s, c, min_rows=min_rows)
        kept = ref.select(s, c, min_rows=min_rows, min_stat=thr)
        assert 0 < len(kept) < len(enough) < len(scope)
        assert all(abs(ref.rows_of(r[0], r[1]) - min_rows) > 2.0 ** -20 for r in scope)
        assert all(abs(r[4] - thr) > BOUND * (abs(r[3]) + abs(ref.term(s, c, r[0], r[1]))) for r in enough)
        (_, _, _, recs), = run(exe, [(rows, weights, s, c, dict(minspan=4, min_rows=min_rows, min_stat=thr))])[2]
        assert [r[:3] for r in recs] == [r[:3] for r in kept]


def test_the_harness_is_clean_under_the_sanitizers(exe, exe_san):
    """The same cases through a build with -fsanitize=address,undefined, run as a stand-alone program: the same output, bit
    for bit, and no report."""
    inputs = [(random_rows(65000 + L, 65, L), random_weights(65000 + L, 65)) for L in (1, 2, 33, 97)]
    text = text_of([(rows, weights, s, c, thr) for rows, weights in inputs for s in STATISTICS for c in CORRECTIONS for thr in (DEFAULTS, EVERY_CELL)])
    plain = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    checked = subprocess.run([exe_san], input=text, capture_output=True, text=True)
    assert checked.returncode == 0 and not checked.stderr, checked.stderr[-2000:]
    assert checked.stdout == plain.stdout and len(plain.stdout) > 10000
