"""Shared checks of the pairing predicate "may position i pair with j" (the reference's bpboolmatrix, SQRNdbnseq.py:286-304)
as the library's bit-matrix kernels state it (CPU: tests/test_bits_checks.py, tests/test_oracle_golden.py; GPU:
tests/test_hip_bitmatrix.py, tests/test_hip_interchain.py).

The library returns no bit matrix, so the predicate is read back through AnnotateStems: with minlen = 1, minscore = -1e9 and
the empty structure it lists every true cell of the diagonals it visits exactly once, as maximal runs, so its (i, j, len)
stems ARE the matrix on those diagonals (`cells_of(stems) == bool & visited(n)`; tests/test_bits_checks.py asserts this of
the oracle for every record below).  A record's bracket restraints clear the rows and columns of their positions before the
scan (:437-443); `expected` returns the matrix after that step, the one the stems spell out.

RECORDS are fixed by their seed: lengths on both sides of the 32-row words and the 256-diagonal tiles of
sq_bits_direct_kernel, chain separators at the ends, doubled and on word boundaries, restraint lines with every symbol,
reactivities, all capital letters; BIG is the 4,097-nt record of the fill kernel's generic path and the direct kernel's grid
stride.  WEIGHTS are two pair tables with different sets of pairs, so that every record owns two bit matrices.

`python -m tests.bits_checks nomasks` is the child process of the GPU test of SQ_BITS_NOMASKS (a process-wide switch)."""
import functools
import json
import os
import random
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5                       # tests/test_hip_parity.py: TOL, applied as in its close_stems

#: a negative GU weight (runs whose pieces outscore them) / no GU, purine-pyrimidine and N-N pairs instead
WEIGHTS = ({"GC": 3.25, "AU": 1.25, "GU": -1.25}, {"GC": 3.0, "AU": 2.0, "RY": 1.0, "NN": 0.5})
ALL = dict(minlen=1, minbpscore=-1e9)        # every true cell of the visited diagonals comes back
BIG_SETTINGS = dict(minlen=3, minbpscore=4.5)  # (mk_pset's default threshold) stems against stems


def mk_psets(minlen, minbpscore):
    from tests.test_hip_parity import mk_pset
    return [mk_pset(w, minlen, minbpscore) for w in WEIGHTS]


# ---- the matrix and its diagonals -------------------------------------------------------------------------------------------
def visited(n):
    """The cells AnnotateStems visits: i < j on the diagonals 4 <= i + j <= 2n - 6 (SQRNdbnseq.py:456-457, :486)."""
    i, j = np.indices((n, n))
    return (i < j) & (i + j >= 4) & (i + j <= 2 * n - 6)


def cells_of(stems, n):
    """The bool matrix spelled out by (i, j, len, ...) stems; no cell may come twice."""
    m = np.zeros((n, n), bool)
    for st in stems:
        i, j, ln = int(st[0]), int(st[1]), int(st[2])
        k = np.arange(ln)
        assert ln >= 1 and 0 <= i and j < n and i + ln - 1 < j - ln + 1, (st, n)
        assert not m[i + k, j - k].any(), ("cell listed twice", st)
        m[i + k, j - k] = True
    return m


def short_form(record):
    """(sequence, reactivities, restraint line) as SQRNdbnseq prepares them (:1004-1023; the records have no gap column)."""
    seq, reacts, restraints = record
    seq = seq.upper().replace("T", "U")
    return seq, list(reacts) if reacts else [0.5] * len(seq), restraints or "." * len(seq)


@functools.lru_cache(maxsize=None)
def _expected(record, which, interchainonly, minlen, minbpscore):
    from oracle import sqrn_oracle as O
    seq, reacts, restraints = short_form(record)
    rbps, rxs, rl, rr = O.ParseRestraints(restraints)
    b, s = O.BPMatrix(seq, WEIGHTS[which], rxs, rl, rr, interchainonly, reacts=reacts)
    stems = O.AnnotateStems(b, s, rbps, [], minlen, minbpscore)
    m = b != 0
    for v, w in rbps:                                                # :437-443
        keep = m[v, w]
        m[v, :] = m[:, v] = m[w, :] = m[:, w] = False
        m[v, w] = keep
    m.setflags(write=False)
    return m, stems


def expected(record, which, interchainonly, minlen=1, minbpscore=-1e9):
    """(bool matrix as AnnotateStems scans it, [(i, j, len, bpscore)] in the reference's emission order) of `record` under
    WEIGHTS[which], from the oracle; computed once per argument list and shared (the matrix is read-only)."""
    return _expected(record, which, bool(interchainonly), minlen, minbpscore)


# ---- the records ---------------------------------------------------------------------------------------------------------
def _put(seq, at, seps="&;"):
    seq = list(seq)
    for k, p in enumerate(at):
        seq[p] = seps[k % len(seps)]
    return "".join(seq)


def _restraint_line(rng, seq):
    """Every symbol ParseRestraints knows -- '_' '+' (unpaired), '/' (no partner to the left), '\\' (none to the right) and two
    bracket pairs -- on letters only."""
    n = len(seq)
    line = ["."] * n
    free = [p for p in range(n) if seq[p] not in "&;"]
    rng.shuffle(free)
    marks = "_+/\\" * max(2, n // 40)
    for ch, p in zip(marks, free):
        line[p] = ch
    rest = sorted(free[len(marks):])
    a, b, c, d = rest[len(rest) // 8], rest[len(rest) // 2], rest[len(rest) // 3], rest[-len(rest) // 6]
    line[a], line[b], line[c], line[d] = "(", ")", "[", "]"            # a < c < b < d: the two pairs cross
    assert a < c < b < d
    return "".join(line)


def _records():
    rng = random.Random(20261020)
    rnd = lambda n, alphabet="ACGUN": "".join(rng.choice(alphabet) for _ in range(n))      # noqa: E731
    none, low, high, ends, doubled, word, words = "none", "1|2", "n-3|n-2", "first+last", "doubled", "31|32|33", "63+64"
    plan = [(5, low, [1]), (6, high, [3]), (31, none, []), (32, ends, [0, 31]), (33, doubled, [16, 17]), (64, word, [32]),
            (65, words, [63, 64]), (127, high, [124]), (128, low, [2]), (129, word, [33]), (160, words, [63, 64]),
            (255, ends, [0, 254]), (256, doubled, [127, 128]), (257, none, []), (300, word, [31])]
    names, recs, places = [], [], []
    for n, place, at in plan:
        names.append("%d-%s" % (n, place)), recs.append((_put(rnd(n), at, ";&" if place == doubled else "&;"), None, None))
        places.append((place, at))
    for n, at in ((129, [64]), (257, [1, 255]), (300, [32, 150])):      # restraint lines
        seq = _put(rnd(n), at)
        names.append("%d-restraints" % n), recs.append((seq, None, _restraint_line(rng, seq)))
    for n, at in ((65, [32]), (160, []), (300, [128, 129])):            # reactivities other than 0.5
        names.append("%d-reacts" % n), recs.append((_put(rnd(n), at), tuple(round(rng.random(), 3) for _ in range(n)), None))
    names.append("200-letters")                                         # all capital letters: widens the mask kernel's table
    recs.append((_put("ABCDEFGHIJKLMNOPQRSTUVWXYZ" + rnd(174, "ABCDEFGHIJKLMNOPQRSTUVWXYZ"), [70, 96]), None, None))
    big = (_put(rnd(4097), [1000, 4064]), None, None)
    return names, recs, places, big


NAMES, RECORDS, PLACEMENTS, BIG = _records()
#: the records whose interchain stems tests/golden/interchain.json holds from the reference itself (under WEIGHTS[0])
GOLDEN_RECORDS = ("33-doubled", "129-31|32|33", "257-restraints", "300-31|32|33")


def tiles_of(n):
    """(word-rows, 256-diagonal tiles per word-row) of an n-nt job's bit matrix: nw and ceil(bpitch / 256) as sq_batch.hip lays
    it out (bits_nw, bits_pitch: 2n rounded up to 64, plus 64)."""
    bpitch = (2 * n + 63) // 64 * 64 + 64
    return (n + 31) // 32, (bpitch + 255) // 256


def load_golden():
    with open(os.path.join(GOLDEN, "interchain.json")) as f:
        return json.load(f)


# ---- the comparison of one batch (GPU) -------------------------------------------------------------------------------------
def same_stems(got, exp, what):
    """(i, j, len) exactly and in order, bpscore within test_hip_parity's bar; `got` is one structured array of
    Batch.optimal(as_array=True).  A difference is reported by its first stem, not by the whole lists."""
    from tests.test_hip_parity import close_stems
    g = list(zip(got["i"].tolist(), got["j"].tolist(), got["len"].tolist(), got["bpscore"].tolist()))
    for k, (a, b) in enumerate(zip(g, exp)):
        assert a[:3] == tuple(b[:3]) and abs(a[3] - b[3]) <= TOL * max(1.0, abs(b[3])), (what, "stem", k, a, b, len(g), len(exp))
    assert len(g) == len(exp), (what, "stems", len(g), len(exp), (g + [None])[len(exp)] if len(g) > len(exp) else exp[len(g)])
    close_stems(g, [tuple(e) for e in exp], what)


def check_batch(records, names, settings, interchainonly=False, fp32=False, fill=False, cells=True, golden=None):
    """One batch of `records` under the two paramsets of WEIGHTS (job = 2 * record + paramset): AnnotateStems of the empty
    structure of every job (Batch.optimal, mode 1) against `expected`, and the cells of the stems against the matrix.
    fill: sq_bpmatrix_fill first (the fp32 matrix; the bit words then come from it, or with SQ_BITS_DIRECT from the inputs).
    golden: {name: [[i, j, len, score]]} of the reference under WEIGHTS[0] with the chain test.  Returns the number of jobs."""
    from squarna_amd.engine import Batch, Prepared
    psets = mk_psets(**settings)
    preps = [Prepared(seq, list(reacts) if reacts else None, restraints) for seq, reacts, restraints in records]
    with Batch(preps, [psets] * len(preps), interchainonly=interchainonly, fp32=fp32) as b:
        njobs = b.njobs
        assert njobs == 2 * len(records) and b.job_seq.tolist() == [k // 2 for k in range(njobs)]
        if fill:
            b.fill()
        got = b.optimal(list(range(njobs)), [[]] * njobs, mode=1, as_array=True)
    for job in range(njobs):
        rec, which = records[job // 2], job % 2
        what = (names[job // 2], "weights %d" % which, "chain test" if interchainonly else "")
        m, stems = expected(rec, which, interchainonly, settings["minlen"], settings["minbpscore"])
        same_stems(got[job], stems, what)
        if cells:
            n = m.shape[0]
            assert np.array_equal(cells_of(zip(got[job]["i"].tolist(), got[job]["j"].tolist(), got[job]["len"].tolist()), n),
                                  m & visited(n)), what
        if golden and interchainonly and which == 0 and names[job // 2] in golden:
            same_stems(got[job], golden[names[job // 2]], what + ("reference",))
    return njobs


def check_route(interchainonly=False, fp32=False, fill=False, big=False, golden=None):
    """The route's batches: every record of RECORDS in one batch and in a second one reversed (mixed n, bits_off and nw per
    job), or BIG in a batch of its own (big=True; big="mixed": four of the records behind it)."""
    if big == "mixed":                       # ... with shorter records beside it: the fill kernel picks its path per job
        names = ["4097", "300-31|32|33", "160-reacts", "129-restraints", "33-doubled"]
        return check_batch([BIG] + [RECORDS[NAMES.index(x)] for x in names[1:]], names, BIG_SETTINGS, interchainonly, fp32, fill, cells=False)
    if big:
        return check_batch([BIG], ["4097"], BIG_SETTINGS, interchainonly, fp32, fill, cells=False)
    jobs = check_batch(RECORDS, NAMES, ALL, interchainonly, fp32, fill, golden=golden)
    return jobs + check_batch(RECORDS[::-1], NAMES[::-1], ALL, interchainonly, fp32, fill, golden=golden)


if __name__ == "__main__":
    assert sys.argv[1:] == ["nomasks"] and os.environ.get("SQ_BITS_NOMASKS") == "1", sys.argv
    print("%d jobs, 0 mismatches" % (check_route() + check_route(big=True)), flush=True)
