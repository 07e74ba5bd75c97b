"""GPU: the launched kernels whose dynamic LDS sq_launch_lds.h lays out -- state, scan, score, select and chain -- on batches whose
jobs are SHORTER than the sequence the launch sized its LDS for, with the staging limits moved down to small records, and at the
length where the scoring launch first asks for more than 64 KB.  Width-1 pools under `fastest`; all comparisons are exact (packed
records byte for byte; against the oracle the scores within test_hip_parity's bar)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import launch_lds_checks as C
from tests.test_hip_parity import _same_fold
from tests.test_launch_lds_host import NR_LIM, SCORE_CROSSINGS, STATE_LIM, score_decisions, score_ints

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: twice the 1.7 s the same route -- the four batches of launch_lds_checks.staging_batches() on the launched rounds, the library's
#: imports and the process's first GPU call included -- took in-process on an MI355X (the child itself, interpreter start
#: included, took 2.1 s)
CHILD_TIMEOUT = 3.4


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("SQ_NO_ROUNDS", "SQ_NO_CHAIN", "SQ_SCORE_NR_LIM", "SQ_SCORE_STATE_LIM"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def oracle():
    """the oracle's folds of the records, once for the module: {(seq, reacts as a tuple): [consensus, structures]}"""
    from oracle import sqrn_oracle as O
    ps = C.psets()
    out = {}
    for s, r in C.records():
        e = O.SQRNdbnseq(s, r, None, None, ps, poollim=1)
        out[(s, tuple(r) if r is not None else None)] = [e[0], [[d, list(sc), list(p)] for d, sc, p in e[1]]]
    return out


def same(got, exp, tag):
    """test_hip_parity's comparison of a fold with the oracle's; neither side carries metrics of a known structure here"""
    _same_fold(list(got[:2]) + [[], []], list(exp[:2]) + [[], []], tag)


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_mixed_lengths_on_the_three_routes(order, oracle):
    """5 - 300 nt in one batch: every launch sizes its LDS for 300 nt and carves it for jobs of 5 nt on.  The persistent round
    kernel (the default), the launched chained rounds (SQ_NO_ROUNDS: state, scan, score, chain) and the host-driven rounds
    (SQ_NO_CHAIN: state, scan, score, select) give the same packed records, and the oracle's folds."""
    recs = C.records() if order == "forward" else C.records()[::-1]
    assert sorted({len(s) for s, _ in recs}) == sorted(C.LENGTHS) and len(recs) == 3 * len(C.LENGTHS)
    (pd, rd, dd, hd), (pl, rl, dl, hl), (ph, rh, dh, hh) = (C.fold(recs, route) for route in ("default", "launched", "hosted"))
    assert (dd, dl, dh) == (1, 1, 0) and (hd & 4) and not (hl & 4) and not (hh & 4), (dd, dl, dh, hd, hl, hh)
    for k, (s, r) in enumerate(recs):
        assert pd[k] == pl[k] == ph[k], (order, k, len(s), rd[k][:2], rl[k][:2], rh[k][:2])
        same(C.plain(rd[k]), oracle[(s, tuple(r) if r is not None else None)], (order, k, len(s)))


def test_staging_limits_moved_down_to_small_records(oracle):
    """SQ_SCORE_NR_LIM=64, SQ_SCORE_STATE_LIM=1 (read once per process: a child): on the launched rounds the batch's launches stage
    no reactivities (300 nt > 64) and no state copies -- the layouts with lds_nr = lds_ns = 0 beside lds_n = 300; a second
    batch of the records up to 64 nt stages the reactivities of the 64-nt record, one up to 65 nt does not.  The oracle's folds."""
    env = dict(os.environ, SQ_SCORE_NR_LIM="64", SQ_SCORE_STATE_LIM="1")
    r = subprocess.run([sys.executable, "-m", "tests.launch_lds_checks", "staging"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = json.loads(r.stdout)
    for name, recs in C.staging_batches():
        got = out[name]
        assert got["driver"] == 1 and not (got["paths"] & 4), (name, got["driver"], got["paths"])
        assert len(got["results"]) == len(recs)
        for k, (s, rc) in enumerate(recs):
            same(got["results"][k], oracle[(s, tuple(rc) if rc is not None else None)], (name, k, len(s)))


@pytest.mark.parametrize("n", [SCORE_CROSSINGS[0], SCORE_CROSSINGS[2]])
def test_score_launch_beyond_64_kb(n):
    """One float-reactivity record of a length at which the mode-0 scoring launch with room for SQ_LDS_STRANDS = 1,024 strands asks
    for more than 64 KB of dynamic LDS (tests/test_launch_lds_host.py: from 1,277 nt with the state copies staged, from 2,125 nt
    without).  Only the host-driven rounds (SQ_NO_CHAIN) give every structure that room; the chained rounds (SQ_NO_ROUNDS) size
    it by the batch's longest possible stem list -- 322 and 534 strands here, launches of 58,532 and 60,652 bytes -- and stay
    below.  So the host-driven fold is the launch under test; the chained rounds and the persistent round kernel are folded
    beside it.  The same packed bytes on all three and no error.  The routes are compared with each other, not with the
    oracle: the oracle needs far longer at this length (0.5 s and 1.8 s for the two records, against the folds' milliseconds)."""
    from squarna_amd import _lib
    minlen = min(int(p["minlen"]) for p in C.psets())
    decided = score_decisions(n, True, 0, NR_LIM, STATE_LIM)
    # (cell table: 32 doubles, a batch's smallest; 512 threads: a sequence beyond 400 nt outside the pools)
    assert score_ints(*decided, 32, 512, 0, 1024)[3] > 64 * 1024                               # the host-driven launch
    assert score_ints(*decided, 32, 512, 0, min(1024, 2 * (n // (2 * minlen) + 1) + 2))[3] <= 64 * 1024   # the chained one
    rng = np.random.default_rng(n)
    recs = [("".join(rng.choice(list("ACGU"), n)), [float(x) for x in rng.random(n)])]
    L = _lib.load()
    before = L.sq_last_error()
    # (Batch.fold raises on any status but 0: three folds that return are three folds that reported success)
    (ph, rh, dh, hh), (pl, rl, dl, hl), (pd, rd, dd, hd) = (C.fold(recs, route) for route in ("hosted", "launched", "default"))
    assert (dh, dl, dd) == (0, 1, 1) and not (hh & 4) and not (hl & 4) and (hd & 4), (dh, dl, dd, hh, hl, hd)
    assert ph == pl == pd and len(ph[0]) > 0 and rh[0][1], (n, rh[0][:2], rl[0][:2], rd[0][:2])
    assert L.sq_last_error() == before          # (the text is per thread and never cleared: empty in a process without earlier errors)
