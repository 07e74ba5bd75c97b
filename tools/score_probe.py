#!/usr/bin/env python3
"""Score() on the device against the host loop on the same rows: K random valid structures for each of N random records
(a known structure and reactivities each), scored by Score (a padded CUDA tensor of partners) and by core.ReferenceScores +
align.Metrics per row.  Prints both times and whether the results are equal.

Usage:  python tools/score_probe.py N K [length]
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from squarna_amd import Score
from squarna_amd.align import Metrics
from squarna_amd.core import ReferenceScores
from squarna_amd.dbn import PairsToDBN

N, K = int(sys.argv[1]), int(sys.argv[2])
n = int(sys.argv[3]) if len(sys.argv) > 3 else 120
rng = np.random.default_rng(1)


def random_row():
    row = np.full(n, -1, np.int32)
    for _ in range(int(rng.integers(1, 6))):
        a, b, ln = int(rng.integers(0, n - 1)), int(rng.integers(1, n)), int(rng.integers(2, 8))
        for q in range(ln):
            v, w = a + q, b - q
            if v < w and row[v] < 0 and row[w] < 0:
                row[v], row[w] = w, v
    return row


def dbn(row):
    return PairsToDBN([(i, int(p)) for i, p in enumerate(row) if p > i], n)


seqs = [''.join(rng.choice(list("ACGU"), n)) for _ in range(N)]
reacts = [[float(x) for x in rng.random(n).round(3)] for _ in range(N)]
rows = np.stack([np.stack([random_row() for _ in range(K)]) for _ in range(N)])
known = [dbn(random_row()) for _ in range(N)]
records = [(">r%d" % r, seqs[r], reacts[r], None, known[r]) for r in range(N)]
text = [[dbn(rows[r, k]) for k in range(K)] for r in range(N)]        # (the host loop's input, formed outside its timing)

dev = torch.from_numpy(rows).cuda()
Score(records=records[:1], structures=dev[:1])                        # (loads the library)
times = []
for _ in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = Score(records=records, structures=dev)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
# where the call's time goes: the per-record preparation on the host (ScoreRecord, the rows' offsets) and the engine's part
# (one upload, both launches, the wait for the number of stems), each timed alone
from squarna_amd.engine import get_engine
from squarna_amd.score import ScoreRecord, _partner_rows
prep, dev_part = [], []
for _ in range(3):
    t0 = time.perf_counter()
    recs = [ScoreRecord(rec[0], rec[1], rec[2], rec[4]) for rec in records]
    partner, row_start, row_rec, _ = _partner_rows(dev, None, recs, True)
    prep.append(time.perf_counter() - t0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    get_engine().score_tensors(recs, partner, row_start, row_rec)
    torch.cuda.synchronize()
    dev_part.append(time.perf_counter() - t0)
t0 = time.perf_counter()
want_s = [ReferenceScores(seqs[r], text[r][k], reacts[r]) for r in range(N) for k in range(K)]
want_m = [Metrics(known[r], text[r][k]) for r in range(N) for k in range(K)]
t_host = time.perf_counter() - t0
equal = res.scores.cpu().tolist() == [list(s) for s in want_s] and res.metrics.cpu().tolist() == [[float(x) for x in m] for m in want_m]
print("score_probe N=%d K=%d length=%d: Score on the device %.2f ms (best of 3; %s; of which host preparation of the records %.2f ms, "
      "upload + kernels + stem count %.2f ms, each best of 3), host loop %.1f ms, equal: %s, rows handed back to the host: %d"
      % (N, K, n, min(times) * 1e3, res.source, min(prep) * 1e3, min(dev_part) * 1e3, t_host * 1e3, equal, res.recomputed), flush=True)
