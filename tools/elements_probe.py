#!/usr/bin/env python3
"""Elements() on the device against the host path on the same rows, timed three ways: the whole call (a CUDA tensor of
partners in, device tensors out), the two kernels alone between HIP events (everything uploaded and allocated beforehand),
and what a user did without the entry: .cpu() of the partners plus the host path.  Prints the three times and whether the
three outputs are equal.

Usage:  python tools/elements_probe.py ROWS N [WARMUP] [TIMED]
ROWS random rows of N nt (nested helices, bulges, internal loops, multiloops and up to three crossing helices), or, with
ROWS = "fold", the rows of Fold(SRtest150, nobpp) (N is ignored).
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from squarna_amd import Elements, Fold, _lib
from squarna_amd import engine as E
from squarna_amd.elements import ScoreRecord, _elements_host, _partner_rows
from tests.elements_checks import equal_results, random_row

N = int(sys.argv[2])
WARMUP = int(sys.argv[3]) if len(sys.argv) > 3 else 2
TIMED = int(sys.argv[4]) if len(sys.argv) > 4 else 5

if sys.argv[1] == "fold":
    fold = Fold(inputfile="datasets/SRtest150.fas", inputformat="qf", configfile="nobpp")
    records, structures, shape = [(n, s, None, None, None) for n, s in zip(fold.names, fold.sequences)], fold, "the rows of Fold(SRtest150, nobpp)"
else:
    ROWS = int(sys.argv[1])
    seq = ''.join(np.random.default_rng(1).choice(list("ACGU"), N))
    records = [(">r", seq, None, None, None)]
    structures = torch.from_numpy(np.stack([random_row(q, N, k=q % 4)[1] for q in range(ROWS)])[None]).cuda()
    shape = "%d random rows of %d nt" % (ROWS, N)


def best(fn, sync=True, warmup=WARMUP, timed=TIMED):
    times = []
    for k in range(warmup + timed):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        if k >= warmup:
            times.append(time.perf_counter() - t0)
    return min(times) * 1e3, out


t_call, res = best(lambda: Elements(records=records, structures=structures))

# the two kernels alone: the call's own tensors, formed once; a pass between two events on torch's current stream
recs = [ScoreRecord(rec[0], rec[1]) for rec in records]
partner, row_start, row_rec, _ = _partner_rows(structures, None, recs, True)
passes = []
LIB = _lib.load()


class _Timed:
    """The library as elements_tensors sees it, with every sq_elements_rows call between two events."""
    def __getattr__(self, name):
        return getattr(LIB, name)

    def sq_elements_rows(self, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); rc = LIB.sq_elements_rows(*args); b.record()
        passes.append((a, b))
        return rc


load = _lib.load
kern = []
for k in range(WARMUP + TIMED):
    del passes[:]
    _lib.load = lambda: _Timed()
    try:
        tables = E.get_engine().elements_tensors(recs, partner, row_start, row_rec)
    finally:
        _lib.load = load
    torch.cuda.synchronize()
    if k >= WARMUP:
        kern.append([a.elapsed_time(b) for a, b in passes])
t_levels, t_loops = (min(t[p] for t in kern) for p in (0, 1))


def host_path():
    p = partner.cpu().numpy()
    return _elements_host(recs, p, row_start, row_rec)


t_host, host = best(host_path, sync=False, warmup=0, timed=1)           # (seconds of Python: once)
from squarna_amd.elements import ElementsResult
host["row_off"] = res.row_off.cpu().numpy()
want = ElementsResult(res.names, res.sequences, {k: torch.from_numpy(v) for k, v in host.items()}, "host")
dev2 = ElementsResult(res.names, res.sequences, dict(tables, row_off=res.row_off), "device")
equal = True
try:
    equal_results(res, want)
    if not res.recomputed:
        equal_results(dev2, want)
except AssertionError as e:
    equal = "NO (%s)" % e
rows, cells, loops = len(res.status), int(res.cell_off[-1]), len(res.loops)
# what each kernel has to move per row, from the shapes (a column read again by the same wave comes from the cache): the levels
# kernel reads the partner row (4 B a column) and writes element, level, loop_of (1 + 2 + 4 B a column) and a 4-byte opener per
# loop but the exterior one; the loops kernel reads partner and level (4 + 2 B a column) and the openers, writes 24 B a loop
# and loop_of + element (4 + 1 B) for every column that is in no pair of level 1
per_row = lambda x: x / max(rows, 1)
inloop = int((res.loop_of >= 0).sum())
b_levels = per_row(11 * cells + 4 * (loops - rows) + 16 * rows)
b_loops = per_row(6 * cells + 4 * (loops - rows) + 24 * loops + 5 * inloop)
print("elements_probe %s (%d rows, %d columns, %d loops; best of %d after %d): Elements on the device %.2f ms (%s, %d rows handed back); "
      "of which the levels kernel %.3f ms and the loops kernel %.3f ms between events; .cpu() + the host path %.1f ms; equal: %s; "
      "columns per row %.1f, loops per row %.2f, bytes per row: the levels kernel %.0f, the loops kernel %.0f"
      % (shape, rows, cells, loops, TIMED, WARMUP, t_call, res.source, res.recomputed, t_levels, t_loops, t_host, equal,
         per_row(cells), per_row(loops), b_levels, b_loops), flush=True)
