#!/usr/bin/env python3
"""BASELINE config 5 as data: FoldAlignment(step3='u') against Predict(alignment=True, write_to=<null sink>) on the synthetic
NSEQ x NCOL alignment of a5000_full.py, alternating, the median of REPS runs each; then one FoldAlignment with every engine
call timed (a synchronize around each: the split, not the total).
usage: a5000_fold_align.py [NSEQ] [NCOL] [REPS]"""
import os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import scale_soak as S
from squarna_amd import FoldAlignment, Predict, engine as E

nseq = int(sys.argv[1]) if len(sys.argv) > 1 else 512
ncol = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5


class NullSink:
    def write(self, text):
        return len(text)


class TimedEngine(E.HipEngine):
    """Every engine call FoldAlignment makes, bracketed by a device synchronize."""
    spent = {}

    def _timed(name):
        def call(self, *a, **kw):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = getattr(E.HipEngine, name)(self, *a, **kw)
            torch.cuda.synchronize()
            self.spent[name] = self.spent.get(name, 0.0) + time.perf_counter() - t0
            return out
        return call
    stem_matrix, matrix_select, first_fit = _timed("stem_matrix"), _timed("matrix_select"), _timed("first_fit")
    fold_tensors, align_pair_count = _timed("fold_tensors"), _timed("align_pair_count")


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


rng = random.Random(5000)
with tempfile.NamedTemporaryFile("w", suffix=".afa", delete=False) as f:
    f.write(S.msa(rng, nseq, ncol))
    path = f.name
try:
    timed(lambda: Predict(inputfile=path, alignment=True, step3="u", write_to=NullSink()))      # warm-up of both
    _, res = timed(lambda: FoldAlignment(inputfile=path, step3="u"))
    t_fold, t_pred = [], []
    for rep in range(reps):
        t_fold.append(timed(lambda: FoldAlignment(inputfile=path, step3="u"))[0])
        t_pred.append(timed(lambda: Predict(inputfile=path, alignment=True, step3="u", write_to=NullSink()))[0])
    print("%d x %d alignment, step3=u, median of %d alternating runs: FoldAlignment %.3f s (%s), Predict(alignment=True) %.3f s (%s)" % (
        nseq, ncol, reps, statistics.median(t_fold), " ".join("%.3f" % t for t in t_fold), statistics.median(t_pred),
        " ".join("%.3f" % t for t in t_pred)), flush=True)
    print("first-fit rounds (iteration 1, iteration 2, consensus): %s; distinct column pairs %d; pairs of steps 1-3: %s; source %s / rows %s" % (
        list(res.first_fit_rounds), int(res.pair_count.numel()), [len(res.pairs(k)) for k in (1, 2, 3)], res.source, res.rows.source), flush=True)
    with E.use_engine(TimedEngine()) as eng:
        total, _ = timed(lambda: FoldAlignment(inputfile=path, step3="u"))
    sp = eng.spent
    print("one run with a synchronize around every engine call: %.3f s; %s; rest (parsing, device sorts, O(L) host work) %.3f s" % (
        total, ", ".join("%s %.3f" % (k, sp[k]) for k in ("stem_matrix", "matrix_select", "first_fit", "fold_tensors", "align_pair_count")),
        total - sum(sp.values())), flush=True)
    print("peak device memory %.1f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
finally:
    os.unlink(path)
