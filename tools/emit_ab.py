#!/usr/bin/env python3
"""A/B of the three entries whose kernels go through the block's emission stage (sq_emit.h) between two prebuilt libraries
(tools/_libA.so, tools/_libB.so: lib_ab.sh's convention), both loaded into this one process and alternated on the same inputs:
  sq_colmatrix_select    the step-1 matrix of the 512 x 5000 alignment at its own threshold; the dense L = 2304 matrix
  sq_align_pair_count    the pair tables of that alignment's step 2; 900 dense antidiagonal records of L = 2000
  sq_window_pair_count   30,000 nt in windows of 150, step 5
Each entry between HIP events (its memsets included), buffers allocated before, two warm-up launches per library, then 7
alternating launches; the results of A and B are compared as sets.
usage: emit_ab.py"""
import ctypes as C
import os, random, statistics, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import scale_soak as S
from squarna_amd import FoldAlignment, FoldWindows, engine as E

LIBS = {v: C.CDLL(os.path.join(ROOT, "tools", "_lib%s.so" % v)) for v in "AB"}
dev = torch.device("cuda", torch.cuda.current_device())
p = lambda t: C.c_void_p(t.data_ptr())
new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
I64, I32, F64 = torch.int64, torch.int32, torch.float64


def ab(name, launch, results, n_out):
    """launch(lib, stream) enqueues the entry; results() -> (number, [result tensors]) after a synchronize."""
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    times, sets = {v: [] for v in LIBS}, {}
    for v, lib in LIBS.items():
        for _ in range(2):
            assert launch(lib, stream) == 0, name
        torch.cuda.synchronize()
    for _ in range(7):
        for v, lib in LIBS.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert launch(lib, stream) == 0
            e1.record()
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1e3)
            if v not in sets:
                n, cols = results()
                assert n <= int(cols[0].numel()), (name, n)
                order = torch.argsort(cols[0][:n])
                sets[v] = (n, [c[:n][order].clone() for c in cols])
    same = sets["A"][0] == sets["B"][0] and all(torch.equal(a, b) for a, b in zip(sets["A"][1], sets["B"][1]))
    assert sets["A"][0] == n_out or n_out is None, (sets["A"][0], n_out)
    for v in LIBS:
        t = times[v]
        print("%-44s %s: median %8.1f us, min %8.1f, max %8.1f, spread %7.1f (%s)" % (
            name, v, statistics.median(t), min(t), max(t), max(t) - min(t), " ".join("%.1f" % x for x in t)), flush=True)
    print("%-44s records %d, A and B equal as sets: %s; median B - median A = %+.1f us" % (
        name, sets["A"][0], same, statistics.median(times["B"]) - statistics.median(times["A"])), flush=True)
    assert same


def select(name, matrix, thr, n_out=None):
    L = int(matrix.shape[0])
    cap = n_out if n_out else 1 << 22
    idx, val, cnt = new(cap, I64), new(cap, F64), torch.zeros(1, dtype=I64, device=dev)
    for lib in LIBS.values():
        lib.sq_colmatrix_select.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    ab(name, lambda lib, st: lib.sq_colmatrix_select(p(matrix), L, float(thr), 4, p(idx), p(val), cap, p(cnt), st),
       lambda: (int(cnt.item()), [idx, val]), n_out)


def pair_count(name, partner, cell_off, gap_maps, L, n_out=None):
    nrec = len(gap_maps)
    col_off = np.zeros(nrec + 1, np.int32)
    np.cumsum([len(g) for g in gap_maps], out=col_off[1:])
    d_off, d_cols = E._upload_once([col_off, np.concatenate(gap_maps).astype(np.int32)], dev)
    cap = int(col_off[-1]) // 2
    for lib in LIBS.values():
        lib.sq_align_pair_count_scratch.restype = C.c_size_t
        lib.sq_align_pair_count.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p]
    nbytes = int(LIBS["A"].sq_align_pair_count_scratch(C.c_int32(L)))
    scratch, flat, count, first, out = new(nbytes // 4, I32), new(cap, I64), new(cap, I32), new(cap, I32), new(2, I64)
    ab(name, lambda lib, st: lib.sq_align_pair_count(p(partner), p(cell_off), p(d_off), p(d_cols), nrec, L, 1, p(scratch), nbytes, p(flat),
                                                     p(count), p(first), cap, p(out), st),
       lambda: (out.tolist()[0], [flat, count, first]), n_out)


class Capture(E.HipEngine):
    """The first matrix_select and the align_pair_count of a FoldAlignment call, as they were given."""
    got = {}

    def matrix_select(self, matrix, threshold, minspan=4):
        self.got.setdefault("select", (matrix.clone(), threshold))
        return E.HipEngine.matrix_select(self, matrix, threshold, minspan)

    def align_pair_count(self, partner, cell_off, gap_maps, Lcols, threshold=1):
        self.got["count"] = (partner, cell_off, gap_maps, Lcols)
        return E.HipEngine.align_pair_count(self, partner, cell_off, gap_maps, Lcols, threshold)


# ---- the 512 x 5000 alignment of the bench ----
with tempfile.NamedTemporaryFile("w", suffix=".afa", delete=False) as f:
    f.write(S.msa(random.Random(5000), 512, 5000))
    path = f.name
try:
    with E.use_engine(Capture()) as eng:
        FoldAlignment(inputfile=path, step3="u")
finally:
    os.unlink(path)
matrix, thr = eng.got["select"]
select("sq_colmatrix_select A5000 L=5000 thr %g" % thr, matrix, thr)
pair_count("sq_align_pair_count A5000 512 x 5000", *eng.got["count"])
del matrix, eng

# ---- the dense shapes of tests/test_hip_fold_align.py ----
L = 2304
m = torch.from_numpy(np.random.default_rng(2304).integers(4, 12, (L, L)).astype(np.float64)).to(dev)
select("sq_colmatrix_select dense L=2304", m, 4.0, 2646150)
L = 2000
part = np.full((900, L), -1, np.int32)
for r in range(900):
    s = L - 1 - r
    i = np.arange((s + 1) // 2)
    part[r, i], part[r, s - i] = s - i, i
pair_count("sq_align_pair_count dense 900 x 2000", torch.from_numpy(part.reshape(-1)).to(dev),
           torch.arange(901, dtype=I64, device=dev) * L, [np.arange(L, dtype=np.int32)] * 900, L, 697500)

# ---- sliding windows: 30,000 nt, window 150, step 5 ----
N = 30000
rng = random.Random(N)
seq = "".join(rng.choice("ACGU") for _ in range(N))
res = FoldWindows(records=[(">probe", seq, None, None, None)], window=150, step=5, configfile="nobpp")
w, T, P = res.windows, int(res.win_off[-1]), int(res.pair_count.numel())
starts, lens = res.starts.contiguous(), w.lengths.to(I32)
flat, small, out = new(P + 1, I64), [new(P + 1, I32) for _ in range(3)], new(2, I64)
for lib in LIBS.values():
    lib.sq_window_pair_count.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + \
                                        [C.c_int64, C.c_void_p, C.c_void_p]
ab("sq_window_pair_count 30000 nt / 150 / 5", lambda lib, st: lib.sq_window_pair_count(p(w.partner), p(w.cell_off), 0, T, p(starts), p(lens), N, p(flat),
                                                                                        p(small[0]), p(small[1]), p(small[2]), P + 1, p(out), st),
   lambda: (out.tolist()[0], [flat] + small), P)
