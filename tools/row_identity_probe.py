#!/usr/bin/env python3
"""Row identities, neighbour counts and the greedy filter of one random alignment of R rows and L columns with planted
near-duplicates (families of rows that differ from their founder in a few columns), timed three ways:
 (a) the whole RowIdentity call, sq_row_identity alone between HIP events (buffers allocated before), and each of its three
     kernels alone (sq_row_identity_phases on the buffers the whole call left);
 (b) len, neighbours and the matrices with torch ops on the device: one-hot matrix products, chunked over rows where R x R
     would not fit.  Not the filter: every row's verdict needs the verdicts before it, which no torch op expresses;
 (c) the rows downloaded and everything with numpy (float matrix products: exact at these sizes, and BLAS), the filter as a
     loop over packed bit rows (above 4096 rows: two calls, no warm-up -- a call takes seconds).
The outputs are asserted equal.  The matrices are formed when R <= 4096.  Best and median over the timed calls.
usage: row_identity_probe.py R L [THRESHOLD] [WARMUP] [TIMED]"""
import ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import RowIdentity, _lib, covariation as CV

R, L = int(sys.argv[1]), int(sys.argv[2])
threshold = float(sys.argv[3]) if len(sys.argv) > 3 else 0.8
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 3
timed = int(sys.argv[5]) if len(sys.argv) > 5 else 5
T = int(round(threshold * 10000))
matrix = R <= 4096
rng = random.Random(R * 100003 + L)
families = max(R // 12, 1)
founders = ["".join(rng.choice("ACGU-") if rng.random() < 0.97 else "N" for _ in range(L)) for _ in range(families)]
seqs = []
for r in range(R):                                                        # a family member: 0 .. 30 % of the columns redrawn
    rate = rng.random() * 0.3
    seqs.append("".join(rng.choice("ACGU-") if rng.random() < rate else ch for ch in founders[rng.randrange(families)]))
med = statistics.median
show = lambda us: "best %.1f us, median %.1f us (%s)" % (min(us), med(us), " ".join("%.1f" % t for t in us))


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


# ---- (a) the whole call
a_total = []
for k in range(warmup + timed):
    t0 = sync_time()
    res = RowIdentity(sequences=seqs, threshold=threshold, matrix=matrix)
    t = sync_time() - t0
    if k >= warmup:
        a_total.append(t)
assert res.source == "device"
print("R %d x L %d, %d families, threshold %d bp, denominator shorter, matrices %s: %d rows kept, neff %.1f, most neighbours %d; "
      "%d warm-up, %d timed calls" % (R, L, families, T, "formed" if matrix else "not formed", int(res.keep.sum()), float(res.neff()),
                                      int(res.neighbours.max()), warmup, timed), flush=True)
print("(a) RowIdentity (rows to bytes, upload, the three kernels, the result words) best %.6f s, median %.6f s" % (min(a_total), med(a_total)), flush=True)

# ---- sq_row_identity alone and its kernels alone, between HIP events with buffers allocated before
lib = _lib.load()
dev = res.device
d_rows = torch.from_numpy(np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).reshape(R, L).copy()).to(dev)
nbytes = int(lib.sq_row_identity_scratch(R, L))
new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
scratch, out = new(nbytes // 8, torch.int64), new(2, torch.int64)
d_len, d_bases, d_nb, d_keep = new(R, torch.int32), new(R, torch.int32), new(R, torch.int32), new(R, torch.uint8)
d_same, d_both = (new((R, R), torch.int32), new((R, R), torch.int32)) if matrix else (None, None)
p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
tail = (p(d_rows), R, L, 0, T, p(scratch), nbytes, p(d_len), p(d_bases), p(d_same), p(d_both), p(d_nb), p(d_keep), p(out), stream)
whole_us, phase_us = [], ([], [], [])
for k in range(warmup + timed):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    ev[0].record()
    _lib.check(lib.sq_row_identity(*tail))
    ev[1].record()
    torch.cuda.synchronize()
    for j in range(3):                                                    # (every phase finds what the whole call left)
        ev[2 + 2 * j].record()
        _lib.check(lib.sq_row_identity_phases(1 << j, *tail))
        ev[3 + 2 * j].record()
        torch.cuda.synchronize()
    if k >= warmup:
        whole_us.append(ev[0].elapsed_time(ev[1]) * 1e3)
        for j in range(3):
            phase_us[j].append(ev[2 + 2 * j].elapsed_time(ev[3 + 2 * j]) * 1e3)
for got, ref in ((d_len, res.len), (d_bases, res.bases), (d_nb, res.neighbours), (d_keep.bool(), res.keep)) + (((d_same, res.same), (d_both, res.both)) if matrix else ()):
    assert torch.equal(got, ref)
Wc, Rpad, Wr = (L + 63) // 64, (R + 63) // 64 * 64, (R + 63) // 64
plane_b, nbr_b, tiles = 4 * Wc * Rpad * 8, R * Wr * 8, Wr * (Wr + 1) // 2
print("    sq_row_identity between HIP events (4 memsets + 3 kernels): %s" % show(whole_us), flush=True)
print("    planes kernel alone (+ 3 memsets): %s; reads %d bytes of rows, writes %d bytes of planes" % (show(phase_us[0]), R * L, plane_b), flush=True)
print("    pairs kernel alone (+ 2 memsets): %s; %d tiles read 2 x %d bytes of planes each = %d bytes (from L2 after the first), write %d bytes "
      "of neighbour bits%s" % (show(phase_us[1]), tiles, 4 * Wc * 64 * 8, tiles * 2 * 4 * Wc * 64 * 8, nbr_b,
                               " and 2 x %d bytes of matrices" % (4 * R * R) if matrix else ""), flush=True)
print("    filter kernel alone (+ 1 memset): %s; one wave reads the %d bytes of neighbour bits (%d of them at or below the diagonal: the rest "
      "meets kept bits that are still zero), writes %d bytes" % (show(phase_us[2]), nbr_b, sum(8 * (a // 64 + 1) for a in range(R)), R), flush=True)
print("    share of the filter kernel in the call between events: %.2f (best over best)" % (min(phase_us[2]) / min(whole_us)), flush=True)

# ---- (b) torch ops on the device: counts and neighbours, chunked over rows
lut = torch.from_numpy(CV._classes(np.arange(256, dtype=np.uint8))).to(dev)
CHUNK = max(1, min(R, (1 << 28) // max(R, 1)))                            # rows of a chunk: 2^28 cells at a time


def torch_counts():
    cls = lut[d_rows.long()]
    hot = [(cls == k).float() for k in range(4)]
    resf = (cls != 4).float()
    length = resf.sum(1).long()
    nb = torch.empty(R, dtype=torch.int64, device=dev)
    same_m = torch.empty((R, R), dtype=torch.int32, device=dev) if matrix else None
    both_m = torch.empty((R, R), dtype=torch.int32, device=dev) if matrix else None
    for r0 in range(0, R, CHUNK):
        r1 = min(R, r0 + CHUNK)
        same = sum(h[r0:r1] @ h.T for h in hot).long()
        den = torch.minimum(length[r0:r1, None], length[None, :])
        near = (den > 0) & (same * 10000 >= T * den)
        near[torch.arange(r1 - r0, device=dev), torch.arange(r0, r1, device=dev)] = False
        nb[r0:r1] = 1 + near.sum(1)
        if matrix:
            same_m[r0:r1] = same.int()
            both_m[r0:r1] = (resf[r0:r1] @ resf.T).int()
    return length, nb, same_m, both_m


torch_us = []
for k in range(warmup + timed):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    t_len, t_nb, t_same, t_both = torch_counts()
    ev[1].record()
    torch.cuda.synchronize()
    if k >= warmup:
        torch_us.append(ev[0].elapsed_time(ev[1]) * 1e3)
assert torch.equal(t_len.int(), res.len) and torch.equal(t_nb.int(), res.neighbours)
if matrix:
    assert torch.equal(t_same, res.same) and torch.equal(t_both, res.both)
del t_same, t_both
print("(b) len, neighbours%s with torch ops on the device (float32 one-hot products, %d rows at a time; NOT the filter: a row's verdict "
      "needs the verdicts before it), between HIP events: %s" % (", same, both" if matrix else "", CHUNK, show(torch_us)), flush=True)

# ---- (c) download + numpy, the filter over packed bit rows
c_down, c_np = [], []
c_warm, c_timed = (warmup, timed) if matrix else (0, min(timed, 2))
ftype = np.float32 if L * 10000 < 1 << 24 else np.float64               # (same * 10000 and T * den stay exact)
for k in range(c_warm + c_timed):
    t0 = sync_time()
    host = d_rows.cpu().numpy()
    t1 = time.perf_counter()
    cls = CV._classes(host)
    same = sum(h @ h.T for h in ((cls == q).astype(ftype) for q in range(4)))
    resf = (cls != 4).astype(ftype)
    length = resf.sum(1)
    both = resf @ resf.T if matrix else None
    den = np.minimum(length[:, None], length[None, :])
    near = (den > 0) & (same * 10000 >= T * den)
    near[np.arange(R), np.arange(R)] = False
    n_nb = 1 + near.sum(1)
    bits = np.packbits(near, axis=1, bitorder="little")
    kept = np.zeros(bits.shape[1], np.uint8)
    n_keep = np.zeros(R, bool)
    for a in range(R):
        if not (bits[a] & kept).any():
            kept[a >> 3] |= 1 << (a & 7)
            n_keep[a] = True
    t2 = time.perf_counter()
    if k >= c_warm:
        c_down.append(t1 - t0); c_np.append(t2 - t1)
assert np.array_equal(length.astype(np.int32), res.len.cpu().numpy()) and np.array_equal(n_nb.astype(np.int32), res.neighbours.cpu().numpy())
assert np.array_equal(n_keep, res.keep.cpu().numpy())
if matrix:
    assert np.array_equal(same.astype(np.int32), res.same.cpu().numpy()) and np.array_equal(both.astype(np.int32), res.both.cpu().numpy())
print("(c) download best %.6f s + numpy (counts, neighbours, filter) best %.4f s, median %.4f s; the outputs are equal" % (min(c_down), min(c_np), med(c_np)), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
