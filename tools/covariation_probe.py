#!/usr/bin/env python3
"""The covariation table of one random alignment of R rows and L columns with planted helices (column pairs that hold a
canonical pair in most rows, the pair type drawn per row), timed three ways:
 (a) the whole Covariation call, and sq_covariation_scan alone between HIP events (buffers allocated before; the bit planes
     alone are timed as sq_covariation_pairs with no pair);
 (b) the same table with torch ops on the device: one-hot matrix products per pair type, the thresholds, nonzero;
 (c) the rows downloaded and the same table with numpy (float64 matrix products: exact at these sizes, and BLAS).
The three tables are asserted equal.  Medians over the timed calls.
usage: covariation_probe.py R L [minspan] [WARMUP] [TIMED] [MIN_ROWS]      (MIN_ROWS: default R // 2; min_cov stays 1)"""
import ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import Covariation, _lib, covariation as CV

R, L = int(sys.argv[1]), int(sys.argv[2])
minspan = int(sys.argv[3]) if len(sys.argv) > 3 else 4
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 3
timed = int(sys.argv[5]) if len(sys.argv) > 5 else 10
min_rows = int(sys.argv[6]) if len(sys.argv) > 6 else R // 2
min_cov = 1
rng = random.Random(R * 100003 + L)
rows = [[rng.choice("ACGU-") if rng.random() < 0.97 else "N" for _ in range(L)] for _ in range(R)]
helices = max(L // 60, 1)
for h in range(helices):                                                  # helices of 6 pairs, loops of at least 4
    i0 = rng.randrange(0, L - 16)
    j0 = rng.randrange(i0 + 15, L)
    for k in range(6):
        for r in range(R):
            if rng.random() < 0.9:
                rows[r][i0 + k], rows[r][j0 - k] = rng.choice(CV.TYPES)
seqs = ["".join(r) for r in rows]
TYPE_IDX = [("ACGU".index(t[0]), "ACGU".index(t[1])) for t in CV.TYPES]
med = statistics.median


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def dense(xp, cls, as_float, as_int):
    hot = [as_float(cls == k) for k in range(5)]
    c = as_int(xp.stack([hot[a].T @ hot[b] for a, b in TYPE_IDX] + [hot[4].T @ hot[4]], -1))
    n = c[..., :6]
    cov = n.sum(-1) ** 2 - (n * n).sum(-1) - (n[..., 4] * (n[..., 0] + n[..., 2]) + n[..., 5] * (n[..., 1] + n[..., 3]))
    return c, n.sum(-1), cov


def torch_table(d_rows, lut):
    """(b): (flat, counts, cov) sorted by flat index, with torch ops on the rows' device."""
    c, bp, cov = dense(torch, lut[d_rows.long()], lambda m: m.float(), lambda m: m.long())
    span = torch.arange(L, device=d_rows.device)[None, :] - torch.arange(L, device=d_rows.device)[:, None]
    at = ((span >= max(minspan, 1)) & (bp >= min_rows) & (cov >= min_cov)).nonzero(as_tuple=True)
    return at[0] * L + at[1], c[at[0], at[1]], cov[at[0], at[1]]


def numpy_table(d_rows):
    """(c): (seconds of the download, of numpy, the table)."""
    t0 = sync_time()
    host = d_rows.cpu().numpy()
    t1 = time.perf_counter()
    c, bp, cov = dense(np, CV._classes(host), lambda m: m.astype(np.float64), lambda m: m.astype(np.int64))
    span = np.arange(L)[None, :] - np.arange(L)[:, None]
    at = np.nonzero((span >= max(minspan, 1)) & (bp >= min_rows) & (cov >= min_cov))
    table = (at[0] * L + at[1], c[at], cov[at])
    return t1 - t0, time.perf_counter() - t1, table


# ---- (a) the whole call
a_total = []
for k in range(warmup + timed):
    t0 = sync_time()
    res = Covariation(sequences=seqs, minspan=minspan, min_rows=min_rows, min_cov=min_cov)
    t = sync_time() - t0
    if k >= warmup:
        a_total.append(t)
assert res.source == "device" and res.mode == "scan"
P = len(res)
flat_ref = (res.pair_cols[:, 0].long() * L + res.pair_cols[:, 1].long())
print("R %d x L %d, %d planted helices, minspan %d, min_rows %d, min_cov %d: %d of %d cells emitted, %d of them covary; %d warm-up, "
      "%d timed calls, medians" % (R, L, helices, minspan, min_rows, min_cov, P, L * (L - 1) // 2, int(res.covarying().sum()), warmup, timed), flush=True)
print("(a) Covariation (rows to bytes, upload, planes, scan, sort by cell) %.6f s" % med(a_total), flush=True)

# ---- sq_covariation_scan alone, the planes alone, and (b), between HIP events with buffers allocated before
lib = _lib.load()
dev = res.device
d_rows = torch.from_numpy(np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).reshape(R, L).copy()).to(dev)
lut = torch.from_numpy(CV._classes(np.arange(256, dtype=np.uint8))).to(dev)
nbytes = int(lib.sq_covariation_scratch(R, L))
cap = max(P, 1)
scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
flat, counts, cov = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty((cap, 7), dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
out = torch.empty(2, dtype=torch.int64, device=dev)
p = lambda x: ctypes.c_void_p(x.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
scan_us, planes_us, torch_us = [], [], []
for k in range(warmup + timed):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    ev[0].record()
    _lib.check(lib.sq_covariation_scan(p(d_rows), R, L, minspan, min_rows, min_cov, p(scratch), nbytes, p(flat), p(counts), p(cov), cap, p(out), stream))
    ev[1].record()
    torch.cuda.synchronize()
    assert out.tolist() == [P, 0]
    ev[2].record()
    _lib.check(lib.sq_covariation_pairs(p(d_rows), R, L, None, 0, p(scratch), nbytes, None, None, p(out), stream))
    ev[3].record()
    torch.cuda.synchronize()
    ev[4].record()
    t_flat, t_counts, t_cov = torch_table(d_rows, lut)
    ev[5].record()
    torch.cuda.synchronize()
    if k >= warmup:
        scan_us.append(ev[0].elapsed_time(ev[1]) * 1e3); planes_us.append(ev[2].elapsed_time(ev[3]) * 1e3); torch_us.append(ev[4].elapsed_time(ev[5]) * 1e3)
order = torch.argsort(flat[:P])
assert torch.equal(flat[:P][order], flat_ref) and torch.equal(counts[:P][order], res.counts) and torch.equal(cov[:P][order], res.cov)
assert torch.equal(t_flat, flat_ref) and torch.equal(t_counts.int(), res.counts) and torch.equal(t_cov, res.cov)
del t_flat, t_counts, t_cov
print("    sq_covariation_scan between HIP events (memset + planes kernel + scan kernel): median %.1f us (%s)" % (
    med(scan_us), " ".join("%.1f" % t for t in scan_us)), flush=True)
print("    of it the planes (sq_covariation_pairs with no pair: memset + planes kernel): median %.1f us; planes %d bytes" % (med(planes_us), nbytes), flush=True)
print("(b) the same table with torch ops on the device, between HIP events: median %.1f us (%s)" % (
    med(torch_us), " ".join("%.1f" % t for t in torch_us)), flush=True)

# ---- (c) download + numpy
c_down, c_np = [], []
for k in range(warmup + timed):
    d, n, table = numpy_table(d_rows)
    if k >= warmup:
        c_down.append(d); c_np.append(n)
assert np.array_equal(table[0], flat_ref.cpu().numpy()) and np.array_equal(table[1], res.counts.cpu().numpy()) and np.array_equal(table[2], res.cov.cpu().numpy())
print("(c) download %.6f s + numpy %.4f s; the three tables are equal" % (med(c_down), med(c_np)), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
