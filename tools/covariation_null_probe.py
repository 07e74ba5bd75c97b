#!/usr/bin/env python3
"""The shuffled-column null of one random alignment of R rows and L columns with planted helices (covariation_probe.py's
alignment), K samples, for the observed pairs of Covariation(min_rows = R // 2), timed three ways:
 (a) the whole CovariationSignificance call, and sq_covariation_null alone between HIP events (buffers allocated before), with
     its kernels' shares: the call without pairs (no pairs kernel), and the planes of the same batches alone
     (sq_covariation_null_planes: the classes and the planes kernel) -- scan = without pairs - planes, pairs = whole - without
     pairs; beside them one
     sq_covariation_scan of the same alignment, the yardstick of the null scan's time per sample;
 (b) the same numbers with torch ops on the device: the sort keys in int64 arithmetic, argsort, one-hot matrix products, the
     bins by searchsorted + bincount;
 (c) the rows downloaded and the same with numpy (float64 matrix products: exact at these sizes, and BLAS), for the first
     C samples only (a sample takes seconds at 512 x 5000), extrapolated to K.
(a) and (b) are asserted equal for all K samples, (c) with (b)'s state after C samples.  Medians over the timed calls.
usage: covariation_null_probe.py R L K [minspan] [WARMUP] [TIMED] [C]"""
import ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import CovariationSignificance, _lib, covariation as CV, covariation_significance as CS

R, L, K = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
minspan = int(sys.argv[4]) if len(sys.argv) > 4 else 4
warmup = int(sys.argv[5]) if len(sys.argv) > 5 else 2
timed = int(sys.argv[6]) if len(sys.argv) > 6 else 5
C = min(int(sys.argv[7]) if len(sys.argv) > 7 else 2, K)
seed, min_rows = 12345, R // 2
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


def signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def dense_cov(xp, cls, as_float, as_int):
    hot = [as_float(cls == k) for k in range(4)]
    n = as_int(xp.stack([hot[a].T @ hot[b] for a, b in TYPE_IDX], -1))
    return n.sum(-1) ** 2 - (n * n).sum(-1) - (n[..., 4] * (n[..., 0] + n[..., 2]) + n[..., 5] * (n[..., 1] + n[..., 3]))


def torch_keys(k, dev):
    """The sort keys of sample k as int64 whose signed order is the keys' unsigned order (two's complement products wrap as the
    definition's; a logical shift is the arithmetic one masked; the top bit is flipped at the end)."""
    r = torch.arange(R, device=dev)[:, None]
    c = torch.arange(L, device=dev)[None, :]
    z = (signed((k * L) & CS._MASK) + c) * R + r
    z = (z + 1) * signed(0x9E3779B97F4A7C15) + signed(seed)
    for shift, mul in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
        z = (z ^ ((z >> shift) & ((1 << (64 - shift)) - 1))) * signed(mul)
    z = z ^ ((z >> 31) & ((1 << 33) - 1))
    return ((z & ~0xFFFF) | r) ^ signed(1 << 63)


def torch_null(d_cls, cols, cov, thresholds, scope, snapshot_at):
    """(b): (hist, own_ge, null_max) with torch ops on the rows' device, and their state after `snapshot_at` samples."""
    dev = d_cls.device
    hist = torch.zeros(len(thresholds) + 1, dtype=torch.int64, device=dev)
    own_ge, null_max = torch.zeros(len(cov), dtype=torch.int64, device=dev), torch.zeros(K, dtype=torch.int64, device=dev)
    v, w = cols[:, 0].long(), cols[:, 1].long()
    snap = None
    for k in range(K):
        shuffled = torch.gather(d_cls, 0, torch.argsort(torch_keys(k, dev), dim=0))
        null = dense_cov(torch, shuffled, lambda m: m.float(), lambda m: m.long())
        cells = null[scope]
        hist += torch.bincount(torch.searchsorted(thresholds, cells, right=True), minlength=len(hist))
        null_max[k] = cells.max() if cells.numel() else 0
        own_ge += null[v, w] >= cov
        if k + 1 == snapshot_at:
            snap = (hist.clone(), own_ge.clone(), null_max[:snapshot_at].clone())
    return (hist, own_ge, null_max), snap


def numpy_null(d_rows, cols, cov, thresholds, samples):
    """(c): (seconds of the download, of numpy, (hist, own_ge, null_max)) for the first `samples` samples."""
    t0 = sync_time()
    host = d_rows.cpu().numpy()
    t1 = time.perf_counter()
    cls = CV._classes(host)
    span = np.arange(L)[None, :] - np.arange(L)[:, None]
    scope = span >= max(minspan, 1)
    hist, own_ge, null_max = np.zeros(len(thresholds) + 1, np.int64), np.zeros(len(cov), np.int64), np.zeros(samples, np.int64)
    for k in range(samples):
        null = dense_cov(np, CS._shuffled_classes(cls, k, seed), lambda m: m.astype(np.float64), lambda m: m.astype(np.int64))
        cells = null[scope]
        hist += np.bincount(np.searchsorted(thresholds, cells, side="right"), minlength=len(hist))
        null_max[k] = cells.max(initial=0)
        own_ge += null[cols[:, 0], cols[:, 1]] >= cov
    return t1 - t0, time.perf_counter() - t1, (hist, own_ge, null_max)


# ---- (a) the whole call
a_total = []
for k in range(warmup + timed):
    t0 = sync_time()
    res = CovariationSignificance(sequences=seqs, minspan=minspan, min_rows=min_rows, samples=K, seed=seed)
    t = sync_time() - t0
    if k >= warmup:
        a_total.append(t)
assert res.source == "device" and res.observed.mode == "scan"
P, dev = len(res), res.device
print("R %d x L %d, %d planted helices, minspan %d, min_rows %d: %d observed pairs, %d samples, %d null cells, %d pairs with evalue <= 0.05; "
      "%d warm-up, %d timed calls, medians" % (R, L, helices, minspan, min_rows, P, K, res.null_cells, int(res.significant().sum()), warmup, timed), flush=True)
print("(a) CovariationSignificance (rows to bytes, upload, Covariation, thresholds, the null, suffix sums) %.6f s" % med(a_total), flush=True)

# ---- sq_covariation_null alone and its shares, between HIP events with buffers allocated before
from squarna_amd import device_calls as DC
lib = _lib.load()
d_rows = torch.from_numpy(np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).reshape(R, L).copy()).to(dev)
cols, cov = res.observed.pair_cols.contiguous(), res.observed.cov.contiguous()
thresholds = torch.unique(cov)
U = int(thresholds.numel())
per = 5 * ((R + 63) // 64) * ((L + 63) // 64 * 64) * 8
batch = max(1, min(K, DC.COVAR_NULL_BATCH, DC.COVAR_NULL_BATCH_BYTES // per))
nbytes = int(lib.sq_covariation_null_scratch(R, L, batch))
scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
hist, own_ge, null_max = torch.empty(U + 1, dtype=torch.int64, device=dev), torch.empty(P, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
hist0, max0 = torch.empty_like(hist), torch.empty_like(null_max)
out = torch.empty(2, dtype=torch.int64, device=dev)
scan_bytes = int(lib.sq_covariation_scratch(R, L))
scan_scratch = torch.empty(scan_bytes // 8, dtype=torch.int64, device=dev)
cap = max(P, 1)
s_flat, s_counts, s_cov = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty((cap, 7), dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
whole_us, nopairs_us, planes_us, scan_us = [], [], [], []
for k in range(warmup + timed):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    ev[0].record()
    _lib.check(lib.sq_covariation_null(p(d_rows), R, L, minspan, p(cols if P else None), p(cov if P else None), P, p(thresholds if U else None), U, K,
                                       seed, batch, p(scratch), nbytes, p(hist), p(own_ge if P else None), p(null_max), p(out), stream))
    ev[1].record()
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]
    ev[2].record()
    _lib.check(lib.sq_covariation_null(p(d_rows), R, L, minspan, None, None, 0, p(thresholds if U else None), U, K, seed, batch, p(scratch), nbytes,
                                       p(hist0), None, p(max0), p(out), stream))
    ev[3].record()
    torch.cuda.synchronize()
    ev[4].record()
    for s in range(0, K, batch):
        _lib.check(lib.sq_covariation_null_planes(p(d_rows), R, L, s, min(batch, K - s), seed, p(scratch), nbytes, stream))
    ev[5].record()
    torch.cuda.synchronize()
    ev[6].record()
    _lib.check(lib.sq_covariation_scan(p(d_rows), R, L, minspan, min_rows, 1, p(scan_scratch), scan_bytes, p(s_flat), p(s_counts), p(s_cov), cap, p(out), stream))
    ev[7].record()
    torch.cuda.synchronize()
    if k >= warmup:
        whole_us.append(ev[0].elapsed_time(ev[1]) * 1e3); nopairs_us.append(ev[2].elapsed_time(ev[3]) * 1e3)
        planes_us.append(ev[4].elapsed_time(ev[5]) * 1e3); scan_us.append(ev[6].elapsed_time(ev[7]) * 1e3)
assert torch.equal(hist, hist0) and torch.equal(null_max, max0) and torch.equal(null_max, res.null_max) and torch.equal(own_ge, res.own_ge)
from_bin = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
assert torch.equal(from_bin[torch.searchsorted(thresholds, cov) + 1], res.null_ge) and int(hist.sum()) == res.null_cells
whole, nopairs, planes = med(whole_us), med(nopairs_us), med(planes_us)
print("    sq_covariation_null between HIP events (%d samples a batch, %d thresholds): median %.1f us (%s)" % (
    batch, U, whole, " ".join("%.1f" % t for t in whole_us)), flush=True)
print("    without pairs %.1f us; the planes of the same batches alone (sq_covariation_null_planes) %.1f us; so planes %.1f, scan %.1f, pairs %.1f us per sample" % (
    nopairs, planes, planes / K, (nopairs - planes) / K, (whole - nopairs) / K), flush=True)
print("    one sq_covariation_scan of the same alignment (memset + planes + scan, %d cells emitted): median %.1f us; the null scan takes %.2f x that per sample" % (
    P, med(scan_us), (nopairs - planes) / K / med(scan_us)), flush=True)

# ---- (b) torch ops on the device
lut = torch.from_numpy(CV._classes(np.arange(256, dtype=np.uint8))).to(dev)
span = torch.arange(L, device=dev)[None, :] - torch.arange(L, device=dev)[:, None]
scope = span >= max(minspan, 1)
torch_s = []
for k in range(1 + min(timed, 2)):
    t0 = sync_time()
    b_all, b_snap = torch_null(lut[d_rows.long()], cols, cov, thresholds, scope, C)
    t = sync_time() - t0
    if k:
        torch_s.append(t)
assert torch.equal(b_all[0], hist) and torch.equal(b_all[1].int(), own_ge) and torch.equal(b_all[2], null_max)
print("(b) the same numbers with torch ops on the device: median %.4f s" % med(torch_s), flush=True)

# ---- (c) download + numpy, the first C samples
d, n, c_got = numpy_null(d_rows, cols.cpu().numpy().astype(np.int64), cov.cpu().numpy(), thresholds.cpu().numpy(), C)
assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(c_got, b_snap))
print("(c) download %.6f s + numpy %.3f s for %d samples = %.1f s for %d; the outputs are equal" % (d, n, C, n / C * K, K), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
