#!/usr/bin/env python3
"""The shuffled-column null of a covariation statistic of one random alignment of R rows and L columns with planted helices
(covariation_probe.py's alignment), K samples, for the observed pairs of CovariationStatistics(min_rows = R // 2, MIN_STAT),
timed three ways:
 (a) the whole CovariationStatisticsSignificance call, and sq_covariation_stat_null alone between HIP events (buffers allocated
     before), with its kernels' shares: the call without pairs (no pairs kernel), the same without a correction (no pass 1:
     the difference is pass 1 and its two reductions) and the planes of the same batches alone (sq_covariation_null_planes) --
     planes, scan = without a correction - planes, pass 1 = with - without a correction, pairs = whole - without pairs;
 (b) the same numbers formed by K calls of the entry behind CovariationStatistics (HipEngine.covariation_stat_scan with room for
     every cell in scope, min_rows 0: one scan a call and none of CovariationStatistics' sorting, the leanest form of the loop)
     on rows shuffled with torch ops on the device, plus torch ops: searchsorted + bincount, max, covariation_stat_pairs for the
     pairs' own cells;
 (c) the rows downloaded and the same with numpy (float64 matrix products: exact at these sizes, and BLAS), for the first
     C samples only, extrapolated to K.
(a) and (b) are asserted equal for all K samples.  (c) is compared under a bracket with the device's counts for the first C
samples: numpy sums in another order, so a count can differ where a null value lies within the float bound of an observed one;
the band is 2 (L + 8) 2^-53 of the two scales |S| + |correction term| (each side errs by at most (L + 8) 2^-53 of its scale:
a column sum of L - 1 addends of one sign and a few operations).  Medians over the timed calls.
usage: covariation_stat_null_probe.py R L K [statistic] [correction] [MIN_STAT] [minspan] [WARMUP] [TIMED] [C]"""
import ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import CovariationStatisticsSignificance, _lib, covariation as CV, covariation_significance as CS
from squarna_amd import covariation_statistics as ST, device_calls as DC
from squarna_amd.engine import HipEngine

R, L, K = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
statistic = sys.argv[4] if len(sys.argv) > 4 else "gt"
correction = (None if sys.argv[5] == "none" else sys.argv[5]) if len(sys.argv) > 5 else "apc"
min_stat = (None if sys.argv[6] == "none" else float(sys.argv[6])) if len(sys.argv) > 6 else 20.0
minspan = int(sys.argv[7]) if len(sys.argv) > 7 else 4
warmup = int(sys.argv[8]) if len(sys.argv) > 8 else 1
timed = int(sys.argv[9]) if len(sys.argv) > 9 else 3
C = min(int(sys.argv[10]) if len(sys.argv) > 10 else 1, K)
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
med = statistics.median
stat, corr = DC.COVAR_STATISTICS.index(statistic), DC.COVAR_CORRECTIONS.index(correction)
scope_cells = CS.scope_cells(L, minspan)


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def torch_keys(k, dev):
    """The sort keys of sample k as int64 whose signed order is the keys' unsigned order (covariation_null_probe.py)."""
    r = torch.arange(R, device=dev)[:, None]
    c = torch.arange(L, device=dev)[None, :]
    z = (signed((k * L) & CS._MASK) + c) * R + r
    z = (z + 1) * signed(0x9E3779B97F4A7C15) + signed(seed)
    for shift, mul in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
        z = (z ^ ((z >> shift) & ((1 << (64 - shift)) - 1))) * signed(mul)
    z = z ^ ((z >> 31) & ((1 << 33) - 1))
    return ((z & ~0xFFFF) | r) ^ signed(1 << 63)


def composed_null(eng, d_rows, cols, value, thresholds):
    """(b): (hist, own_ge, null_max) from K calls of the scan entry on shuffled rows and torch ops."""
    dev = d_rows.device
    hist = torch.zeros(len(thresholds) + 1, dtype=torch.int64, device=dev)
    own_ge = torch.zeros(len(value), dtype=torch.int32, device=dev)
    null_max = torch.full((K,), float("-inf"), dtype=torch.float64, device=dev)
    for k in range(K):
        shuffled = torch.gather(d_rows, 0, torch.argsort(torch_keys(k, dev), dim=0)).contiguous()
        cells = eng.covariation_stat_scan(shuffled, statistic, correction, minspan=minspan, min_rows=0, min_stat=None, cap=max(scope_cells, 1))[3]
        hist += torch.bincount(torch.searchsorted(thresholds, cells, right=True), minlength=len(hist))
        if cells.numel():
            null_max[k] = cells.max()
        if len(value):
            own_ge += (eng.covariation_stat_pairs(shuffled, cols, statistic, correction)[2] >= value).int()
    return hist, own_ge, null_max


def numpy_tables(cls):
    hot = [(cls == k).astype(np.float64) for k in range(4)]
    return np.stack([hot[a].T @ hot[b] for a in range(4) for b in range(4)], -1).astype(np.int64)


def numpy_values(cls):
    """(C float64[L, L], its scale |S| + |the correction term|) of class bytes, CovariationStatistics' numpy path."""
    S = ST._host_raw(numpy_tables(cls), statistic)
    mean, mean_all = ST._host_means(S) if correction is not None else (np.zeros(L), 0.0)
    value = ST._host_corrected(S, mean[:, None], mean[None, :], mean_all, correction)
    return value, np.abs(S) + np.abs(S - value)


def numpy_brackets(d_rows, cols, samples):
    """(c): (seconds of the download, of numpy, lo and hi of null_ge and of own_ge per pair) for the first `samples` samples."""
    t0 = sync_time()
    host = d_rows.cpu().numpy()
    t1 = time.perf_counter()
    bound = 2.0 * (L + 8) * 2.0 ** -53
    cls = CV._classes(host)
    v, w = cols[:, 0], cols[:, 1]
    obs, obs_scale = (a[v, w] for a in numpy_values(cls))
    span = np.arange(L)[None, :] - np.arange(L)[:, None]
    scope = span >= max(minspan, 1)
    low, high = [], []
    own = np.zeros((2, len(cols)), np.int64)
    for k in range(samples):
        null, scale = numpy_values(CS._shuffled_classes(cls, k, seed))
        low.append((null - bound * scale)[scope])
        high.append((null + bound * scale)[scope])
        own[0] += null[v, w] - bound * scale[v, w] >= obs + bound * obs_scale
        own[1] += null[v, w] + bound * scale[v, w] >= obs - bound * obs_scale
    low, high = np.sort(np.concatenate(low)), np.sort(np.concatenate(high))
    pooled = (len(low) - np.searchsorted(low, obs + bound * obs_scale), len(high) - np.searchsorted(high, obs - bound * obs_scale))
    return t1 - t0, time.perf_counter() - t1, pooled, own


# ---- (a) the whole call
a_total = []
for k in range(warmup + timed):
    t0 = sync_time()
    res = CovariationStatisticsSignificance(sequences=seqs, statistic=statistic, correction=correction, minspan=minspan, min_rows=min_rows,
                                            min_stat=min_stat, samples=K, seed=seed)
    t = sync_time() - t0
    if k >= warmup:
        a_total.append(t)
assert res.source == "device" and res.observed.mode == "scan"
P, dev = len(res), res.device
print("R %d x L %d, %d planted helices, %s / %s, minspan %d, min_rows %d, min_stat %s: %d observed pairs, %d samples, %d null cells, "
      "%d pairs with evalue <= 0.05; %d warm-up, %d timed calls, medians" % (R, L, helices, statistic, correction, minspan, min_rows, min_stat, P, K,
                                                                             res.null_cells, int(res.significant().sum()), warmup, timed), flush=True)
print("(a) CovariationStatisticsSignificance (rows to bytes, upload, CovariationStatistics, thresholds, the null, suffix sums) %.6f s" % med(a_total),
      flush=True)

# ---- sq_covariation_stat_null alone and its shares, between HIP events with buffers allocated before
lib = _lib.load()
d_rows = torch.from_numpy(np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).reshape(R, L).copy()).to(dev)
cols, value = res.observed.pair_cols.contiguous(), res.observed.value.contiguous()
thresholds = torch.unique(value)
U = int(thresholds.numel())
per = int(lib.sq_covariation_stat_null_scratch(R, L, 2)) - int(lib.sq_covariation_stat_null_scratch(R, L, 1))
batch = max(1, min(K, DC.COVAR_NULL_BATCH, DC.COVAR_NULL_BATCH_BYTES // per))
nbytes = int(lib.sq_covariation_stat_null_scratch(R, L, batch))
scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
hist, own_ge, null_max, out = new(U + 1, torch.int64), new(P, torch.int32), new(K, torch.float64), new(2, torch.int64)
hist0, max0, hist1, max1 = torch.empty_like(hist), torch.empty_like(null_max), torch.empty_like(hist), torch.empty_like(null_max)
p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def entry(corr_, with_pairs, hist_, max_, samples=K):
    _lib.check(lib.sq_covariation_stat_null(p(d_rows), R, L, stat, corr_, minspan, p(cols if with_pairs and P else None),
                                            p(value if with_pairs and P else None), P if with_pairs else 0, p(thresholds if U else None), U,
                                            samples, seed, batch, p(scratch), nbytes, p(hist_), p(own_ge if with_pairs and P else None), p(max_),
                                            p(out), stream))


whole_us, nopairs_us, nocorr_us, planes_us = [], [], [], []
for k in range(warmup + timed):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    ev[0].record()
    entry(corr, True, hist, null_max)
    ev[1].record()
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]
    ev[2].record()
    entry(corr, False, hist0, max0)
    ev[3].record()
    torch.cuda.synchronize()
    ev[4].record()
    entry(0, False, hist1, max1)
    ev[5].record()
    torch.cuda.synchronize()
    ev[6].record()
    for s in range(0, K, batch):
        _lib.check(lib.sq_covariation_null_planes(p(d_rows), R, L, s, min(batch, K - s), seed, p(scratch), nbytes, stream))
    ev[7].record()
    torch.cuda.synchronize()
    if k >= warmup:
        for times, a in ((whole_us, 0), (nopairs_us, 2), (nocorr_us, 4), (planes_us, 6)):
            times.append(ev[a].elapsed_time(ev[a + 1]) * 1e3)
same_bits = lambda x, y: torch.equal(x.view(torch.int64), y.view(torch.int64))
assert torch.equal(hist, hist0) and same_bits(null_max, max0) and same_bits(null_max, res.null_max) and torch.equal(own_ge, res.own_ge)
from_bin = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
assert torch.equal(from_bin[torch.searchsorted(thresholds, value) + 1], res.null_ge) and int(hist.sum()) == res.null_cells == int(hist1.sum())
whole, nopairs, nocorr, planes = med(whole_us), med(nopairs_us), med(nocorr_us), med(planes_us)
print("    sq_covariation_stat_null between HIP events (%d samples a batch, %d thresholds): median %.1f us (%s)" % (
    batch, U, whole, " ".join("%.1f" % t for t in whole_us)), flush=True)
print("    without pairs %.1f us; without pairs and without a correction (no pass 1) %.1f us; the planes of the same batches alone "
      "(sq_covariation_null_planes) %.1f us; so per sample planes %.1f, pass 1 and its reductions %.1f, scan %.1f, pairs %.1f us" % (
          nopairs, nocorr, planes, planes / K, (nopairs - nocorr) / K, (nocorr - planes) / K, (whole - nopairs) / K), flush=True)

# ---- (b) K calls of the scan entry on shuffled rows + torch ops
eng = HipEngine()
loop_s = []
for k in range(1 + min(timed, 1)):
    t0 = sync_time()
    b_hist, b_own, b_max = composed_null(eng, d_rows, cols, value, thresholds)
    t = sync_time() - t0
    if k:
        loop_s.append(t)
assert torch.equal(b_hist, hist) and torch.equal(b_own, own_ge) and torch.equal(b_max, null_max)
print("(b) the same numbers from %d calls of covariation_stat_scan (+ covariation_stat_pairs) on rows shuffled with torch ops, + torch ops: "
      "%.4f s, equal to (a) in every count and maximum; the entry alone takes %.2f x less, the whole call %.2f x less" % (
          K, med(loop_s), med(loop_s) / (whole * 1e-6), med(loop_s) / med(a_total)), flush=True)

# ---- (c) download + numpy, the first C samples, under the bracket
entry(corr, True, hist, null_max, C)
torch.cuda.synchronize()
from_bin = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
dev_ge = from_bin[torch.searchsorted(thresholds, value) + 1].cpu().numpy() if P else np.zeros(0, np.int64)
dev_own = own_ge.cpu().numpy()
d, n, pooled, own = numpy_brackets(d_rows, cols.cpu().numpy().astype(np.int64), C)
assert ((pooled[0] <= dev_ge) & (dev_ge <= pooled[1])).all() and ((own[0] <= dev_own) & (dev_own <= own[1])).all()
print("(c) download %.6f s + numpy %.3f s for %d samples = %.1f s for %d; the device's counts lie in numpy's brackets "
      "(%d of %d pairs with lo == hi, uncertain %d of %d counted cells)" % (
          d, n, C, n / C * K, K, int((pooled[0] == pooled[1]).sum()), P, int((pooled[1] - pooled[0]).sum()), int(pooled[1].sum())), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
