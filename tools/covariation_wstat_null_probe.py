#!/usr/bin/env python3
"""The shuffled-column null of a weighted covariation statistic of one random alignment of R rows and L columns with planted
helices (covariation_stat_probe.py's alignment) and row weights 1 / k, k drawn from 1 .. 8 per row (covariation_wstat_probe.py's
weights), K samples, for the observed pairs of CovariationStatistics(weights=, min_rows = R / 8, MIN_STAT), timed three ways:
 (a) the whole CovariationStatisticsSignificance(weights=) call, and sq_covariation_wstat_null alone between HIP events (buffers
     allocated before), with its kernels' shares: the call without pairs (no pairs kernel), the same without a correction (no
     pass 1: the difference is pass 1 and its two reductions) and the planes of the same batches alone
     (sq_covariation_null_planes) -- planes, scan = without a correction - planes, pass 1 = with - without a correction,
     pairs = whole - without pairs;
 (b) the same numbers formed by K calls of the entry behind CovariationStatistics(weights=) (HipEngine.covariation_wstat_scan with
     room for every cell in scope, min_rows 0: one scan a call and none of CovariationStatistics' sorting, the leanest form of
     the loop) on rows shuffled with torch ops on the device and the same weights, plus torch ops: searchsorted + bincount,
     max, covariation_wstat_pairs for the pairs' own cells; asserted equal to (a) for all K samples, bit for bit;
 (c) the unweighted sq_covariation_stat_null at the same shape, K and batch rule between HIP events, for the observed pairs of
     the unweighted CovariationStatistics at about as many rows.
One warm-up, then the median over the timed regions.  Every step that uses the GPU is a process of its own under its own time
limit; the first that fails ends the probe.
usage: covariation_wstat_null_probe.py R L K [statistic] [correction] [MIN_STAT] [minspan] [WARMUP] [TIMED]
       (defaults: gt apc 20 4 1 3; correction "none" for None; MIN_STAT "none" for None)"""
import ctypes, os, random, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("entry", 600), ("composed", 900), ("unweighted", 300))          # (step, its time limit in seconds)

if "--step" not in sys.argv:                                              # the parent: no GPU here, one child per step
    for step, limit in STEPS:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--step", step], timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit("step %s: no end within %d s" % (step, limit))
        if done.returncode:
            sys.exit("step %s: exit status %d" % (step, done.returncode))
    sys.exit(0)

import numpy as np
import torch
from squarna_amd import CovariationStatistics, CovariationStatisticsSignificance, _lib, covariation as CV, covariation_significance as CS
from squarna_amd import device_calls as DC
from squarna_amd.engine import HipEngine

step = sys.argv[sys.argv.index("--step") + 1]
args = sys.argv[1:sys.argv.index("--step")]
R, L, K = int(args[0]), int(args[1]), int(args[2])
statistic = args[3] if len(args) > 3 else "gt"
correction = (None if args[4] == "none" else args[4]) if len(args) > 4 else "apc"
min_stat = (None if args[5] == "none" else float(args[5])) if len(args) > 5 else 20.0
minspan = int(args[6]) if len(args) > 6 else 4
warmup = int(args[7]) if len(args) > 7 else 1
timed = int(args[8]) if len(args) > 8 else 3
seed, min_rows = 12345, R / 8
stat, corr = DC.COVAR_STATISTICS.index(statistic), DC.COVAR_CORRECTIONS.index(correction)
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
weights = np.array([1.0 / rng.randrange(1, 9) for _ in range(R)])
med = statistics.median
scope_cells = CS.scope_cells(L, minspan)
dev = torch.device("cuda", torch.cuda.current_device())
d_weights = torch.from_numpy(weights).to(dev)
d_rows = torch.from_numpy(np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).reshape(R, L).copy()).to(dev)
lib = _lib.load()
p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
same_bits = lambda x, y: torch.equal(x.view(torch.int64), y.view(torch.int64))


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def batch_of(scratch_of):
    per = int(scratch_of(R, L, 2)) - int(scratch_of(R, L, 1))
    return max(1, min(K, DC.COVAR_NULL_BATCH, DC.COVAR_NULL_BATCH_BYTES // per))


def observed():
    """(pairs int32[P, 2], value, thresholds) of the weighted scan: the observed pairs of the null."""
    res = CovariationStatistics(sequences=seqs, weights=d_weights, statistic=statistic, correction=correction, minspan=minspan, min_rows=min_rows,
                                min_stat=min_stat)
    assert res.source == "device" and res.mode == "scan"
    return res.pair_cols.contiguous(), res.value.contiguous(), torch.unique(res.value)


class Entry:
    """sq_covariation_wstat_null with buffers allocated once."""

    def __init__(self, cols, value, thresholds):
        self.cols, self.value, self.thresholds, self.P, self.U = cols, value, thresholds, int(value.numel()), int(thresholds.numel())
        self.batch = batch_of(lib.sq_covariation_wstat_null_scratch)
        self.nbytes = int(lib.sq_covariation_wstat_null_scratch(R, L, self.batch))
        self.scratch = new(self.nbytes // 8, torch.int64)
        self.own_ge, self.out = new(self.P, torch.int32), new(2, torch.int64)

    def __call__(self, corr_, with_pairs, hist, null_max):
        P, U = self.P if with_pairs else 0, self.U
        _lib.check(lib.sq_covariation_wstat_null(p(d_rows), R, L, stat, corr_, minspan, p(self.cols if P else None), p(self.value if P else None), P,
                                                 p(self.thresholds if U else None), U, K, seed, self.batch, p(self.scratch), self.nbytes, p(hist),
                                                 p(self.own_ge if P else None), p(null_max), p(self.out), stream, p(d_weights)))

    def results(self):
        hist, null_max = new(self.U + 1, torch.int64), new(K, torch.float64)
        self(corr, True, hist, null_max)
        torch.cuda.synchronize()
        assert self.out.tolist() == [0, 0]
        return hist, self.own_ge.clone(), null_max


if step == "entry":
    a_total = []
    for k in range(warmup + timed):
        t0 = sync_time()
        res = CovariationStatisticsSignificance(sequences=seqs, weights=d_weights, statistic=statistic, correction=correction, minspan=minspan,
                                                min_rows=min_rows, min_stat=min_stat, samples=K, seed=seed)
        t = sync_time() - t0
        if k >= warmup:
            a_total.append(t)
    assert res.source == "device" and res.observed.mode == "scan"
    print("R %d x L %d, %d planted helices, weights 1 / k (their sum %.1f), %s / %s, minspan %d, min_rows %g, min_stat %s: %d observed pairs, "
          "%d samples, %d null cells, %d pairs with evalue <= 0.05; %d warm-up, %d timed calls, medians" % (
              R, L, helices, weights.sum(), statistic, correction, minspan, min_rows, min_stat, len(res), K, res.null_cells,
              int(res.significant().sum()), warmup, timed), flush=True)
    print("(a) CovariationStatisticsSignificance(weights=) (rows to bytes, upload, CovariationStatistics(weights=), thresholds, the null, suffix "
          "sums) %.6f s" % med(a_total), flush=True)
    entry = Entry(res.observed.pair_cols.contiguous(), res.observed.value.contiguous(), torch.unique(res.observed.value))
    hist, null_max = new(entry.U + 1, torch.int64), new(K, torch.float64)
    hist0, max0, hist1, max1 = torch.empty_like(hist), torch.empty_like(null_max), torch.empty_like(hist), torch.empty_like(null_max)
    whole_us, nopairs_us, nocorr_us, planes_us = [], [], [], []
    for k in range(warmup + timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ev[0].record()
        entry(corr, True, hist, null_max)
        ev[1].record()
        torch.cuda.synchronize()
        assert entry.out.tolist() == [0, 0]
        ev[2].record()
        entry(corr, False, hist0, max0)
        ev[3].record()
        torch.cuda.synchronize()
        ev[4].record()
        entry(0, False, hist1, max1)
        ev[5].record()
        torch.cuda.synchronize()
        ev[6].record()
        for s in range(0, K, entry.batch):
            _lib.check(lib.sq_covariation_null_planes(p(d_rows), R, L, s, min(entry.batch, K - s), seed, p(entry.scratch), entry.nbytes, stream))
        ev[7].record()
        torch.cuda.synchronize()
        if k >= warmup:
            for times, a in ((whole_us, 0), (nopairs_us, 2), (nocorr_us, 4), (planes_us, 6)):
                times.append(ev[a].elapsed_time(ev[a + 1]) * 1e3)
    assert torch.equal(hist, hist0) and same_bits(null_max, max0) and same_bits(null_max, res.null_max) and torch.equal(entry.own_ge, res.own_ge)
    from_bin = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
    assert torch.equal(from_bin[torch.searchsorted(entry.thresholds, entry.value) + 1], res.null_ge)
    assert int(hist.sum()) == res.null_cells == int(hist1.sum())
    whole, nopairs, nocorr, planes = med(whole_us), med(nopairs_us), med(nocorr_us), med(planes_us)
    print("    sq_covariation_wstat_null between HIP events (%d samples a batch, %d thresholds, COVAR_WSTAT_NULL_LDS_BINS %d): median %.1f us (%s)" % (
        entry.batch, entry.U, DC.COVAR_WSTAT_NULL_LDS_BINS, whole, " ".join("%.1f" % t for t in whole_us)), flush=True)
    print("    without pairs %.1f us; without pairs and without a correction (no pass 1) %.1f us; the planes of the same batches alone "
          "(sq_covariation_null_planes) %.1f us; so per sample planes %.1f, pass 1 and its reductions %.1f, scan %.1f, pairs %.1f us" % (
              nopairs, nocorr, planes, planes / K, (nopairs - nocorr) / K, (nocorr - planes) / K, (whole - nopairs) / K), flush=True)
    print("    peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "composed":
    def signed(x):
        return x - (1 << 64) if x >= 1 << 63 else x

    def torch_keys(k):
        """The sort keys of sample k as int64 whose signed order is the keys' unsigned order (covariation_null_probe.py)."""
        r = torch.arange(R, device=dev)[:, None]
        c = torch.arange(L, device=dev)[None, :]
        z = (signed((k * L) & CS._MASK) + c) * R + r
        z = (z + 1) * signed(0x9E3779B97F4A7C15) + signed(seed)
        for shift, mul in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
            z = (z ^ ((z >> shift) & ((1 << (64 - shift)) - 1))) * signed(mul)
        z = z ^ ((z >> 31) & ((1 << 33) - 1))
        return ((z & ~0xFFFF) | r) ^ signed(1 << 63)

    def composed_null(eng, cols, value, thresholds):
        """(hist, own_ge, null_max) from K calls of the weighted scan entry on shuffled rows and torch ops."""
        hist = torch.zeros(len(thresholds) + 1, dtype=torch.int64, device=dev)
        own_ge = torch.zeros(len(value), dtype=torch.int32, device=dev)
        null_max = torch.full((K,), float("-inf"), dtype=torch.float64, device=dev)
        for k in range(K):
            shuffled = torch.gather(d_rows, 0, torch.argsort(torch_keys(k), dim=0)).contiguous()
            cells = eng.covariation_wstat_scan(shuffled, d_weights, statistic, correction, minspan=minspan, min_rows=0.0, min_stat=None,
                                               cap=max(scope_cells, 1))[3]
            hist += torch.bincount(torch.searchsorted(thresholds, cells, right=True), minlength=len(hist))
            if cells.numel():
                null_max[k] = cells.max()
            if len(value):
                own_ge += (eng.covariation_wstat_pairs(shuffled, d_weights, cols, statistic, correction)[2] >= value).int()
        return hist, own_ge, null_max

    cols, value, thresholds = observed()
    hist, own_ge, null_max = Entry(cols, value, thresholds).results()
    eng = HipEngine()
    loop_s = []
    for k in range(warmup + timed):
        t0 = sync_time()
        b_hist, b_own, b_max = composed_null(eng, cols, value, thresholds)
        t = sync_time() - t0
        if k >= warmup:
            loop_s.append(t)
    assert torch.equal(b_hist, hist) and torch.equal(b_own, own_ge) and same_bits(b_max, null_max)
    print("(b) the same numbers from %d calls of covariation_wstat_scan (+ covariation_wstat_pairs) on rows shuffled with torch ops, + torch ops: "
          "median %.4f s (%s), equal to (a) in every count and maximum; peak device memory %.2f GB" % (
              K, med(loop_s), " ".join("%.4f" % t for t in loop_s), torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "unweighted":
    plain_rows = int(np.ceil(min_rows * R / weights.sum()))               # about as many observed pairs as the weighted scan
    plain = CovariationStatistics(sequences=seqs, statistic=statistic, correction=correction, minspan=minspan, min_rows=plain_rows, min_stat=min_stat)
    cols, value = plain.pair_cols.contiguous(), plain.value.contiguous()
    thresholds = torch.unique(value)
    P, U = int(value.numel()), int(thresholds.numel())
    batch = batch_of(lib.sq_covariation_stat_null_scratch)
    nbytes = int(lib.sq_covariation_stat_null_scratch(R, L, batch))
    scratch = new(nbytes // 8, torch.int64)
    hist, own_ge, null_max, out = new(U + 1, torch.int64), new(P, torch.int32), new(K, torch.float64), new(2, torch.int64)
    times = []
    for k in range(warmup + timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        _lib.check(lib.sq_covariation_stat_null(p(d_rows), R, L, stat, corr, minspan, p(cols if P else None), p(value if P else None), P,
                                                p(thresholds if U else None), U, K, seed, batch, p(scratch), nbytes, p(hist),
                                                p(own_ge if P else None), p(null_max), p(out), stream))
        ev[1].record()
        torch.cuda.synchronize()
        assert out.tolist() == [0, 0]
        if k >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    print("(c) the unweighted sq_covariation_stat_null between HIP events (min_rows %d, %d observed pairs, %d thresholds, %d samples a batch): "
          "median %.1f us (%s)" % (plain_rows, P, U, batch, med(times), " ".join("%.1f" % t for t in times)), flush=True)
