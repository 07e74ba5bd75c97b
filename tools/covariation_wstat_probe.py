#!/usr/bin/env python3
"""The weighted covariation statistics of one random alignment of R rows and L columns with planted helices
(covariation_stat_probe.py's alignment) and row weights 1 / k, k drawn from 1 .. 8 per row, timed three ways:
 (a) the whole CovariationStatistics(weights=) call, and sq_covariation_wstat_scan alone between HIP events (buffers allocated
     before), with the unweighted sq_covariation_stat_scan at the same shape and thresholds beside it;
 (b) the same numbers with torch ops on the device: one-hot float64 matrix products per cell of the joint table (exact: the
     sums stay below 2^53), S cell by cell in float64, the means, C, the thresholds, nonzero; Q is asserted equal to the entry's;
 (c) the rows and weights downloaded and the same numbers with numpy (the same array code).
The results are compared with the call's: the same cells but for values within 1e-9 of the threshold, the same Q, raw and value
within 1e-9 * (1 + |value|).  Best and median over the timed calls.  Every step that uses the GPU is a process of its own under
its own time limit; the first that fails ends the probe.
usage: covariation_wstat_probe.py R L [statistic] [correction] [MIN_STAT] [WARMUP] [TIMED] [MIN_ROWS]
       (defaults: gt apc 20 2 5 R / 8; correction "none" for None; MIN_STAT "none" for None; minspan stays 4)"""
import ctypes, os, random, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("entries", 300), ("torch", 300), ("numpy", 600))                 # (step, its time limit in seconds)

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
from squarna_amd import CovariationStatistics, _lib, covariation as CV
from squarna_amd.device_calls import COVAR_CORRECTIONS, COVAR_STATISTICS, COVAR_WSTAT_ONE as ONE

step = sys.argv[sys.argv.index("--step") + 1]
args = sys.argv[1:sys.argv.index("--step")]
R, L = int(args[0]), int(args[1])
statistic = args[2] if len(args) > 2 else "gt"
correction = (None if args[3] == "none" else args[3]) if len(args) > 3 else "apc"
min_stat = (None if args[4] == "none" else float(args[4])) if len(args) > 4 else 20.0
floor = float("-inf") if min_stat is None else min_stat      # what the entries and the array forms take
warmup = int(args[5]) if len(args) > 5 else 2
timed = int(args[6]) if len(args) > 6 else 5
min_rows = float(args[7]) if len(args) > 7 else R / 8
minspan = 4
stat, corr = COVAR_STATISTICS.index(statistic), COVAR_CORRECTIONS.index(correction)
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
show = lambda ts: "best %.1f us, median %.1f us (%s)" % (min(ts), statistics.median(ts), " ".join("%.1f" % t for t in ts))


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def table(xp, cls, q, as_double, where, arange):
    """(flat, Q, raw, value) sorted by flat index with the array module xp (torch on the device, or numpy): q = the quantised
    weights as float64; one-hot float64 matrix products per cell of the table, S cell by cell, the means, C, the thresholds."""
    hot = [as_double(cls == k) for k in range(4)]
    Q = [hot[a].T @ (hot[b] * q[:, None]) for a in range(4) for b in range(4)]
    n = [x / ONE for x in Q]
    na = [(Q[4 * a] + Q[4 * a + 1] + Q[4 * a + 2] + Q[4 * a + 3]) / ONE for a in range(4)]
    nb = [(Q[b] + Q[4 + b] + Q[8 + b] + Q[12 + b]) / ONE for b in range(4)]
    N = (Q[0] + Q[1] + Q[2] + Q[3] + Q[4] + Q[5] + Q[6] + Q[7] + Q[8] + Q[9] + Q[10] + Q[11] + Q[12] + Q[13] + Q[14] + Q[15]) / ONE
    S = N * 0.0
    for k in range(16):
        m = na[k >> 2] * nb[k & 3]
        if statistic == "chi":
            e = m / N
            S += where(m > 0, (n[k] - e) * (n[k] - e) / e)
        else:
            S += where(n[k] > 0, (n[k] / N if statistic == "mi" else n[k]) * xp.log(n[k] * N / m))
    S = where(N > 0, S) * (2.0 if statistic == "gt" else 1.0)
    C = S
    if correction is not None:
        upper = xp.triu(S, 1)
        mean = (upper + upper.T).sum(1) / (L - 1)
        mean_all = upper.sum() / (L * (L - 1) // 2)
        C = S - mean[:, None] * mean[None, :] / mean_all if correction == "apc" else S - (mean[:, None] + mean[None, :] - mean_all)
    span = arange[None, :] - arange[:, None]
    at = xp.nonzero((span >= minspan) & (N >= min_rows) & (C >= floor))
    at = (at[:, 0], at[:, 1]) if xp is torch else at
    return at[0] * L + at[1], xp.stack([x[at] for x in Q], 1), S[at], C[at]


def same(name, flat, Q, raw, value, ref):
    """The result against the call's: the cells but for values at the threshold, Q exactly, raw and value."""
    flat_ref = ref.pair_cols[:, 0].long() * L + ref.pair_cols[:, 1].long()
    both = np.intersect1d(flat.cpu().numpy(), flat_ref.cpu().numpy())
    a, b = torch.isin(flat, torch.from_numpy(both).to(flat.device)), torch.isin(flat_ref, torch.from_numpy(both).to(flat_ref.device))
    edge = lambda v: min_stat is not None and bool(((v - min_stat).abs() <= 1e-9 * (1 + abs(min_stat))).all()) or not v.numel()
    assert edge(value[~a]) and edge(ref.value[~b]), name
    assert torch.equal(Q[a].to(ref.joint.device).double(), ref.joint[b] * ONE), name
    for got, exp in ((raw[a], ref.raw[b]), (value[a], ref.value[b])):
        assert bool(((got.to(exp.device) - exp).abs() <= 1e-9 * (1 + exp.abs())).all()), name
    return int((~a).sum()) + int((~b).sum())


call = lambda: CovariationStatistics(sequences=seqs, weights=d_weights, statistic=statistic, correction=correction, minspan=minspan,
                                     min_rows=min_rows, min_stat=min_stat)
dev = torch.device("cuda", torch.cuda.current_device())
d_weights = torch.from_numpy(weights).to(dev)
d_rows = torch.from_numpy(np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).reshape(R, L).copy()).to(dev)

if step == "entries":
    a_total = []
    for k in range(warmup + timed):
        t0 = sync_time()
        res = call()
        t = sync_time() - t0
        if k >= warmup:
            a_total.append(t)
    assert res.source == "device" and res.mode == "scan"
    P = len(res)
    print("R %d x L %d, %d planted helices, weights 1 / k (their sum %.1f), %s / %s, minspan %d, min_rows %g, min_stat %s: %d of %d cells emitted; "
          "%d warm-up, %d timed calls" % (R, L, helices, weights.sum(), statistic, correction, minspan, min_rows, min_stat, P, L * (L - 1) // 2,
                                          warmup, timed), flush=True)
    print("(a) CovariationStatistics(weights=) (rows to bytes, upload, planes, weights, pass 1, pass 2, sort by cell): best %.6f s, median %.6f s" % (
        min(a_total), statistics.median(a_total)), flush=True)
    lib = _lib.load()
    nbytes, plain_bytes = int(lib.sq_covariation_wstat_scratch(R, L)), int(lib.sq_covariation_stat_scratch(R, L))
    cap = max(P, 1)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    mean = torch.empty(L + 1, dtype=torch.float64, device=dev)
    flat, Q = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty((cap, 16), dtype=torch.int64, device=dev)
    raw, value = torch.empty(cap, dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)
    plain_rows = int(np.ceil(min_rows * R / weights.sum()))                # the unweighted entry: about as many cells emitted
    plain = CovariationStatistics(sequences=seqs, statistic=statistic, correction=correction, minspan=minspan, min_rows=plain_rows, min_stat=min_stat)
    p_cap = max(len(plain), 1)
    p_flat, p_joint = torch.empty(p_cap, dtype=torch.int64, device=dev), torch.empty((p_cap, 16), dtype=torch.int32, device=dev)
    p_raw, p_value = torch.empty(p_cap, dtype=torch.float64, device=dev), torch.empty(p_cap, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.int64, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    entries = {
        "planes + weights": lambda: lib.sq_covariation_wstat_pairs(p(d_rows), R, L, p(d_weights), stat, 0, None, 0, p(scratch), nbytes, None,
                                                                   None, None, None, p(out), stream),
        "planes + weights + pass 1 + reductions": lambda: lib.sq_covariation_wstat_pairs(p(d_rows), R, L, p(d_weights), stat, corr or 1, None, 0,
                                                                                         p(scratch), nbytes, p(mean), None, None, None, p(out), stream),
        "sq_covariation_wstat_scan": lambda: lib.sq_covariation_wstat_scan(p(d_rows), R, L, p(d_weights), stat, corr, minspan, min_rows, floor,
                                                                          p(scratch), nbytes, p(mean), p(flat), p(Q), p(raw), p(value), cap, p(out),
                                                                          stream),
        "sq_covariation_stat_scan (unweighted, min_rows %d, %d cells emitted)" % (plain_rows, len(plain)): lambda: lib.sq_covariation_stat_scan(
            p(d_rows), R, L, stat, corr, minspan, plain_rows, floor, p(scratch), plain_bytes, p(mean), p(p_flat), p(p_joint), p(p_raw), p(p_value),
            p_cap, p(out), stream),
    }
    times = {name: [] for name in entries}
    for k in range(warmup + timed):
        for name, entry in entries.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            _lib.check(entry())
            ev[1].record()
            torch.cuda.synchronize()
            if k >= warmup:
                times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)
            if name == "sq_covariation_wstat_scan":
                assert out.tolist() == [P, 0]
    order = torch.argsort(flat[:P])
    assert same("entry", flat[:P][order], Q[:P][order], raw[:P][order], value[:P][order], res) == 0
    assert torch.equal(raw[:P][order], res.raw) and torch.equal(value[:P][order], res.value)           # two calls: the same bits
    for name in entries:
        print("    %s between HIP events: %s" % (name, show(times[name])), flush=True)
    names = list(entries)
    print("    weighted / unweighted entry (bests): %.2f; pass 1 + reductions alone (difference of the bests): %.1f us; scratch %d bytes" % (
        min(times[names[2]]) / min(times[names[3]]), min(times[names[1]]) - min(times[names[0]]), nbytes), flush=True)
    print("    peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "torch":
    res = call()
    lut = torch.from_numpy(CV._classes(np.arange(256, dtype=np.uint8))).to(dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    times = []
    for k in range(warmup + timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        q = torch.round(d_weights * ONE)                                 # (ties to even)
        got = table(torch, lut[d_rows.long()], q, lambda m: m.double(), lambda c, x: torch.where(c, x, zero), torch.arange(L, device=dev))
        ev[1].record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    edge_cells = same("torch", *got, res)
    print("(b) the same numbers with torch ops on the device, between HIP events: %s; Q equal; %d cells at the threshold differ; peak device memory %.2f GB" % (
        show(times), edge_cells, torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "numpy":
    res = call().cpu()
    c_down, c_np = [], []
    for k in range(min(timed, 2)):
        t0 = sync_time()
        host, host_weights = d_rows.cpu().numpy(), d_weights.cpu().numpy()
        t1 = time.perf_counter()
        with np.errstate(divide="ignore", invalid="ignore"):
            got = table(np, CV._classes(host), np.rint(host_weights * ONE), lambda m: m.astype(np.float64), lambda c, x: np.where(c, x, 0.0), np.arange(L))
        c_down.append(t1 - t0); c_np.append(time.perf_counter() - t1)
    edge_cells = same("numpy", *(torch.from_numpy(x) for x in got), res)
    print("(c) download best %.6f s + numpy best %.3f s; %d cells at the threshold differ" % (min(c_down), min(c_np), edge_cells), flush=True)
