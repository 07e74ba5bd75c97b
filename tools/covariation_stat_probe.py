#!/usr/bin/env python3
"""The covariation statistics of one random alignment of R rows and L columns with planted helices (covariation_probe.py's
alignment), timed three ways:
 (a) the whole CovariationStatistics call, and the entries alone between HIP events (buffers allocated before): the planes
     alone (sq_covariation_stat_pairs with no pair and no correction), the planes with pass 1 and the two reductions (the
     same with a correction), the planes with pass 2 (sq_covariation_stat_scan without a correction) and the whole
     sq_covariation_stat_scan; pass 1 and pass 2 alone are the differences to the planes;
 (b) the same numbers with torch ops on the device: one-hot matrix products per cell of the joint table, S cell by cell in
     float64, the means, C, the thresholds, nonzero;
 (c) the rows downloaded and the same numbers with numpy (the same array code; float64 matrix products).
The three results are compared: the same cells but for values within 1e-9 of the threshold, the same counters, raw and value
within 1e-9 * (1 + |value|).  Best and median over the timed calls.
usage: covariation_stat_probe.py R L [statistic] [correction] [MIN_STAT] [WARMUP] [TIMED] [MIN_ROWS]
       (defaults: gt apc 20 2 5 R // 2; correction "none" for None; MIN_STAT "none" for None: every cell with MIN_ROWS rows
       is a record; minspan stays 4)"""
import ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import CovariationStatistics, _lib, covariation as CV
from squarna_amd.device_calls import COVAR_CORRECTIONS, COVAR_STATISTICS

R, L = int(sys.argv[1]), int(sys.argv[2])
statistic = sys.argv[3] if len(sys.argv) > 3 else "gt"
correction = (None if sys.argv[4] == "none" else sys.argv[4]) if len(sys.argv) > 4 else "apc"
min_stat = (None if sys.argv[5] == "none" else float(sys.argv[5])) if len(sys.argv) > 5 else 20.0
floor = float("-inf") if min_stat is None else min_stat      # what the entries and the array forms take
warmup = int(sys.argv[6]) if len(sys.argv) > 6 else 2
timed = int(sys.argv[7]) if len(sys.argv) > 7 else 5
min_rows = int(sys.argv[8]) if len(sys.argv) > 8 else R // 2
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
show = lambda ts: "best %.1f us, median %.1f us (%s)" % (min(ts), statistics.median(ts), " ".join("%.1f" % t for t in ts))


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def table(xp, cls, as_float, as_double, where, arange):
    """(flat, joint, raw, value) sorted by flat index with the array module xp (torch on the device, or numpy): one-hot matrix
    products per cell of the joint table, S cell by cell in float64, the means, C, the thresholds, nonzero."""
    hot = [as_float(cls == k) for k in range(4)]
    n = [as_double(hot[a].T @ hot[b]) for a in range(4) for b in range(4)]
    na = [n[4 * a] + n[4 * a + 1] + n[4 * a + 2] + n[4 * a + 3] for a in range(4)]
    nb = [n[b] + n[4 + b] + n[8 + b] + n[12 + b] for b in range(4)]
    N = na[0] + na[1] + na[2] + na[3]
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
    return at[0] * L + at[1], xp.stack([x[at] for x in n], 1), S[at], C[at]


def torch_table(d_rows, lut):
    """(b): float32 products of 0 / 1 (exact below 2^24 rows), the rest in float64."""
    zero = torch.zeros((), dtype=torch.float64, device=d_rows.device)
    flat, joint, raw, value = table(torch, lut[d_rows.long()], lambda m: m.float(), lambda m: m.double(), lambda c, x: torch.where(c, x, zero),
                                    torch.arange(L, device=d_rows.device))
    return flat, joint.int(), raw, value


def numpy_table(host):
    """(c): float64 products (exact at these sizes, and BLAS)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        flat, joint, raw, value = table(np, CV._classes(host), lambda m: m.astype(np.float64), lambda m: m, lambda c, x: np.where(c, x, 0.0),
                                        np.arange(L))
    return torch.from_numpy(flat), torch.from_numpy(joint.astype(np.int32)), torch.from_numpy(raw), torch.from_numpy(value)


def same(name, flat, joint, raw, value, ref):
    """The result against the call's: the cells but for values at the threshold, the counters, raw and value."""
    flat_ref = ref.pair_cols[:, 0].long() * L + ref.pair_cols[:, 1].long()
    both = np.intersect1d(flat.cpu().numpy(), flat_ref.cpu().numpy())
    a, b = torch.isin(flat, torch.from_numpy(both).to(flat.device)), torch.isin(flat_ref, torch.from_numpy(both).to(flat_ref.device))
    edge = lambda v: min_stat is not None and bool(((v - min_stat).abs() <= 1e-9 * (1 + abs(min_stat))).all()) or not v.numel()
    assert edge(value[~a]) and edge(ref.value[~b]), name
    assert torch.equal(joint[a].to(ref.joint.device), ref.joint[b]), name
    for got, exp in ((raw[a], ref.raw[b]), (value[a], ref.value[b])):
        assert bool(((got.to(exp.device) - exp).abs() <= 1e-9 * (1 + exp.abs())).all()), name
    return int((~a).sum()) + int((~b).sum())


# ---- (a) the whole call
a_total = []
for k in range(warmup + timed):
    t0 = sync_time()
    res = CovariationStatistics(sequences=seqs, statistic=statistic, correction=correction, minspan=minspan, min_rows=min_rows, min_stat=min_stat)
    t = sync_time() - t0
    if k >= warmup:
        a_total.append(t)
assert res.source == "device" and res.mode == "scan"
P = len(res)
print("R %d x L %d, %d planted helices, %s / %s, minspan %d, min_rows %d, min_stat %s: %d of %d cells emitted; %d warm-up, %d timed calls" % (
    R, L, helices, statistic, correction, minspan, min_rows, min_stat, P, L * (L - 1) // 2, warmup, timed), flush=True)
print("(a) CovariationStatistics (rows to bytes, upload, planes, pass 1, pass 2, sort by cell): best %.6f s, median %.6f s" % (
    min(a_total), statistics.median(a_total)), flush=True)

# ---- the entries alone and (b), between HIP events with buffers allocated before
lib = _lib.load()
dev = res.device
d_rows = torch.from_numpy(np.frombuffer("".join(seqs).encode("latin-1"), np.uint8).reshape(R, L).copy()).to(dev)
lut = torch.from_numpy(CV._classes(np.arange(256, dtype=np.uint8))).to(dev)
nbytes = int(lib.sq_covariation_stat_scratch(R, L))
cap = max(P, 1)
scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
mean = torch.empty(L + 1, dtype=torch.float64, device=dev)
flat, joint = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty((cap, 16), dtype=torch.int32, device=dev)
raw, value = torch.empty(cap, dtype=torch.float64, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)
out = torch.empty(2, dtype=torch.int64, device=dev)
p = lambda x: ctypes.c_void_p(x.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
entries = {
    "planes": lambda: lib.sq_covariation_stat_pairs(p(d_rows), R, L, stat, 0, None, 0, p(scratch), nbytes, None, None, None, None, p(out), stream),
    "planes + pass 1 + reductions": lambda: lib.sq_covariation_stat_pairs(p(d_rows), R, L, stat, corr or 1, None, 0, p(scratch), nbytes, p(mean),
                                                                         None, None, None, p(out), stream),
    "planes + pass 2 (no correction)": lambda: lib.sq_covariation_stat_scan(p(d_rows), R, L, stat, 0, minspan, min_rows, floor, p(scratch), nbytes,
                                                                           None, p(flat), p(joint), p(raw), p(value), cap, p(out), stream),
    "sq_covariation_stat_scan": lambda: lib.sq_covariation_stat_scan(p(d_rows), R, L, stat, corr, minspan, min_rows, floor, p(scratch), nbytes,
                                                                    p(mean), p(flat), p(joint), p(raw), p(value), cap, p(out), stream),
}
times = {name: [] for name in entries}
times["torch"] = []
for k in range(warmup + timed):
    for name, call in list(entries.items()) + [("torch", None)]:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        if call is None:
            t_flat, t_joint, t_raw, t_value = torch_table(d_rows, lut)
        else:
            _lib.check(call())
        ev[1].record()
        torch.cuda.synchronize()
        if k >= warmup:
            times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)
assert out.tolist() == [P, 0]
order = torch.argsort(flat[:P])
assert same("entry", flat[:P][order], joint[:P][order], raw[:P][order], value[:P][order], res) == 0
assert torch.equal(raw[:P][order], res.raw) and torch.equal(value[:P][order], res.value)           # two calls: the same bits
edge_cells = same("torch", t_flat, t_joint, t_raw, t_value, res)
del t_flat, t_joint, t_raw, t_value
for name in entries:
    print("    %s between HIP events: %s" % (name, show(times[name])), flush=True)
print("    pass 1 + reductions alone (difference of the bests): %.1f us; pass 2 alone: %.1f us; scratch %d bytes" % (
    min(times["planes + pass 1 + reductions"]) - min(times["planes"]), min(times["planes + pass 2 (no correction)"]) - min(times["planes"]), nbytes), flush=True)
print("(b) the same numbers with torch ops on the device, between HIP events: %s; %d cells at the threshold differ" % (show(times["torch"]), edge_cells), flush=True)

# ---- (c) download + numpy
c_down, c_np = [], []
for k in range(min(timed, 2)):
    t0 = sync_time()
    host = d_rows.cpu().numpy()
    t1 = time.perf_counter()
    h = numpy_table(host)
    c_down.append(t1 - t0); c_np.append(time.perf_counter() - t1)
edge_cells = same("numpy", *h, res.cpu())
print("(c) download best %.6f s + numpy best %.3f s; %d cells at the threshold differ" % (min(c_down), min(c_np), edge_cells), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
