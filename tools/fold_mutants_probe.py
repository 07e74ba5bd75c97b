#!/usr/bin/env python3
"""One mutational scan of a random N-nt sequence (3 N variants), timed three ways:
 (a) the whole FoldMutants call, and sq_variant_diff alone between HIP events (buffers allocated before);
 (b) the same summary formed with torch ops on the device from the FoldResult;
 (c) the way without FoldMutants: Fold(records=wild type + variants), .cpu(), a numpy diff on the host.
The three summaries are asserted equal.  (a) and (c) alternate call by call; medians over the timed calls.
usage: fold_mutants_probe.py N [CONFIG] [WARMUP] [TIMED]"""
import ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import Fold, FoldMutants, _lib, fold_mutants as FM

N = int(sys.argv[1])
config = sys.argv[2] if len(sys.argv) > 2 else "nobpp"
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
timed = int(sys.argv[4]) if len(sys.argv) > 4 else 10
rng = random.Random(N)
seq = ''.join(rng.choice("ACGU") for _ in range(N))
record = (">probe", seq, None, None, None)


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def scan():
    """(a): (seconds of the call, of the Fold call inside it, the result)."""
    inner = {}
    fold = FM._fold.Fold

    def timed_fold(*a, **kw):
        t0 = sync_time()
        out = fold(*a, **kw)
        inner["fold"] = sync_time() - t0
        return out
    FM._fold.Fold = timed_fold
    try:
        t0 = sync_time()
        res = FoldMutants(records=[record], configfile=config)
        total = sync_time() - t0
    finally:
        FM._fold.Fold = fold
    return total, inner["fold"], res


def by_hand(recs):
    """(c): (seconds of Fold, of .cpu(), of the numpy diff, the summary)."""
    t0 = sync_time()
    folds = Fold(records=recs, configfile=config)
    t1 = sync_time()
    host = folds.cpu()
    t2 = time.perf_counter()
    V = len(recs) - 1
    diff, pos_changed = FM._host_diff(host, 1, np.zeros(V, np.int64), np.array([0, N], np.int64))
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, (diff, pos_changed)


def torch_summary(f, V):
    """(b): diff and pos_changed of one record's scan with torch ops on the rows' device."""
    t = torch.arange(N, device=f.device)
    w = f.partner[:N].long()                                              # (record 0 is the wild type, its row 0 comes first)
    v = f.partner[(f.cell_off[1:V + 1, None] + t[None, :])].long()
    up, changed = w > t, v != w
    some = changed.any(1)
    first = torch.where(some, changed.int().argmax(1), torch.full_like(some, -1, dtype=torch.int64))
    last = torch.where(some, N - 1 - changed.flip(1).int().argmax(1), torch.full_like(some, -1, dtype=torch.int64))
    diff = torch.stack(((up & changed).sum(1), ((v > t) & changed).sum(1), (up & ~changed).sum(1), changed.sum(1), first, last), 1)
    return diff.to(torch.int32), changed.sum(0).to(torch.int32)


a_total, a_fold, c_fold, c_cpu, c_diff = [], [], [], [], []
res = recs = None
for k in range(warmup + timed):
    total, fold_s, res = scan()
    if recs is None:
        recs = [record] + [(n, s, None, None, None) for n, s in zip(res.folds.names[1:], res.folds.sequences[1:])]
    f, h, d, by = by_hand(recs)
    assert by[0].tolist() == res.diff.tolist() and by[1].tolist() == res.pos_changed.tolist()
    if k >= warmup:
        a_total.append(total); a_fold.append(fold_s); c_fold.append(f); c_cpu.append(h); c_diff.append(d)
    print("call %d: FoldMutants %.4f s (Fold %.4f), by hand %.4f s" % (k, total, fold_s, f + h + d), flush=True)
V = len(res.folds) - 1
med = statistics.median
print("N %d config %s: %d variants, %d of them change the structure, source %s; %d warm-up, %d timed calls, medians" % (
    N, config, V, int((res.diff[:, 3] > 0).sum()), res.source, warmup, timed), flush=True)
print("(a) FoldMutants %.4f s: Fold %.4f s, the rest (variant records, uploads, sq_variant_diff, its two words read) %.4f s" % (
    med(a_total), med(a_fold), med([t - f for t, f in zip(a_total, a_fold)])), flush=True)

# sq_variant_diff alone: the two memsets and the kernel between two events, buffers allocated before
f = res.folds
wt_rec = torch.zeros(V, dtype=torch.int32, device=res.device)
diff = torch.empty((V, 6), dtype=torch.int32, device=res.device)
pos_changed = torch.empty(N, dtype=torch.int32, device=res.device)
out = torch.empty(2, dtype=torch.int64, device=res.device)
p = lambda x: ctypes.c_void_p(x.data_ptr())
stream = torch.cuda.current_stream()
kernel_us, torch_us = [], []
for k in range(warmup + timed):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_lib.load().sq_variant_diff(p(f.partner), p(f.cell_off), p(f.lengths), 1, V, p(wt_rec), p(res.pos_off), N, p(diff),
                                           p(pos_changed), p(out), ctypes.c_void_p(stream.cuda_stream)))
    e1.record()
    torch.cuda.synchronize()
    e2, e3 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e2.record()
    t_diff, t_pos = torch_summary(f, V)
    e3.record()
    torch.cuda.synchronize()
    if k >= warmup:
        kernel_us.append(e0.elapsed_time(e1) * 1e3); torch_us.append(e2.elapsed_time(e3) * 1e3)
assert out.tolist() == [0, 0] and diff.tolist() == res.diff.tolist() and pos_changed.tolist() == res.pos_changed.tolist()
assert t_diff.tolist() == res.diff.tolist() and t_pos.tolist() == res.pos_changed.tolist()
print("    sq_variant_diff between HIP events (two memsets + kernel): median %.1f us (%s)" % (
    med(kernel_us), " ".join("%.1f" % t for t in kernel_us)), flush=True)
print("(b) the same summary with torch ops on the device, between HIP events: median %.1f us (%s)" % (
    med(torch_us), " ".join("%.1f" % t for t in torch_us)), flush=True)
print("(c) by hand %.4f s: Fold(records=...) %.4f s, .cpu() %.4f s, numpy diff %.4f s; summaries equal" % (
    med([x + y + z for x, y, z in zip(c_fold, c_cpu, c_diff)]), med(c_fold), med(c_cpu), med(c_diff)), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
