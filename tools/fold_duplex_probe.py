#!/usr/bin/env python3
"""One interaction screen of T random N-nt targets against Q 21-nt queries (every other one the reverse complement of a
target's window), timed three ways:
 (a) the whole FoldDuplex call, and sq_duplex_summary alone between HIP events (buffers allocated before);
 (b) the same summary formed with torch ops on the device from the two FoldResults;
 (c) the way without FoldDuplex: Fold(records=solos), Fold(records=duplexes), .cpu(), a numpy summary on the host.
The three summaries are asserted equal.  (a) and (c) alternate call by call; medians over the timed calls.
usage: fold_duplex_probe.py T Q N [CONFIG] [WARMUP] [TIMED]"""
import ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import Fold, FoldDuplex, _lib, fold_duplex as FD

T, Q, N = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
config = sys.argv[4] if len(sys.argv) > 4 else "nobpp"
warmup = int(sys.argv[5]) if len(sys.argv) > 5 else 3
timed = int(sys.argv[6]) if len(sys.argv) > 6 else 10
W = min(21, N)
rng = random.Random(T * 1000003 + Q * 1009 + N)
letters = lambda n: ''.join(rng.choice("ACGU") for _ in range(n))
targets = [(">t%d" % a, letters(N), None, None, None) for a in range(T)]
queries = []
for q in range(Q):
    if q % 2:
        queries.append((">q%d" % q, letters(W), None, None, None))
    else:                                                                 # the reverse complement of a window of target q % T
        lo = rng.randint(0, N - W)
        window = targets[q % T][1][lo:lo + W]
        queries.append((">q%d" % q, ''.join({"A": "U", "C": "G", "G": "C", "U": "A"}[ch] for ch in reversed(window)), None, None, None))
P = T * Q


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def screen():
    """(a): (seconds of the call, of the two Fold calls inside it, the result)."""
    inner = []
    fold = FD._fold.Fold

    def timed_fold(*a, **kw):
        t0 = sync_time()
        out = fold(*a, **kw)
        inner.append(sync_time() - t0)
        return out
    FD._fold.Fold = timed_fold
    try:
        t0 = sync_time()
        res = FoldDuplex(targets=targets, queries=queries, configfile=config)
        total = sync_time() - t0
    finally:
        FD._fold.Fold = fold
    return total, sum(inner), res


def by_hand(srecs, drecs, a_rec, b_rec, pos_off):
    """(c): (seconds of the two Fold calls, of .cpu(), of the numpy summary, the summary)."""
    t0 = sync_time()
    solos, folds = Fold(records=srecs, configfile=config), Fold(records=drecs, configfile=config)
    t1 = sync_time()
    hs, hf = solos.cpu(), folds.cpu()
    t2 = time.perf_counter()
    summary, bound = FD._host_summary(hs, hf, a_rec, b_rec, pos_off)
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, (summary, bound)


def torch_summary(res):
    """(b): summary and bound of the screen with torch ops on the rows' device (every target N, every query W positions)."""
    s, f, dev = res.solos, res.folds, res.device
    n = N + 1 + W
    D = f.partner[f.cell_off[:P, None] + torch.arange(n, device=dev)[None, :]].long()
    A = s.partner[s.cell_off[:T, None] + torch.arange(N, device=dev)[None, :]].long()[res.a_rec.long()]
    B = s.partner[s.cell_off[T:T + Q, None] + torch.arange(W, device=dev)[None, :]].long()[res.b_rec.long() - T]
    Da, Db = D[:, :N], D[:, N + 1:]
    ta, tb, ub = torch.arange(N, device=dev), torch.arange(N + 1, n, device=dev), torch.arange(W, device=dev)
    inter_a, inter_b = Da > N, (Db >= 0) & (Db < N)

    def ends(hit, width):
        some = hit.any(1)
        none = torch.full_like(some, -1, dtype=torch.int64)
        return torch.where(some, hit.int().argmax(1), none), torch.where(some, width - 1 - hit.flip(1).int().argmax(1), none)
    cols = [inter_a.sum(1), ((Da > ta) & (Da < N)).sum(1), (Db > tb).sum(1), ((A > ta) & (Da != A)).sum(1),
            ((B > ub) & (Db != B + N + 1)).sum(1), *ends(inter_a, N), *ends(inter_b, W)]
    bound = torch.zeros(int(res.pos_off[-1]), dtype=torch.int32, device=dev)
    bound.index_add_(0, (res.pos_off[res.a_rec.long(), None] + ta[None, :]).reshape(-1), inter_a.reshape(-1).int())
    bound.index_add_(0, (res.pos_off[res.b_rec.long(), None] + ub[None, :]).reshape(-1), inter_b.reshape(-1).int())
    return torch.stack(cols, 1).to(torch.int32), bound


a_total, a_fold, c_fold, c_cpu, c_sum = [], [], [], [], []
res = srecs = None
for k in range(warmup + timed):
    total, fold_s, res = screen()
    if srecs is None:
        srecs = targets + queries
        drecs = [(n, s, None, None, None) for n, s in zip(res.folds.names, res.folds.sequences)]
        a_rec, b_rec, pos_off = res.a_rec.cpu().numpy().astype(np.int64), res.b_rec.cpu().numpy().astype(np.int64), res.pos_off.cpu().numpy()
    f, h, d, by = by_hand(srecs, drecs, a_rec, b_rec, pos_off)
    assert by[0].tolist() == res.summary.tolist() and by[1].tolist() == res.bound.tolist()
    if k >= warmup:
        a_total.append(total); a_fold.append(fold_s); c_fold.append(f); c_cpu.append(h); c_sum.append(d)
    print("call %d: FoldDuplex %.4f s (two Fold calls %.4f), by hand %.4f s" % (k, total, fold_s, f + h + d), flush=True)
med = statistics.median
print("T %d x Q %d, targets of %d nt, queries of %d nt, config %s: %d duplexes, %d of them with an inter-chain pair, %d open a pair of a "
      "partner, source %s; %d warm-up, %d timed calls, medians" % (T, Q, N, W, config, P, int((res.summary[:, 0] > 0).sum()),
                                                                  int((res.disruption() > 0).sum()), res.source, warmup, timed), flush=True)
print("(a) FoldDuplex %.4f s: the two Fold calls %.4f s, the rest (duplex records, uploads, sq_duplex_summary, its two words read) %.4f s" % (
    med(a_total), med(a_fold), med([t - f for t, f in zip(a_total, a_fold)])), flush=True)

# sq_duplex_summary alone: the two memsets and the kernel between two events, buffers allocated before
s, f = res.solos, res.folds
Ltot = int(pos_off[-1])
summary = torch.empty((P, 9), dtype=torch.int32, device=res.device)
bound = torch.empty(Ltot, dtype=torch.int32, device=res.device)
out = torch.empty(2, dtype=torch.int64, device=res.device)
p = lambda x: ctypes.c_void_p(x.data_ptr())
stream = torch.cuda.current_stream()
kernel_us, torch_us = [], []
for k in range(warmup + timed):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_lib.load().sq_duplex_summary(p(s.partner), p(s.cell_off), p(s.lengths), T + Q, p(f.partner), p(f.cell_off), p(f.lengths), P,
                                             p(res.a_rec), p(res.b_rec), p(res.pos_off), Ltot, p(summary), p(bound), p(out),
                                             ctypes.c_void_p(stream.cuda_stream)))
    e1.record()
    torch.cuda.synchronize()
    e2, e3 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e2.record()
    t_summary, t_bound = torch_summary(res)
    e3.record()
    torch.cuda.synchronize()
    if k >= warmup:
        kernel_us.append(e0.elapsed_time(e1) * 1e3); torch_us.append(e2.elapsed_time(e3) * 1e3)
assert out.tolist() == [0, 0] and summary.tolist() == res.summary.tolist() and bound.tolist() == res.bound.tolist()
assert t_summary.tolist() == res.summary.tolist() and t_bound.tolist() == res.bound.tolist()
print("    sq_duplex_summary between HIP events (two memsets + kernel): median %.1f us (%s)" % (
    med(kernel_us), " ".join("%.1f" % t for t in kernel_us)), flush=True)
print("(b) the same summary with torch ops on the device, between HIP events: median %.1f us (%s)" % (
    med(torch_us), " ".join("%.1f" % t for t in torch_us)), flush=True)
print("(c) by hand %.4f s: the two Fold(records=...) %.4f s, .cpu() %.4f s, numpy summary %.4f s; summaries equal" % (
    med([x + y + z for x, y, z in zip(c_fold, c_cpu, c_sum)]), med(c_fold), med(c_cpu), med(c_sum)), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
