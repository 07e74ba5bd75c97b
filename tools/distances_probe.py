#!/usr/bin/env python3
"""The base-pair distances of S random structures of W columns in groups of GROUP rows (S / 100 families of near-duplicates: a
random nested founder with up to three pairs removed, so that identical and close structures occur), at radius 2, timed three
ways:
 (a) the whole Distances call, sq_structure_distances alone between HIP events (buffers allocated before), and each of its
     three kernels alone (sq_structure_distances_phases on the buffers the whole call left); the filter's cost per row;
 (b) the same numbers with torch ops on the device: the pairs as keys i * W + j, a 0 / 1 incidence matrix of the rows over the
     distinct keys, one float32 matrix product (exact: sums below 2^24), the distances, the neighbour test, the group mask and
     the counts -- no filter;
 (c) the partner rows downloaded and the same numbers, filter included, with numpy (Distances' own fallback).
The outputs are asserted equal.  Best and median over the timed calls.  Every step that uses the GPU is a process of its own
under its own time limit; the first that fails ends the probe.
usage: distances_probe.py S W [GROUP] [WARMUP] [TIMED]      (defaults: one group, 2, 5)"""
import ctypes, os, random, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("entries", 300), ("torch", 300), ("numpy", 900))                 # (step, its time limit in seconds)

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
from squarna_amd import Distances, _lib
from squarna_amd import distances as D
from squarna_amd.rows import offsets

step = sys.argv[sys.argv.index("--step") + 1]
args = sys.argv[1:sys.argv.index("--step")]
S, W = int(args[0]), int(args[1])
group = int(args[2]) if len(args) > 2 else S
warmup = int(args[3]) if len(args) > 3 else 2
timed = int(args[4]) if len(args) > 4 else 5
RADIUS = 2
if S < 1 or W < 1 or group < 1 or S % group:
    sys.exit("S is a multiple of GROUP")
rng = random.Random(S * 100003 + W)


def founder():
    row, stack = [-1] * W, []
    for c in range(W):
        x = rng.random()
        if x < 0.3:
            stack.append(c)
        elif x < 0.6 and stack:
            o = stack.pop()
            row[o], row[c] = c, o
    return row


founders = [founder() for _ in range(max(S // 100, 1))]
partner = np.empty((S, W), np.int32)
for q in range(S):
    row = list(rng.choice(founders))
    opens = [c for c in range(W) if row[c] > c]
    for c in rng.sample(opens, min(rng.randrange(4), len(opens))):
        row[row[c]], row[c] = -1, -1
    partner[q] = row
sizes = np.full(S // group, group, np.int64)
group_off = offsets(sizes)
G = len(sizes)
show = lambda ts: "best %.1f us, median %.1f us (%s)" % (min(ts), statistics.median(ts), " ".join("%.1f" % t for t in ts))
dev = torch.device("cuda", torch.cuda.current_device())
d_partner = torch.from_numpy(partner.reshape(G, group, W)).to(dev)
call = lambda: Distances(d_partner, radius=RADIUS)


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


if step == "entries":
    a_total = []
    for k in range(warmup + timed):
        t0 = sync_time()
        res = call()
        t = sync_time() - t0
        if k >= warmup:
            a_total.append(t)
    assert res.source == "device" and res.S == S and res.G == G
    tiles = D.plan_tiles(group_off)
    T = len(tiles)
    print("S %d x W %d in %d groups of %d, %d families, radius %d: %d planned tiles of %d, matrix %s, %d rows kept, mean neighbours %.2f; "
          "%d warm-up, %d timed calls" % (S, W, G, group, len(founders), RADIUS, T, (S + 63) // 64 * ((S + 63) // 64 + 1) // 2,
                                          "on" if res.common is not None else "off", int(res.keep.sum()), float(res.neighbours.double().mean()),
                                          warmup, timed), flush=True)
    print("(a) Distances (the tables up, the three kernels, the result words) best %.6f s, median %.6f s" % (min(a_total), statistics.median(a_total)),
          flush=True)
    lib = _lib.load()
    nbytes = int(lib.sq_structure_distances_scratch(S, W, T))
    matrix = res.common is not None
    cells = int(res.mat_off[-1]) if matrix else 0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    flat = d_partner.reshape(-1)
    t_start, t_width = up(np.arange(S, dtype=np.int64) * W), up(np.full(S, W, np.int32))
    t_group, t_goff, t_moff, t_tiles = up(np.repeat(np.arange(G, dtype=np.int32), sizes)), up(group_off.astype(np.int32)), up(offsets(sizes * sizes)), up(tiles)
    new = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=dev)
    scratch, status, npairs, common = new(nbytes // 8, torch.int64), new(S, torch.int32), new(S, torch.int32), new(cells, torch.int32)
    nb, leader, keep, out = new(S, torch.int32), new(S, torch.int32), new(S, torch.uint8), new(2, torch.int64)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = (p(flat), S * W, p(t_start), p(t_width), p(t_group), S, W, p(t_goff), p(t_moff), G, int(sizes.max()), p(t_tiles), T, 0, RADIUS, p(scratch),
            nbytes, p(status), p(npairs), p(common) if matrix else None, cells, p(nb), p(leader), p(keep), p(out), stream)
    entries = {"sq_structure_distances (3 memsets + 3 kernels)": lambda: lib.sq_structure_distances(*tail),
               "planes kernel": lambda: lib.sq_structure_distances_phases(1, *tail),
               "pairs kernel (with its memsets)": lambda: lib.sq_structure_distances_phases(2, *tail),
               "filter kernel": lambda: lib.sq_structure_distances_phases(4, *tail)}
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
            assert out.tolist() == [0, 0]
    for got, exp in ((status, res.status), (npairs, res.npairs), (nb, res.neighbours), (leader, res.leader), (keep.bool(), res.keep)):
        assert torch.equal(got[:S], exp)
    assert not matrix or torch.equal(common[:cells], res.common)
    for name in entries:
        print("    %s between HIP events: %s" % (name, show(times[name])), flush=True)
    names = list(entries)
    whole = min(times[names[0]])
    print("    shares of the whole (bests): planes %.1f %%, pairs %.1f %%, filter %.1f %%; the filter costs %.3f us a row; scratch %d bytes" % (
        100 * min(times[names[1]]) / whole, 100 * min(times[names[2]]) / whole, 100 * min(times[names[3]]) / whole, min(times[names[3]]) / S, nbytes),
        flush=True)
    print("    peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "torch":
    res = call()
    rows_group = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(sizes).to(dev))
    times = []
    for k in range(warmup + timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        p2 = d_partner.reshape(S, W).long()
        cols = torch.arange(W, device=dev)
        opening = p2 > cols[None, :]
        at = opening.nonzero()
        uniq, col = torch.unique(at[:, 1] * W + p2[opening], return_inverse=True)
        inc = torch.zeros((S, max(int(uniq.numel()), 1)), dtype=torch.float32, device=dev)
        inc[at[:, 0], col] = 1
        common = (inc @ inc.T).long()
        n = opening.sum(1)
        near = D._near(0, RADIUS, n[:, None], n[None, :], common) & (rows_group[:, None] == rows_group[None, :])
        near.fill_diagonal_(False)
        neighbours = 1 + near.sum(1)
        ev[1].record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    assert torch.equal(n.int(), res.npairs) and torch.equal(neighbours.int(), res.neighbours)
    if res.common is not None:
        for g in range(0, G, max(G // 16, 1)):
            a, b = int(group_off[g]), int(group_off[g + 1])
            assert torch.equal(common[a:b, a:b], res.common_of(g))
    print("(b) the same numbers with torch ops on the device (no filter), between HIP events: %s; npairs, neighbours%s equal; peak device memory %.2f GB" % (
        show(times), " and common" if res.common is not None else "", torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "numpy":
    res = call().cpu()
    c_down, c_np = [], []
    for k in range(1):
        t0 = sync_time()
        host = d_partner.cpu().numpy().reshape(-1)
        t1 = time.perf_counter()
        got = D._host_distances(host, np.arange(S, dtype=np.int64) * W, np.full(S, W, np.int32), group_off, 0, RADIUS, res.common is not None)
        c_down.append(t1 - t0); c_np.append(time.perf_counter() - t1)
    for key, value in got.items():
        assert value is None and getattr(res, key) is None or torch.equal(torch.from_numpy(value), getattr(res, key)), key
    print("(c) download %.6f s + numpy (filter included) %.3f s, once; every output equal" % (min(c_down), min(c_np)), flush=True)
