#!/usr/bin/env python3
"""K shared structure lines over the L columns of R random aligned rows (a fifth of the cells gaps) projected onto the rows,
and the projected lines lifted back onto the columns, timed three ways:
 (a) the whole Project and Lift calls, and sq_project_rows / sq_lift_rows alone between HIP events (buffers allocated before),
     with the bytes they read and write and the rate that makes;
 (b) the same tensors with torch ops on the device: the classes through a lookup tensor, the gap map from cumsum, the pairs
     and the lift through gather and scatter -- asserted equal;
 (c) the step lines and nothing else downloaded (.cpu()) and a dbn.UnAlign loop over every row and line on the host; the pairs
     of every 97th row are compared with Project's.
Best and median over the timed calls.  Every step that uses the GPU is a process of its own under its own time limit; the
first that fails ends the probe.
usage: project_probe.py R L [K] [WARMUP] [TIMED]      (defaults: 3, 2, 5)"""
import ctypes, os, random, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("entries", 300), ("torch", 300), ("unalign", 900))               # (step, its time limit in seconds)

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
from squarna_amd import Lift, Project, _lib, dbn
from squarna_amd import project as P

step = sys.argv[sys.argv.index("--step") + 1]
args = sys.argv[1:sys.argv.index("--step")]
R, L = int(args[0]), int(args[1])
K = int(args[2]) if len(args) > 2 else 3
warmup = int(args[3]) if len(args) > 3 else 2
timed = int(args[4]) if len(args) > 4 else 5
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12                                   # bytes / s: a float4 copy on an MI355X, and the data sheet
rng = random.Random(R * 100003 + L)
np_rng = np.random.default_rng(R * 100003 + L)
letters = np.frombuffer(b"ACGUacguTN", np.uint8)
rows = letters[np_rng.integers(0, len(letters), (R, L))]
rows[np_rng.random((R, L)) < 0.2] = ord("-")
seqs = [bytes(r).decode() for r in rows]


def line():
    row, stack = [-1] * L, []
    for c in range(L):
        x = rng.random()
        if x < 0.3:
            stack.append(c)
        elif x < 0.6 and stack:
            o = stack.pop()
            row[o], row[c] = c, o
    return row


lines = np.array([line() for _ in range(K)], np.int32)
show = lambda ts: "best %.1f us, median %.1f us (%s)" % (min(ts), statistics.median(ts), " ".join("%.1f" % t for t in ts))
dev = torch.device("cuda", torch.cuda.current_device())
d_lines = torch.from_numpy(lines).to(dev)
d_rows = torch.from_numpy(rows.copy()).to(dev)


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def between_events(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3, out


if step == "entries":
    totals = {"Project": [], "Lift": []}
    for k in range(warmup + timed):
        t0 = sync_time()
        res = Project(sequences=seqs, structures=d_lines)
        t1 = sync_time()
        lifted = Lift(sequences=seqs, structures=res.partner)
        t2 = sync_time()
        if k >= warmup:
            totals["Project"].append(t1 - t0)
            totals["Lift"].append(t2 - t1)
    assert res.source == lifted.source == "device"
    Lmax = int(res.partner.shape[2])
    print("R %d x L %d, K %d shared lines of %s pairs, Lmax %d, kept pairs a row and line %.1f; %d warm-up, %d timed calls" % (
        R, L, K, (lines > np.arange(L)).sum(1).tolist(), Lmax, float(res.counts[..., 11].double().mean()), warmup, timed), flush=True)
    for name, ts in totals.items():
        print("(a) %s (the rows classed on the host for Lmax, the rows up, the kernel, the status read) best %.6f s, median %.6f s" % (
            name, min(ts), statistics.median(ts)), flush=True)
    lib = _lib.load()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(length=new(R, torch.int32), col_of=new((R, Lmax), torch.int32), pos_of=new((R, L), torch.int32), partner=new((R, K, Lmax), torch.int32),
               cls=new((R, K, L), torch.uint8), counts=new((R, K, 12), torch.int32), status=new((R, K), torch.int32))
    lift_out = dict(length=new(R, torch.int32), col_of=new((R, Lmax), torch.int32), pos_of=new((R, L), torch.int32),
                    partner=new((R, K, L), torch.int32), status=new((R, K), torch.int32))
    short = res.partner.contiguous().view(-1)
    start = (torch.arange(R, dtype=torch.int64) * K * Lmax).to(dev)
    stride, nstruct = torch.full((R,), Lmax, dtype=torch.int32, device=dev), torch.full((R,), K, dtype=torch.int32, device=dev)
    entries = {
        "sq_project_rows": lambda: lib.sq_project_rows(p(d_rows), R, L, p(d_lines), 0, K, Lmax, 0, 0, *(p(out[k]) for k in out), stream),
        "sq_lift_rows": lambda: lib.sq_lift_rows(p(d_rows), R, L, p(short), short.numel(), p(start), p(stride), p(nstruct), K, Lmax,
                                                 *(p(lift_out[k]) for k in lift_out), stream)}
    written = lambda tensors: sum(t.numel() * t.element_size() for t in tensors.values())
    moved = {"sq_project_rows": R * L + K * L * 4 + written(out), "sq_lift_rows": R * L + short.numel() * 4 + written(lift_out)}
    times = {name: [] for name in entries}
    for k in range(warmup + timed):
        for name, entry in entries.items():
            t, rc = between_events(entry)
            _lib.check(rc)
            if k >= warmup:
                times[name].append(t)
    for key in out:
        assert torch.equal(out[key], getattr(res, key)), key
    for key in lift_out:
        assert torch.equal(lift_out[key], getattr(lifted, key)), key
    for name in entries:
        rate = moved[name] / (min(times[name]) * 1e-6)
        print("    %s between HIP events: %s; %.1f MB read and written (the shared lines counted once), %.2f TB/s at the best time: %.0f %% of "
              "the measured HBM rate (6.29 TB/s), %.0f %% of the data sheet's (8 TB/s)" % (
                  name, show(times[name]), moved[name] / 1e6, rate / 1e12, 100 * rate / HBM_MEASURED, 100 * rate / HBM_SPEC), flush=True)
    print("    peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "torch":
    res = Project(sequences=seqs, structures=d_lines)
    lifted = Lift(sequences=seqs, structures=res.partner)
    Lmax = int(res.partner.shape[2])
    lut = torch.full((256,), 5, dtype=torch.uint8)
    for k, ch in enumerate("ACGU"):
        lut[ord(ch)] = lut[ord(ch.lower())] = k
    lut[ord("T")] = lut[ord("t")] = 3
    for g in "-.~":
        lut[ord(g)] = 4
    lut, pair_class = lut.to(dev), torch.from_numpy(P._PAIR_CLASS.copy()).to(dev)
    cols = torch.arange(L, device=dev)

    def maps():
        cls = lut[d_rows.long()]
        res_mask = cls != 4
        rank = torch.cumsum(res_mask, 1) - 1
        length = res_mask.sum(1)
        pos_of = torch.where(res_mask, rank, torch.full_like(rank, -1))
        col_of = torch.full((R, Lmax + 1), -1, dtype=torch.int64, device=dev)     # (the gap columns scatter to the spare column)
        col_of.scatter_(1, torch.where(res_mask, rank, torch.full_like(rank, Lmax)), cols[None, :].expand(R, L))
        return cls, res_mask, rank, length, pos_of, col_of[:, :Lmax]

    def project_ops():
        cls, res_mask, rank, length, pos_of, col_of = maps()
        partner = torch.full((R, K, Lmax + 1), -1, dtype=torch.int64, device=dev)
        out_cls = torch.zeros((R, K, L), dtype=torch.uint8, device=dev)
        counts = torch.zeros((R, K, 12), dtype=torch.int64, device=dev)
        for k in range(K):
            pk = d_lines[k].long()
            paired, w = pk >= 0, pk.clamp(min=0)
            v_lo, w_hi = torch.minimum(cols, w), torch.maximum(cols, w)
            pc = pair_class[cls[:, v_lo].long(), cls[:, w_hi].long()]           # [R, L]: the class of the pair a paired column lies in
            keep = paired[None, :] & (pc <= 7)                                   # (the defaults: every pair of two residues, any loop)
            opens = (pk > cols)[None, :]
            out_cls[:, k] = torch.where(opens, pc, torch.zeros_like(pc))
            to = torch.where(keep, rank[:, w], torch.full_like(rank, -1))
            partner[:, k].scatter_(1, torch.where(res_mask, rank, torch.full_like(rank, Lmax)), to)
            counts[:, k, 0] = opens.sum(1).expand(R)
            for c in range(1, 10):
                counts[:, k, c] = (opens & (pc == c)).sum(1)
            counts[:, k, 11] = (opens & keep).sum(1)
        return dict(length=length, col_of=col_of, pos_of=pos_of, partner=partner[:, :, :Lmax], cls=out_cls, counts=counts)

    def lift_ops():
        cls, res_mask, rank, length, pos_of, col_of = maps()
        short = res.partner.long()                                              # [R, K, Lmax]
        at = rank.clamp(min=0)[:, None, :].expand(R, K, L)
        q = torch.gather(short, 2, at)
        to = torch.gather(col_of[:, None, :].expand(R, K, Lmax), 2, q.clamp(min=0))
        return dict(length=length, col_of=col_of, pos_of=pos_of, partner=torch.where(res_mask[:, None, :] & (q >= 0), to, torch.full_like(to, -1)))

    for name, ops, ref in (("Project", project_ops, res), ("Lift", lift_ops, lifted)):
        times = []
        for k in range(warmup + timed):
            t, got = between_events(ops)
            if k >= warmup:
                times.append(t)
        for key, value in got.items():
            assert torch.equal(value.to(getattr(ref, key).dtype), getattr(ref, key)), (name, key)
        print("(b) %s's tensors with torch ops on the device, between HIP events: %s; %s equal; peak device memory %.2f GB" % (
            name, show(times), ", ".join(got), torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)

if step == "unalign":
    res = Project(sequences=seqs, structures=d_lines)
    t0 = sync_time()
    host_lines = d_lines.cpu().numpy()
    t1 = time.perf_counter()
    texts = [dbn.PairsToDBN([(v, int(w)) for v, w in enumerate(row) if w > v], L) for row in host_lines]
    t2 = time.perf_counter()
    found = [[dbn.UnAlign(seq, text, want_pairs=True)[2] for text in texts] for seq in seqs]
    t3 = time.perf_counter()
    found = [[pairs if pairs is not None else dbn.DBNToPairs(text) for pairs, text in zip(mine, texts)] for mine in found]   # (a row without gaps)
    partner, length = res.partner.cpu().numpy(), res.length.cpu().numpy()
    for r in range(0, R, 97):
        for k in range(K):
            mine = partner[r, k, :length[r]]
            assert sorted(found[r][k]) == [(i, int(j)) for i, j in enumerate(mine) if j > i], (r, k)
    print("(c) the lines downloaded %.6f s, as dot-bracket text %.3f s, dbn.UnAlign of %d rows x %d lines %.3f s (%.1f us a call), once; the "
          "pairs of every 97th row equal Project's" % (t1 - t0, t2 - t1, R, K, t3 - t2, (t3 - t2) / (R * K) * 1e6), flush=True)
