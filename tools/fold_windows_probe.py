#!/usr/bin/env python3
"""Where the time of one FoldWindows call goes, on a random sequence of N nt: building the window records, the Fold call,
the count kernel (HIP events around the launch alone, buffers allocated before), the device sort into the rank order, the
first fit with its rounds.  Beside it the way without FoldWindows on the same input: Fold(records=windows), every window's
consensus row copied to the host, a dict count there; the two tables are asserted equal.
usage: fold_windows_probe.py N WINDOW STEP [CONFIG]"""
import bisect, ctypes, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from squarna_amd import Fold, FoldWindows, _lib, engine as E, fold_windows as FW

N, window, step = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
config = sys.argv[4] if len(sys.argv) > 4 else "nobpp"
rng = random.Random(N)
seq = ''.join(rng.choice("ACGU") for _ in range(N))
spent, marks = {}, {}


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def timed(name, fn):
    def call(*a, **kw):
        t0 = sync_time()
        marks.setdefault(name + "_start", t0)
        out = fn(*a, **kw)
        spent[name] = spent.get(name, 0.0) + sync_time() - t0
        return out
    return call


class TimedEngine(E.HipEngine):
    """The two engine calls FoldWindows makes behind the fold, bracketed by a device synchronize."""
    window_pair_count = timed("count", E.HipEngine.window_pair_count)
    first_fit = timed("first_fit", E.HipEngine.first_fit)


def run():
    spent.clear(); marks.clear()
    fold, rank = FW._fold.Fold, FW._rank_order
    FW._fold.Fold, FW._rank_order = timed("fold", fold), timed("sort", rank)
    try:
        with E.use_engine(TimedEngine()):
            t0 = sync_time()
            res = FoldWindows(records=[(">probe", seq, None, None, None)], window=window, step=step, configfile=config)
            total = sync_time() - t0
    finally:
        FW._fold.Fold, FW._rank_order = fold, rank
    spent["records"] = marks["fold_start"] - t0
    return total, res


run()                                                                    # warm-up: library load, allocator, first launches
total, res = run()
T, P = int(res.win_off[-1]), int(res.pair_count.numel())
print("N %d window %d step %d config %s: %d windows, %d distinct pairs, %d pairs in the consensus at %.2f, source %s" % (
    N, window, step, config, T, P, len(res.pairs(0)), res.freqlimit, res.source), flush=True)
rest = total - sum(spent[k] for k in ("records", "fold", "count", "sort", "first_fit"))
print("FoldWindows %.4f s: window records %.4f, Fold %.4f, count call %.4f, sort %.4f, first fit %.4f (%s rounds), rest %.4f" % (
    total, spent["records"], spent["fold"], spent["count"], spent["sort"], spent["first_fit"], list(res.first_fit_rounds), rest), flush=True)

# the count kernel alone: the launch between two events, its buffers allocated before
w = res.windows
starts = res.starts.contiguous()
lens = w.lengths.to(torch.int32)
flat = torch.empty(P + 1, dtype=torch.int64, device=res.device)
small = [torch.empty(P + 1, dtype=torch.int32, device=res.device) for _ in range(3)]
out = torch.empty(2, dtype=torch.int64, device=res.device)
p = lambda x: ctypes.c_void_p(x.data_ptr())
stream = torch.cuda.current_stream()
times = []
for _ in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(_lib.load().sq_window_pair_count(p(w.partner), p(w.cell_off), 0, T, p(starts), p(lens), N, p(flat), p(small[0]), p(small[1]),
                                                 p(small[2]), P + 1, p(out), ctypes.c_void_p(stream.cuda_stream)))
    e1.record()
    torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
assert out.tolist() == [P, 0]
print("sq_window_pair_count between HIP events (memset of the result words + kernel), 7 launches: median %.1f us (%s)" % (
    statistics.median(times), " ".join("%.1f" % t for t in times)), flush=True)

# the way without FoldWindows: the same window records through Fold, the rows to the host, a dict there
t0 = sync_time()
recs = [(n, s, None, None, None) for n, s in zip(w.names, w.sequences)]
t1 = sync_time()
plain = Fold(records=recs, configfile=config)
t2 = sync_time()
partner, cell_off = plain.partner.cpu().tolist(), plain.cell_off.cpu().tolist()
t3 = sync_time()
sl = res.starts.tolist()
table = {}
for k, a in enumerate(sl):
    row = partner[cell_off[k]:cell_off[k] + min(window, N)]
    for t, q in enumerate(row):
        if q > t:
            c, f = table.get((a + t, a + q), (0, k))
            table[(a + t, a + q)] = (c + 1, f)
wlen = min(window, N)
full = [(i, j, c, bisect.bisect_right(sl, i) - bisect.bisect_right(sl, j - wlen), f) for (i, j), (c, f) in table.items()]
full.sort(key=lambda e: (-(e[2] / e[3]), -e[2], e[4], e[0], e[1]))
cons = [-1] * N
for i, j, c, cov, f in full:
    if c / cov >= res.freqlimit and cons[i] < 0 and cons[j] < 0:
        cons[i], cons[j] = j, i
t4 = sync_time()
assert res.pair_pos.tolist() == [[e[0], e[1]] for e in full] and res.pair_count.tolist() == [e[2] for e in full]
assert res.pair_cover.tolist() == [e[3] for e in full] and res.pair_first.tolist() == [e[4] for e in full]
assert res.consensus.tolist() == cons
print("without FoldWindows %.4f s: Fold(records=windows) %.4f, rows to host lists %.4f, dict count + sort + first fit in Python %.4f "
      "(window records given: %.4f to wrap them); tables and consensus equal" % (t4 - t1, t2 - t1, t3 - t2, t4 - t3, t1 - t0), flush=True)
print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
