#!/usr/bin/env python3
"""What Fold() costs beside Predict(): the 219 SRtest150 records under nobpp, on one GPU, alternating
    Predict(write_to=StringIO)        the text path, end to end
    Fold(), synchronised at the end   the tensor path, end to end
After warm-up the median of RUNS (default 15, at least 10) runs each, and where Fold's time goes (cProfile of one more call).
usage: fold_api_probe.py [RUNS] [OUTFILE]   (the report goes to stdout and, if given, to OUTFILE)"""
import io, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
runs = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 15
import torch
from squarna_amd import Predict, Fold
kw = dict(inputfile=os.path.join(ROOT, "squarna_amd", "data", "datasets", "SRtest150.fas"), inputformat="qf", configfile="nobpp")


def predict():
    t0 = time.perf_counter()
    Predict(write_to=io.StringIO(), **kw)
    return (time.perf_counter() - t0) * 1e3


def fold():
    t0 = time.perf_counter()
    res = Fold(**kw)
    torch.cuda.synchronize()
    assert res.source == "device" and len(res) == 219
    return (time.perf_counter() - t0) * 1e3


for _ in range(5):
    predict(); fold()
tp, tf = [], []
for _ in range(runs):
    tp.append(predict()); tf.append(fold())
med = lambda v: sorted(v)[len(v) // 2]
lines = ["fold_api_probe: SRtest150 (219 records), nobpp, %d alternating runs each after 5 warm-up pairs, %s" % (runs, torch.cuda.get_device_name(0)),
         "Predict(write_to=StringIO)  median %.3f ms  best %.3f ms" % (med(tp), min(tp)),
         "Fold() + synchronize        median %.3f ms  best %.3f ms" % (med(tf), min(tf)),
         "Fold / Predict              %.3f" % (med(tf) / med(tp))]
import cProfile, pstats
pr = cProfile.Profile()
pr.enable(); fold(); pr.disable()
st = pstats.Stats(pr).stats                      # (file, line, function) -> (calls, primitive calls, own time, cumulative time, callers)
top = sorted(st.items(), key=lambda kv: -kv[1][3])[:20]
lines += ["", "one more Fold() call under cProfile, by cumulative time (ms):", "  cumulative      own   calls  function"]
lines += ["  %10.3f %8.3f %7d  %s:%d(%s)" % (v[3] * 1e3, v[2] * 1e3, v[0], os.path.basename(k[0]), k[1], k[2]) for k, v in top]
report = "\n".join(lines) + "\n"
sys.stdout.write(report)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(report)
