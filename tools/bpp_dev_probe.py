#!/usr/bin/env python3
"""What handing base-pair probabilities over as device tensors saves: RECORDS (default 64) records of 1,000 nt under the `1000`
configuration with synthetic matrices of tests/fake_rna.py's form, on one GPU, alternating
    host terms     a provider returns numpy matrices; bpp_terms forms (bppm / max) ** |bpp| per job, the batch uploads them
    device path    the same matrices as CUDA tensors; sq_bpp_dev.hip forms every job's term in the workspace
After one warm-up pair the median of five runs each of Batch() and of the fold behind it (and of five more runs of the device
path back to back), the two kernels' time from the
HIP events around them (sq_profile_get slot 9) and their bytes / time beside sq_fill_kernel's 5.4 TB/s.
usage: bpp_dev_probe.py [RECORDS] [OUTFILE]   (the report goes to stdout and, if given, to OUTFILE)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from squarna_amd import engine as E
from squarna_amd.config import ParseConfig, builtin_config

R = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N, RUNS = 1000, 5
names, psets = ParseConfig(builtin_config("1000"))
nbpp = sum(1 for ps in psets if ps.get("bpp", 0))
rng = np.random.default_rng(1000)
seqs = ["".join(rng.choice(list("ACGU"), N)) for _ in range(R)]
PAIR = np.zeros((256, 256), bool)
for a, b in ("GC", "CG", "AU", "UA", "GU", "UG"):
    PAIR[ord(a), ord(b)] = True


def matrix(seq, k):
    c = np.frombuffer(seq.encode(), np.uint8)
    u, keep = np.random.default_rng(k).random((2, N, N))
    ok = PAIR[c[:, None], c[None, :]] & (np.arange(N)[None, :] >= np.arange(N)[:, None] + 4) & (keep < 0.6)
    return np.where(ok, u ** 3, 0.0)


host = {s: matrix(s, k) for k, s in enumerate(seqs)}
dev = [torch.from_numpy(host[s]).cuda() for s in seqs]
recs = [(s, None, None, None, psets, None) for s in seqs]
eng = E.HipEngine()
E.set_bpp_provider(lambda seq, reacts, M, B: host[seq])


def run(device):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b, opts = eng._make_batch(E._with_bpp(recs, dev) if device else recs, None, {})
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    kern = b.profile_get(9) if device else (0.0, 0, 0.0)
    b.fold(**opts)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    packed = b.pack_all(copy=True)[0].tobytes()
    b.close()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, kern, packed


ph, pd = run(False), run(True)
assert ph[3] == pd[3], "the two paths fold differently"
th, td = [], []
for _ in range(RUNS):
    th.append(run(False)[:2]); td.append(run(True)[:3])
alone = [run(True)[:2] for _ in range(RUNS)]                          # the device path without the other road's host work in between
med = lambda v: sorted(v)[len(v) // 2]
kms, kbytes = med([x[2][0] for x in td]), td[0][2][2]
lines = ["bpp_dev_probe: %d records of %d nt, `1000` configuration (%d paramsets, %d with bpp != 0), median of %d alternating runs after one warm-up pair, %s"
         % (R, N, len(psets), nbpp, RUNS, torch.cuda.get_device_name(0)),
         "packed results of the two paths: identical",
         "host terms     Batch() %9.2f ms   fold %9.2f ms   (%.2f GB of terms uploaded)" % (med([x[0] for x in th]), med([x[1] for x in th]), 8e-9 * N * N * nbpp * R),
         "device path    Batch() %9.2f ms   fold %9.2f ms" % (med([x[0] for x in td]), med([x[1] for x in td])),
         "device path    Batch() %9.2f ms   fold %9.2f ms   (five runs back to back)" % (med([x[0] for x in alone]), med([x[1] for x in alone])),
         "sq_bpp_max_kernel + sq_bpp_term_kernel: %.3f ms for %.3f GB = %.2f TB/s   (sq_fill_kernel: 5.4 TB/s)"
         % (kms, kbytes * 1e-9, kbytes / (kms * 1e-3) * 1e-12 if kms > 0 else float("nan"))]
report = "\n".join(lines) + "\n"
sys.stdout.write(report)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write(report)
