#!/usr/bin/env python3
"""Generate tests/golden/interchain.json by IMPORTING the reference (febos/SQUARNA v3.2.2).

Runs only in the build container, where /root/reference exists.  Like gen_lowcomplex_golden.py it writes data only: what the
reference returned, with interchainonly on, for records of tests/bits_checks.py and tests/interchain_checks.py --

  "stems"   for the four records bits_checks.GOLDEN_RECORDS (33, 129, 257 and 300 nt: separators at the edges and on a word
            boundary, one with a restraint line) under bits_checks.WEIGHTS[0]: AnnotateStems(BPMatrix(..., interchainonly=True),
            minlen=1, minscore=-1e9) of the empty structure as [i, j, len, score] lists -- the chain test of the pairing
            predicate beyond the 21 nt of bpmatrix.json, as stems, never as dense matrices
  "folds"   for the four cases interchain_checks.GOLDEN_FOLDS: SQRNdbnseq(..., interchainonly=True) in the record form of
            tests.lowcomplex.check (consensus, number of structures, the first TOP of them, the digest of the whole list)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_interchain_golden.py
"""
import json
import os
import sys
import time
from multiprocessing import Pool

sys.dont_write_bytecode = True
REF = "/root/reference/src/SQUARNA"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, REF)
import SQRNdbnseq as R          # noqa: E402  (the reference)
import SQUARNA as RC            # noqa: E402
from tests import bits_checks as B, interchain_checks as I   # noqa: E402


def stems_of(name):
    seq, reacts, restraints = B.short_form(B.RECORDS[B.NAMES.index(name)])
    rbps, rxs, rl, rr = R.ParseRestraints(restraints)
    b, s = R.BPMatrix(seq, B.WEIGHTS[0], rxs, rl, rr, True, reacts)
    stems = R.AnnotateStems(b, s, rbps, [], 1, -1e9)
    return [[int(st[0][0][0]), int(st[0][0][1]), int(st[1]), float(st[2])] for st in stems]


def fold_one(key):
    case = I.find(*key)
    names, psets = RC.ParseConfig(os.path.join(REF, case["config"] + ".conf"))
    t0 = time.time()
    out = R.SQRNdbnseq(case["seq"], None, None, None, psets, mp=False, interchainonly=True, **case["kw"])
    return I.record_form(case, out), time.time() - t0


if __name__ == "__main__":
    stems = {name: stems_of(name) for name in B.GOLDEN_RECORDS}
    for name, st in stems.items():
        print("%-16s %5d stems" % (name, len(st)), flush=True)
    with Pool(4) as pool:
        res = pool.map(fold_one, I.GOLDEN_FOLDS, chunksize=1)
    for rec, dt in res:
        print("%-14s %-11s %5d structures %6.1fs" % (rec["tag"], rec["config"], rec["nstruct"], dt), flush=True)
    path = os.path.join(HERE, "interchain.json")
    with open(path, "w") as f:
        json.dump(dict(stems=stems, folds=[rec for rec, _ in res]), f, separators=(",", ":"))
    print("interchain.json", os.path.getsize(path), "bytes", flush=True)
