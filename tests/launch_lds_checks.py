"""Records and folds of tests/test_hip_launch_lds.py: short records of mixed lengths, each without reactivities, with encoded
reactivities (few levels: the scoring kernels' cell table holds the factors) and with float reactivities (factors per cell, the
reactivities staged in LDS by the job's own length), folded as width-1 pools on a chosen route.

As a program (python -m tests.launch_lds_checks staging): staging_batches() on the launched rounds in a process whose environment
moved the scoring kernel's staging limits down (sq_tuning reads them once per process), as JSON on stdout."""
import json
import os
import sys

import numpy as np

LENGTHS = (5, 33, 64, 65, 200, 201, 300)
ROUTES = {"default": {}, "launched": {"SQ_NO_ROUNDS": "1"}, "hosted": {"SQ_NO_CHAIN": "1"}}


def records(lengths=LENGTHS, seed=24):
    """[(seq, reacts or None)]: every length three times -- plain, encoded reactivities, float reactivities"""
    from squarna_amd.dbn import ProcessReacts, ReactDict
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        seq = "".join(rng.choice(list("ACGU"), n))
        line = rng.choice(list("_+#"), n, p=[0.5, 0.3, 0.2])
        out += [(seq, None), (seq, ProcessReacts([ReactDict[c] for c in line], M=1.8, B=-0.6)), (seq, [float(x) for x in rng.random(n)])]
    return out


def staging_batches():
    """the batches of the staging child: the records in both orders (launches sized for 300 nt), and the records up to 64 nt and
    up to 65 nt as batches of their own -- the staging of reactivities is decided by a launch's longest sequence"""
    recs = records()
    return [("forward", recs), ("reversed", recs[::-1]), ("upto64", [r for r in recs if len(r[0]) <= 64]),
            ("upto65", [r for r in recs if len(r[0]) <= 65])]


def psets():
    from squarna_amd.config import ParseConfig, builtin_config
    return ParseConfig(builtin_config("fastest"))[1]


def fold(recs, route):
    """(packed records, results, driver, paths) of one batch of `recs` folded with poollim = 1 on `route`"""
    from squarna_amd.engine import Batch, Prepared
    env = ROUTES[route]
    assert not any(k in os.environ for k in env), env
    ps = psets()
    os.environ.update(env)
    try:
        with Batch([Prepared(s, r) for s, r in recs], [ps] * len(recs), max_structs=64 * len(recs), fp32=False) as b:
            b.fold(poollim=1)
            buf, off = b.pack_all()
            return ([buf[off[k]:off[k + 1]].tobytes() for k in range(len(recs))], [r[0] for r in b.results_all()], b.fold_driver,
                    b.fold_paths)
    finally:
        for k in env:
            os.environ.pop(k, None)


def plain(result):
    """a fold result as JSON-able lists: [consensus, [[dbn, scores, paramsets], ..]]"""
    return [result[0], [[d, [float(x) for x in sc], [int(x) for x in p]] for d, sc, p in result[1]]]


if __name__ == "__main__":
    assert sys.argv[1:] == ["staging"] and os.environ.get("SQ_SCORE_NR_LIM") and os.environ.get("SQ_SCORE_STATE_LIM")
    out = {}
    for name, rs in staging_batches():
        packed, results, driver, paths = fold(rs, "launched")
        out[name] = dict(results=[plain(r) for r in results], driver=driver, paths=paths)
    json.dump(out, sys.stdout)
