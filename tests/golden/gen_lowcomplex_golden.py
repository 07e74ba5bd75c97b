#!/usr/bin/env python3
"""Generate tests/golden/lowcomplex.json (and a few Predict texts) by IMPORTING the reference (febos/SQUARNA v3.2.2).

Runs only in the build container, where /root/reference exists.  Like gen_golden.py it writes data only: the inputs of
a fixed list of low-complexity records -- dinucleotide and triplet repeats, G/C blocks, two- and three-letter random
sequences from a fixed seed, a stem-free poly-A, repeats under restraints or reactivities -- and what the reference's
SQRNdbnseq returned for them:

  tests/golden/lowcomplex.json          per case: the input, configuration and keyword arguments, the consensus, the
                                        number of structures, the first TOP of them with scores and paramsets, and
                                        tests.lowcomplex.digest over the whole ordered list of (dbn, paramsets)
                                        ("texts": the input of each text below, its line count and sha256)
  tests/golden/text/lowcomplex_*.fas    Predict(inputfile=..., c=500nobpp) on repeat records (E / H / N on stem graphs
  tests/golden/text/lowcomplex_*.txt    of equal-weight edges): the input and the full text

The lengths sit on the kernels' switch points: 90-96 / 97-130 (the survivors' room of the round kernel), 240-256 /
257-300 (SQ_PR_MAXN: the scan form / the list form), 300-620 and 1,000-1,030 (SQ_PR_ROOT_MAXN = 1,024).  `heavy`
marks the cases the oracle test leaves to the GPU test (the 1,000-nt ones).  Cases whose reference fold took minutes
(random GC / GCU records of 400-1,000 nt under pools of 1,000, (AU)^300 under alt) are not in the list.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_lowcomplex_golden.py
"""
import io
import json
import hashlib
import os
import random
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
from tests.lowcomplex import TOP, digest   # noqa: E402

CONFIGS = {"500nobpp": 1000, "alt": 1000, "nobpp": 100, "greedynobpp": 5, "fastest": 1}


def jsonable(x):
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if hasattr(x, "item"):
        x = x.item()
    return x


def rnd(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def reacts_of(line):
    """Reactivities as the reference encodes a '_+#' line (ReactDict, ProcessReacts as in gen_golden.py)."""
    return [float(v) for v in R.ProcessReacts([R.ReactDict[c] for c in line], M=1.8, B=-0.6)]


def cases():
    """(tag, seq, reacts, restraints, config, heavy) -- fixed and in this order."""
    rng = random.Random(2029)
    gc = lambda n: rnd(rng, n, "GC")            # noqa: E731
    gcu = lambda n: rnd(rng, n, "GCU")          # noqa: E731
    out = []

    def add(tag, seq, configs, reacts=None, restraints=None, heavy=()):
        for c in configs:
            out.append((tag, seq, reacts, restraints, c, c in heavy))

    # 90-96 nt: the round kernel's survivors' room for maxn <= 96
    add("GC^48", "GC" * 48, ("500nobpp", "alt", "fastest"))
    add("AU^47", "AU" * 47, ("nobpp", "greedynobpp"))
    add("GU^46", "GU" * 46, ("500nobpp",))
    add("CUG^31", "CUG" * 31, ("alt", "fastest"))
    add("GGGCCC^15", "GGGCCC" * 15, ("nobpp",))
    add("G48C48", "G" * 48 + "C" * 48, ("greedynobpp", "fastest"))
    add("A^96", "A" * 96, ("500nobpp", "fastest"))
    add("gc96", gc(96), ("alt",))
    # 97-130 nt
    add("GC^60", "GC" * 60, ("greedynobpp", "nobpp"))
    add("CUG^40", "CUG" * 40, ("500nobpp",))
    add("G4A4C4^9", "GGGGAAAACCCC" * 9, ("alt", "fastest"))
    add("G50A4C50", "G" * 50 + "AAAA" + "C" * 50, ("500nobpp", "alt"))
    add("gc110", gc(110), ("alt",))
    add("gcu125", gcu(125), ("nobpp",))
    s = "GC" * 55
    add("GC^55+restraints", s, ("nobpp",), restraints="." * 10 + "_" * 6 + "." * 30 + "(" + "." * 40 + ")" + "." * 22)
    # 240-256 nt: the scan form of the round kernel
    add("GC^128", "GC" * 128, ("greedynobpp", "fastest"))
    add("CUG^84", "CUG" * 84, ("nobpp",))
    add("GGGCCC^41", "GGGCCC" * 41, ("500nobpp",))
    add("G120A4C120", "G" * 120 + "AAAA" + "C" * 120, ("fastest", "greedynobpp"))
    add("gcu250", gcu(250), ("greedynobpp",))
    s = "GC" * 125
    r = list("." * 250)
    r[20:32] = "_" * 12
    r[100:104] = "++++"
    r[60], r[181] = "(", ")"
    add("GC^125+restraints", s, ("nobpp",), restraints="".join(r))
    # 257-300 nt: the list form from here on (pools wider than one)
    add("GC^150", "GC" * 150, ("500nobpp",))
    add("AU^140", "AU" * 140, ("alt",))
    add("GU^135", "GU" * 135, ("nobpp",))
    add("G4A4C4^22", "GGGGAAAACCCC" * 22, ("greedynobpp",))
    add("G130C130", "G" * 130 + "C" * 130, ("nobpp",))
    add("CUG^90+reacts", "CUG" * 90, ("500nobpp",), reacts=reacts_of("".join(rng.choice("_+#") for _ in range(270))))
    add("gc290", gc(290), ("greedynobpp",))
    # 300-620 nt
    add("GC^200", "GC" * 200, ("500nobpp", "greedynobpp"))
    add("CUG^150", "CUG" * 150, ("nobpp",))
    add("GGGCCC^90", "GGGCCC" * 90, ("500nobpp",))
    add("G250A4C250", "G" * 250 + "AAAA" + "C" * 250, ("nobpp",))
    s = "GC" * 220
    r = list("." * 440)
    r[0:40] = "_" * 40
    r[300:306] = "_" * 6
    r[120], r[260] = "[", "]"
    add("GC^220+restraints", s, ("greedynobpp",), restraints="".join(r))
    add("A^500", "A" * 500, ("500nobpp",))
    # 1,000-1,030 nt: SQ_PR_ROOT_MAXN (1,024) -- 1,025 leaves the list form
    add("GC^512", "GC" * 512, ("fastest",), heavy=("fastest",))
    add("CUG^342", "CUG" * 342, ("fastest", "greedynobpp"), heavy=("fastest", "greedynobpp"))
    add("GGGCCC^170", "GGGCCC" * 170, ("fastest",), heavy=("fastest",))
    add("A^1030", "A" * 1030, ("500nobpp",), heavy=("500nobpp",))
    return out


def conf(name):
    return RC.ParseConfig(os.path.join(REF, name + ".conf"))


def fold_one(case):
    tag, seq, reacts, restraints, config, heavy = case
    names, psets = conf(config)
    kw = dict(poollim=CONFIGS[config])
    t0 = time.time()
    out = R.SQRNdbnseq(seq, reacts, restraints, None, psets, mp=False, **kw)
    dt = time.time() - t0
    structs = [[d, jsonable(list(sc)), jsonable(list(ps))] for d, sc, ps in out[1]]
    rec = dict(tag=tag, seq=seq, reacts=reacts, restraints=restraints, config=config, kw=kw, heavy=heavy,
               cons=out[0], nstruct=len(structs), top=structs[:TOP], digest=digest(structs))
    return rec, dt


def gen_fold():
    todo = cases()
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(fold_one, todo, chunksize=1)
    for (rec, dt) in res:
        print("%-22s %-11s %5d nt %5d structures %7.1fs%s" % (rec["tag"], rec["config"], len(rec["seq"]), rec["nstruct"], dt,
                                                               "  heavy" if rec["heavy"] else ""), flush=True)
    return [rec for rec, _ in res]


TEXTS = [
    ("lowcomplex_500nobpp_repeats", ">gc48\n" + "GC" * 48 + "\n>cug40\n" + "CUG" * 40 + "\n>gggccc15\n" + "GGGCCC" * 15 + "\n"),
    ("lowcomplex_500nobpp_blocks", ">g30a4c30\n" + "G" * 30 + "AAAA" + "C" * 30 + "\n>g4a4c4x6\n" + "GGGGAAAACCCC" * 6 + "\n>a60\n" + "A" * 60 + "\n"),
    ("lowcomplex_500nobpp_dinuc", ">au50\n" + "AU" * 50 + "\n>gu40\n" + "GU" * 40 + "\n"),
    ("lowcomplex_500nobpp_restrained", ">gc60r\n" + "GC" * 60 + "\n" + ("__++##" * 20) + "\n" + "." * 20 + "(" + "." * 60 + ")" + "_" * 8
     + "." * 30 + "\n"),                            # (sequence, reactivities, restraints: the default input format qtrf)
]


def gen_text():
    digests = {}
    for tag, fas in TEXTS:
        path = os.path.join(HERE, "text", tag + ".fas")
        with open(path, "w") as f:                  # (the input sits beside the text; Predict reads a file)
            f.write(fas)
        buf = io.StringIO()
        RC.Predict(inputfile=path, configfile="500nobpp", write_to=buf, byseq=True, threads=1)
        txt = buf.getvalue()
        with open(os.path.join(HERE, "text", tag + ".txt"), "w") as f:
            f.write(txt)
        digests[tag] = dict(inputfile=tag + ".fas", configfile="500nobpp", lines=txt.count("\n"),
                            sha256=hashlib.sha256(txt.encode()).hexdigest())
        print(tag, digests[tag]["lines"], digests[tag]["sha256"][:16], flush=True)
    return digests


if __name__ == "__main__":
    texts = gen_text()
    recs = gen_fold()
    with open(os.path.join(HERE, "lowcomplex.json"), "w") as f:
        json.dump(dict(cases=recs, texts=texts), f, separators=(",", ":"))
    print("lowcomplex.json", os.path.getsize(os.path.join(HERE, "lowcomplex.json")), "bytes", flush=True)
