#!/usr/bin/env python3
"""Generate the synthetic alignment goldens by IMPORTING the reference (febos/SQUARNA v3.2.2), as gen_golden.py does.

Runs only where /root/reference exists.  Nothing of the reference is written into the repository: the outputs are data --
three seeded synthetic alignments and the text the reference's Predict(alignment=True) printed for them:

  tests/golden/align_synth/<tag>.afa     the alignments (planted helices, substitutions, gap columns)
  tests/golden/align_synth/cases.json    per tag: the keyword arguments, the line count and sha256 of the text
  tests/golden/text/ali_synth_<tag>.txt  the reference's output

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_align_golden.py
"""
import hashlib
import io
import json
import os
import random
import sys

sys.dont_write_bytecode = True
REF = "/root/reference/src/SQUARNA"
sys.path.insert(0, REF)
import SQUARNA as RC            # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "align_synth")

COMPLEMENT = {"A": "U", "U": "A", "G": "C", "C": "G"}

#: tag: (rows, columns, seed, Predict's keywords)
CASES = {
    "u": (10, 200, 4101, dict(step3="u")),
    "i_ll1": (14, 420, 4102, dict(step3="i", levellimit=1)),
    "2_fl50": (8, 600, 4103, dict(step3="2", freqlimit=0.5)),
}


def alignment(rng, nrow, ncol):
    """Rows descended from one ancestor with planted helices (a pseudoknotted one among them): substitutions -- in a helix
    often compensated on the other strand, or turned into a G-U pair --, per-row deletions, gap blocks shared by several
    rows and one column that is a gap in every row."""
    anc = [rng.choice("ACGU") for _ in range(ncol)]
    helices, used = [], set()
    for _ in range(max(3, ncol // 30)):
        ln = rng.randint(5, 9)
        a = rng.randint(2, ncol - 2 * ln - 12)
        b = rng.randint(a + 2 * ln + 4, min(ncol - 2, a + 2 * ln + 4 + ncol // 3))
        cols = set(range(a, a + ln)) | set(range(b - ln + 1, b + 1))
        if cols & used:
            continue
        used |= cols
        helices.append((a, b, ln))
        for t in range(ln):
            anc[a + t] = rng.choice("GGCCAU")
            anc[b - t] = COMPLEMENT[anc[a + t]]
    allgap = rng.choice([c for c in range(ncol) if c not in used])
    blocks = [(rng.randint(0, ncol - 12), rng.randint(3, 10), set(rng.sample(range(nrow), rng.randint(1, nrow // 2))))
              for _ in range(ncol // 60 + 1)]
    rows = []
    for k in range(nrow):
        row = list(anc)
        for a, b, ln in helices:
            for t in range(ln):
                x = rng.random()
                if x < 0.10:                                           # compensated substitution
                    row[a + t] = rng.choice("ACGU")
                    row[b - t] = COMPLEMENT[row[a + t]]
                elif x < 0.16 and row[a + t] in "GA":                  # wobble
                    row[b - t] = "U" if row[a + t] == "G" else row[b - t]
                elif x < 0.22:                                         # a mismatch
                    row[b - t] = rng.choice("ACGU")
        for c in range(ncol):
            if c not in used and rng.random() < 0.15:
                row[c] = rng.choice("ACGU")
            if rng.random() < 0.03:
                row[c] = "-"
        for start, ln, members in blocks:
            if k in members:
                row[start:start + ln] = "-" * ln
        row[allgap] = "-"
        rows.append(">synth_%s_%d\n%s" % (ncol, k, "".join(row)))
    return "\n".join(rows) + "\n"


def main():
    os.makedirs(OUT, exist_ok=True)
    os.makedirs(os.path.join(HERE, "text"), exist_ok=True)
    cases = {}
    for tag, (nrow, ncol, seed, kw) in CASES.items():
        path = os.path.join(OUT, tag + ".afa")
        with open(path, "w") as f:
            f.write(alignment(random.Random(seed), nrow, ncol))
        buf = io.StringIO()
        RC.Predict(inputfile=path, alignment=True, write_to=buf, byseq=True, threads=8, **kw)
        txt = buf.getvalue()
        step = {ln.split("\t")[1].split("(")[0]: ln.split("\t")[0] for ln in txt.strip().split("\n")[-3:]}
        assert "(" in step["Step-1"] and "(" in step["Step-2"] and step["Step-1"] != step["Step-2"], (tag, step)
        with open(os.path.join(HERE, "text", "ali_synth_" + tag + ".txt"), "w") as f:
            f.write(txt)
        cases[tag] = dict(args=dict(kw, alignment=True), inputfile="align_synth/" + tag + ".afa", rows=nrow, columns=ncol,
                          lines=txt.count("\n"), sha256=hashlib.sha256(txt.encode()).hexdigest())
        print(tag, cases[tag]["lines"], cases[tag]["sha256"][:16], step, flush=True)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
