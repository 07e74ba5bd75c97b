#!/usr/bin/env python3
"""Generate the golden vectors of the G4 / RBP restraint searches by IMPORTING the reference (febos/SQUARNA v3.2.2).

Runs only where the reference exists (like gen_golden.py).  Nothing from the reference is written into the repo:
the outputs are *data* -- inputs and what the reference returned or printed for them:

  tests/golden/motifs.json         "finders": [seq, FindG4(prepared seq, '+'), FindRBP(prepared seq with U for T),
                                   SearchRfamG4RBP(seq, ..., rfam=False, g4, rbp) for g4 / rbp / both]
                                   (SQRNrfam.py:118-269);
                                   "texts": args, stderr, line count and sha256 of every text below
  tests/golden/text/motif_*.txt    Predict(..., g4 / rbp) full outputs (SQUARNA.py:850-907)
  tests/golden/motif_inputs/*      input files of those texts (written here as well)

ViennaRNA is absent: tests/fake_rna.py is installed as ``RNA`` first, as in gen_bpp_golden.py (only the default-config
text folds with base-pair probabilities; the others use nobpp configurations).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_motif_golden.py
"""
import contextlib
import hashlib
import io
import json
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src/SQUARNA"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
from tests import fake_rna          # noqa: E402
fake_rna.install()                  # BEFORE the reference runs: its `import RNA` finds the stand-in
import SQRNrfam as R                # noqa: E402  (the reference)
import SQUARNA as RC                # noqa: E402

INPUTS = os.path.join(HERE, "motif_inputs")
MOTIFS = ["AUUGCAC", "GGAGA", "UGCAUG", "UGUA{H}AU{W}", "ACUAAC", "GAAACAC"]


def prepared(seq, t_to_u=False):
    short = ''.join('N' if x in ';&' else x for x in seq if x not in '.-~').upper()
    return short.replace('T', 'U') if t_to_u else short


def motif(rng, k):
    m = MOTIFS[k]
    return m.replace("{H}", rng.choice("ACU")).replace("{W}", rng.choice("AU"))


def rnd(rng, n, alphabet="ACGU"):
    return ''.join(rng.choice(alphabet) for _ in range(n))


def g4_construct(rng, runs=(2, 8), loops=(1, 14), loop_alpha="ACGUN", nruns=None):
    parts = []
    for r in range(nruns or rng.randrange(3, 6)):
        if r:
            parts.append(rnd(rng, rng.randrange(loops[0], loops[1] + 1), loop_alpha))
        parts.append('G' * rng.randrange(runs[0], runs[1] + 1))
    return ''.join(parts)


def decorate(rng, seq):
    """Lowercase, T for U, gap characters and separators at random places."""
    out = []
    for ch in seq:
        r = rng.random()
        if r < 0.08:
            out.append(rng.choice(".-~"))
        elif r < 0.11:
            out.append(rng.choice(";&"))
        ch = 'T' if ch == 'U' and rng.random() < 0.5 else ch
        out.append(ch.lower() if rng.random() < 0.15 else ch)
    return ''.join(out)


def score_near(rng, shape, exact, count, tries=200000):
    """G4-shaped strings (non-G loops: the whole string is the match) whose score is exactly / about 1.2."""
    runs, loops = ((2, 5), (1, 2)) if shape == 0 else ((3, 5), (1, 12))
    out = set()
    for _ in range(tries):
        s = g4_construct(rng, runs, loops, loop_alpha="CCCAUN", nruns=4)
        tot = R.G4Hscore(s) * len(s)
        hit = round(tot) * 5 == 6 * len(s) if exact else abs(R.G4Hscore(s) - 1.2) < 0.06
        if hit:
            out.add(s)
            if len(out) >= count:
                break
    return sorted(out)


def finder_inputs(rng):
    seqs = []
    seqs += ['G' * n for n in range(1, 33)]                                       # all-G: greedy runs against lazy loops
    seqs += [g4_construct(rng) for _ in range(170)]                               # runs 2-8, loops 1-14
    seqs += [g4_construct(rng, runs=(5, 9), loops=(1, 4), loop_alpha="GGA") for _ in range(60)]   # runs of 6+, G loops
    seqs += [rnd(rng, rng.randrange(1, 12)) + g4_construct(rng) + rnd(rng, rng.randrange(0, 8)) for _ in range(80)]
    seqs += [rnd(rng, rng.randrange(10, 40), "GGGGGAC") for _ in range(80)]
    for shape in (0, 1):                                                          # scores at and around 1.2
        seqs += score_near(rng, shape, True, 30)
        seqs += score_near(rng, shape, False, 30)
    for _ in range(160):                                                          # planted RBP motifs
        s = rnd(rng, rng.randrange(0, 25))
        for _ in range(rng.randrange(1, 5)):
            k = rng.randrange(len(MOTIFS))
            s += motif(rng, k) * rng.randrange(1, 3) + rnd(rng, rng.randrange(0, 4))
        seqs.append(s)
    seqs += ["GGAGAGGAGAGA", "UGCAUGCAUG", "AUUGCACAUUGCAC", "GAAACACGAAACAC", "ACUAACUAAC", "UGUAAAUAUGUACAUU",
             "UGUAUAUU", "UGUAGAUA", "UGUACAUC", "UGUAUAUA" + "UGUAAAUU"]
    for _ in range(100):                                                          # both G4 and RBP
        s = g4_construct(rng, runs=(3, 5), loops=(1, 6))
        k = rng.randrange(len(MOTIFS))
        cut = rng.randrange(len(s) + 1)
        seqs.append(s[:cut] + motif(rng, k) + s[cut:])
    base = list(seqs)
    seqs += [decorate(rng, s) for s in rng.sample(base, 120)]                     # lowercase, T, .-~ gaps, ; & separators
    seqs += ["", "...", "G;GG&GGG", "gggaagggaagggaaggg", "GGG_GGG_GGG_GGG", "GGG1GGG2GGG3GGG", "GGG GGG GGG GGG",
             "GGG*GGG*GGG*GGG", "auugcac", "ATTGCAC", "UGTACATT", "GAAACAC-GAAACAC", "GGAG.A"]
    for _ in range(3):                                                            # a few long ones
        s = rnd(rng, 300)
        for _ in range(6):
            p = rng.randrange(len(s))
            s = s[:p] + (g4_construct(rng, runs=(3, 5), loops=(1, 7)) if rng.random() < 0.5
                         else motif(rng, rng.randrange(len(MOTIFS)))) + s[p:]
        seqs.append(s)
    return seqs


def gen_finders(rng):
    out = []
    for seq in finder_inputs(rng):
        search = [list(R.SearchRfamG4RBP(seq, None, None, False, g4, rbp))
                  for g4, rbp in ((True, False), (False, True), (True, True))]
        out.append([seq, list(R.FindG4(prepared(seq), '+')), list(R.FindRBP(prepared(seq, True)))] + search)
    return out


def write_inputs():
    rng = random.Random(22)
    os.makedirs(INPUTS, exist_ok=True)
    g4rbp = "GGGCAAGGGAAAGGGCCCGGGAUUGCACAAGGAGAAAUGCAUG"
    files = {
        # default format "qtrf": sequence, reactivities, restraints (replaced by the search), reference
        "default_qtrf.fas": ">G4 and Fab, with reactivities, restraints and a reference\n"
                            "GGCAGGGAAGGGAAGGGAAGGGCGAAACACUGCC\n"
                            "0.1 0.2 0.9 0.8 0.1 0.1 0.1 0.7 0.6 0.1 0.1 0.1 0.5 0.5 0.1 0.2 0.1 0.6 0.4 0.1 0.1 0.1 "
                            "0.3 0.2 0.9 0.9 0.9 0.4 0.3 0.2 0.1 0.1 0.1 0.2\n"
                            "((((..........................))))\n"
                            "((((.......................)..))))\n",
        "two_records.fas": ">first\nGGGAAGGGAAGGGAAGGG\n>second\nAUUGCACAAGGGAGGGAGGGAGGGAA\n",
        "gapped.fas": ">gapped, with separators\nGGG-AAGGG..AAGGG~AAGGG;GCUUGCAUGAAGC&ACUAACGGUUA\n",
    }
    s = rnd(rng, 420)
    for k, ins in enumerate([g4rbp, "GGGAGGGAGGGAGGG", "GAAACAC", "UGUAAAUA", "GGAGA", "GGGUUGGGCUGGGAAGGG", "ACUAAC"]):
        p = 40 + 55 * k
        s = s[:p] + ins + s[p:]
    files["long_500nobpp.fas"] = ">long, G4 and RBP motifs planted\n" + s + "\n"
    for name, text in files.items():
        with open(os.path.join(INPUTS, name), "w") as f:
            f.write(text)


def inp(name):
    return os.path.join("tests", "golden", "motif_inputs", name)


def ex(name):
    return os.path.join("squarna_amd", "data", "examples", name)


TEXT_JOBS = [
    ("motif_readme_g4_nobpp", dict(inputseq="GGGAAGGGAAGGGAAGGG", configfile="nobpp", g4=True)),
    ("motif_readme_g4_fastest", dict(inputseq="GGGAAGGGAAGGGAAGGG", configfile="fastest", g4=True)),
    # (the default configuration's priority paramsets would rank first without the reset a found label makes)
    ("motif_g4_def", dict(inputseq="CGUAAUGCCUUUCCCUAACAGAGUUUUGGGAGGGAGGGAGGGUCGAACUCGUGUUGUCGAGCGACGGAAU", g4=True)),
    ("motif_rfam_ex1_g4_nobpp", dict(inputseq="GGGCCAUUGGGUGGGAUCUGGGGGGG", configfile="nobpp", g4=True)),
    ("motif_rfam_ex2_g4_greedynobpp", dict(inputseq="GGGCAAGGGAAAGGGCCCGGG", configfile="greedynobpp", g4=True)),
    ("motif_rfam_ex3_rbp_nobpp", dict(inputseq="AUUGCACAAGGAGAAAUGCAUGAAUGUACAUAAAACUAACAAGAAACAC",
                                      configfile="nobpp", rbp=True)),
    ("motif_rfam_ex4_g4rbp_alt", dict(inputseq="GGCUGGUGAUUGGGACCGGGCAGGGCGGGCACGGGCCAGCC", configfile="alt",
                                      g4=True, rbp=True)),
    ("motif_g4rbp_nobpp", dict(inputseq="GGGCAAGGGAAAGGGCCCGGGAUUGCACAAGGAGAAAUGCAUG", configfile="nobpp",
                               g4=True, rbp=True)),
    ("motif_g4rbp_fastest_bs", dict(inputseq="GGGCAAGGGAAAGGGCCCGGGAUUGCACAAGGAGAAAUGCAUG", configfile="fastest",
                                    g4=True, rbp=True, byseq=True)),
    ("motif_default_qtrf_g4rbp_nobpp", dict(inputfile=inp("default_qtrf.fas"), configfile="nobpp", g4=True, rbp=True)),
    ("motif_default_qtrf_g4_greedynobpp_bs", dict(inputfile=inp("default_qtrf.fas"), configfile="greedynobpp",
                                                  g4=True, byseq=True, reactformat=10, toplim=3)),
    ("motif_gapped_g4rbp_nobpp", dict(inputfile=inp("gapped.fas"), configfile="nobpp", g4=True, rbp=True)),
    ("motif_nothing_g4rbp_nobpp", dict(inputseq="ACGUACGUACUCGACG", configfile="nobpp", g4=True, rbp=True)),
    ("motif_long_g4rbp_500nobpp", dict(inputfile=inp("long_500nobpp.fas"), configfile="500nobpp", g4=True, rbp=True)),
    ("motif_two_records_g4_nobpp", dict(inputfile=inp("two_records.fas"), configfile="nobpp", g4=True)),
    ("motif_two_records_nobpp", dict(inputfile=inp("two_records.fas"), configfile="nobpp")),
    ("motif_ali_g4", dict(inputfile=ex("ali_input.afa"), alignment=True, g4=True)),
]


def gen_texts():
    os.makedirs(os.path.join(HERE, "text"), exist_ok=True)
    texts = {}
    for tag, kw in TEXT_JOBS:
        run = dict(kw)
        if "inputfile" in run:
            run["inputfile"] = os.path.join(ROOT, run["inputfile"])
        buf, err = io.StringIO(), io.StringIO()
        with contextlib.redirect_stderr(err):
            RC.Predict(write_to=buf, threads=4, **run)
        txt = buf.getvalue()
        with open(os.path.join(HERE, "text", tag + ".txt"), "w") as f:
            f.write(txt)
        texts[tag] = dict(args=kw, stderr=err.getvalue(), lines=txt.count("\n"),
                          sha256=hashlib.sha256(txt.encode()).hexdigest())
        print(tag, texts[tag]["lines"], texts[tag]["sha256"][:16], flush=True)
    return texts


if __name__ == "__main__":
    write_inputs()
    out = dict(finders=gen_finders(random.Random(21)), texts=gen_texts())
    with open(os.path.join(HERE, "motifs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("motifs.json", len(out["finders"]), "finder cases",
          os.path.getsize(os.path.join(HERE, "motifs.json")), "bytes", flush=True)
