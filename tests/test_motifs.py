"""CPU tests of the G4 / RBP restraint searches (squarna_amd.motifs, the g4 / rbp options of Predict and Main) against
what the reference returned and printed (tests/golden/motifs.json, tests/golden/text/motif_*.txt; written by
tests/golden/gen_motif_golden.py).  The folds come from the CPU oracle through the test-only OracleEngine."""
import hashlib
import io
import json
import os

import pytest

from squarna_amd import engine as E
from tests.oracle_engine import OracleEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(GOLDEN))

with open(os.path.join(GOLDEN, "motifs.json")) as f:
    MOTIFS = json.load(f)
TEXTS = MOTIFS["texts"]
BPP_TEXTS = [t for t, d in TEXTS.items() if "configfile" not in d["args"] and "config" not in d["args"]
             and not d["args"].get("alignment")]


def prepared(seq, t_to_u=False):
    """The searched sequence: gaps dropped, separators as N, upper case (T as U for the RBP search)."""
    short = ''.join('N' if x in ';&' else x for x in seq if x not in '.-~').upper()
    return short.replace('T', 'U') if t_to_u else short


def run_predict(args):
    from squarna_amd import Predict
    kw = dict(args)
    if "inputfile" in kw:
        kw["inputfile"] = os.path.join(ROOT, kw["inputfile"])
    buf = io.StringIO()
    with E.use_engine(OracleEngine()):
        Predict(write_to=buf, **kw)
    return buf.getvalue()


def test_finders_match_reference():
    from squarna_amd.motifs import FindG4, FindRBP, SearchG4RBP
    cases = MOTIFS["finders"]
    assert len(cases) >= 900
    for seq, g4, rbp, only_g4, only_rbp, both in cases:
        assert list(FindG4(prepared(seq), '+')) == g4, seq
        assert list(FindRBP(prepared(seq, True))) == rbp, seq
        assert list(SearchG4RBP(seq, True, False)) == only_g4, seq
        assert list(SearchG4RBP(seq, False, True)) == only_rbp, seq
        assert list(SearchG4RBP(seq, True, True)) == both, seq
        assert list(SearchG4RBP(seq, False, False)) == [None, False]


def test_fixture_covers_the_choices():
    """The fixture exercises what the issue names: hits of both searches, both at once, a Fab pair, PUM's classes,
    scores at the limit, lowercase / T / gaps / separators."""
    from squarna_amd.motifs import G4Hscore
    cases = MOTIFS["finders"]
    assert sum(c[1][1] for c in cases) > 300 and sum(bool(c[2][1]) for c in cases) > 200
    assert sum(bool(c[5][1]) and c[5][1].endswith(",G4(+)") and c[5][1] != "G4(+)" for c in cases) > 50
    assert any("(" in c[2][0] for c in cases)
    assert {c[0][k + 4] for c in cases for k in range(len(c[0]) - 8) if c[0][k:k + 4] == "UGUA"} >= set("ACU")
    assert any(G4Hscore(c[0]) == 1.2 for c in cases)
    assert all(any(ch in c[0] for c in cases) for ch in "acgtT.-~;&")


def test_g4_score():
    from squarna_amd.motifs import G4Hscore
    assert G4Hscore("GGGAAGGGAAGGGAAGGG") == 36 / 18
    assert G4Hscore("GGGGGG") == 4.0
    assert G4Hscore("CCGGAC") == (-4 + 4 - 1) / 6
    assert G4Hscore("GGCGGCGGCGGCC") == (16 - 3 - 4) / 13


def test_g4_prefers_greedy_runs_and_lazy_loops():
    """Runs of G's split the way re's backtracking splits them: the earlier runs as long as the rest still matches,
    the G's a loop takes stay unmarked; overlapping matches from later starts add their own runs."""
    from squarna_amd.motifs import FindG4
    assert FindG4("GGGAAGGGAAGGGAAGGG") == ("+++..+++..+++..+++", True)
    assert FindG4("GGGGGGGGGG") == ("..........", False)            # four runs of 2 and three loops need 11
    assert FindG4("GGGGGGGGGGG") == ("++.++.++.++", True)
    assert FindG4("GGGGGGGGGGGGG") == ("++++.++.++.++", True)
    assert FindG4("GGGGGGGGGGGGGGG") == ("+" * 15, True)
    assert FindG4("AGGGGGGGGGGGA") == (".++.++.++.++.", True)
    assert FindG4("UUGGUGGGGGGUGGUGGUU") == ("..++.++++++.++.++..", True)
    assert FindG4("GGAGGAGGAGCC") == ("............", False)       # score below 1.2
    assert FindG4("ACGUACGU") == ("........", False)


@pytest.mark.parametrize("tag", sorted(t for t in TEXTS if t not in BPP_TEXTS))
def test_predict_text_matches_reference(tag, capsys):
    txt = run_predict(TEXTS[tag]["args"])
    with open(os.path.join(GOLDEN, "text", tag + ".txt")) as f:
        exp = f.read()
    assert txt == exp
    assert hashlib.sha256(txt.encode()).hexdigest() == TEXTS[tag]["sha256"]
    assert capsys.readouterr().err == TEXTS[tag]["stderr"]


@pytest.mark.parametrize("tag", BPP_TEXTS)
def test_predict_text_default_config_with_bpp(tag, fake_rna):
    """Default configuration: the label resets the default priority paramsets (bppN, bppH1, bppH2) for the fold too."""
    txt = run_predict(TEXTS[tag]["args"])
    with open(os.path.join(GOLDEN, "text", tag + ".txt")) as f:
        assert txt == f.read()


def test_two_records_warn_and_fold_as_without_flags(capsys):
    args = TEXTS["motif_two_records_g4_nobpp"]["args"]
    assert args.get("g4")
    with_flag = run_predict(args)
    assert capsys.readouterr().err == "WARNING: Found more than one sequence, rfam/G4/RBP search disabled.\n"
    without = run_predict({k: v for k, v in args.items() if k != "g4"})
    assert capsys.readouterr().err == ""
    assert with_flag == without


def test_alignment_mode_ignores_flags(capsys):
    args = TEXTS["motif_ali_g4"]["args"]
    assert run_predict(args) == run_predict({k: v for k, v in args.items() if k != "g4"})
    assert capsys.readouterr().err == ""


def test_main_g4_flag(capsys, monkeypatch):
    from squarna_amd import api
    with open(os.path.join(GOLDEN, "text", "motif_readme_g4_nobpp.txt")) as f:
        exp = "None\n" + f.read()
    for argv in (["s=GGGAAGGGAAGGGAAGGG", "c=nobpp", "G4"], ["-s", "GGGAAGGGAAGGGAAGGG", "--config", "nobpp", "-g4"]):
        monkeypatch.setattr("sys.argv", ["SQUARNA"] + argv)
        with E.use_engine(OracleEngine()):
            api.Main()
        assert capsys.readouterr().out == exp
    with open(os.path.join(GOLDEN, "text", "motif_rfam_ex3_rbp_nobpp.txt")) as f:
        exp = "None\n" + f.read()
    monkeypatch.setattr("sys.argv", ["SQUARNA", "s=AUUGCACAAGGAGAAAUGCAUGAAUGUACAUAAAACUAACAAGAAACAC", "c=nobpp", "RBP"])
    with E.use_engine(OracleEngine()):
        api.Main()
    assert capsys.readouterr().out == exp


def test_rfam_still_out_of_scope():
    from squarna_amd import Predict
    for kw in (dict(rfam=True), dict(rfam=True, g4=True), dict(rfam=True, rbp=True)):
        with pytest.raises(NotImplementedError, match="Rfam"):
            Predict(inputseq="GGGAAGGGAAGGGAAGGG", configfile="nobpp", **kw)


def test_sharded_lengths_pass_does_not_search(capsys):
    """PredictSharded's first pass (_lengths_only) neither searches nor warns: the warning comes once, from the fold."""
    from squarna_amd import Predict
    args = dict(TEXTS["motif_two_records_g4_nobpp"]["args"])
    args["inputfile"] = os.path.join(ROOT, args["inputfile"])
    assert Predict(write_to=io.StringIO(), _lengths_only=True, **args) == [18, 26]
    assert capsys.readouterr().err == ""
