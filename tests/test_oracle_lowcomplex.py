"""The CPU oracle (oracle/) against the reference's folds of low-complexity records (tests/golden/lowcomplex.json): greedy
pools full of ties in finalscore, where a restatement of the reference's tie-breaking would drift unnoticed.  The cases the
fixture marks heavy (seconds of the C oracle each) are left to tests/test_hip_lowcomplex.py."""
import io
import os

import pytest

from oracle import sqrn_oracle as O
from tests.lowcomplex import GOLDEN, check, fold_kwargs, load

FIX = load()


def test_fixture_covers_the_switch_points():
    """The fixture keeps what it is for: every configuration, and records on both sides of each of the kernels' switch
    points (96 / 256 / 1,024 nt) and in the 300-620-nt band of the list form."""
    cases = FIX["cases"]
    assert {c["config"] for c in cases} == {"500nobpp", "alt", "nobpp", "greedynobpp", "fastest"}
    lens = [len(c["seq"]) for c in cases]
    for lo, hi in ((90, 96), (97, 130), (240, 256), (257, 300), (400, 620), (1000, 1024), (1025, 1030)):
        assert any(lo <= n <= hi for n in lens), (lo, hi)
    assert any(c["nstruct"] == 1 and set(c["seq"]) == {"A"} for c in cases)          # the stem-free edge
    assert any(c["restraints"] for c in cases) and any(c["reacts"] for c in cases)
    assert sum(1 for c in cases if c["nstruct"] > len(c["top"])) >= 5                # the digest carries more than the top


@pytest.mark.parametrize("config", sorted({c["config"] for c in FIX["cases"]}))
def test_oracle_equals_the_reference_on_low_complexity(config):
    from squarna_amd.config import ParseConfig, builtin_config
    names, psets = ParseConfig(builtin_config(config))
    n = 0
    for c in FIX["cases"]:
        if c["config"] != config or c["heavy"]:
            continue
        out = O.SQRNdbnseq(c["seq"], c["reacts"], c["restraints"], None, psets, **fold_kwargs(c))
        check(out, c, "%s-%s" % (c["tag"], config))
        n += 1
    assert n > 0


@pytest.mark.parametrize("tag", sorted(FIX["texts"]))
def test_predict_text_on_repeats_matches_reference_on_the_oracle(tag):
    """Predict(c=500nobpp) on repeat records through the oracle engine: E, H and N on stem graphs of equal-weight edges."""
    from squarna_amd import Predict
    from squarna_amd import engine as E
    from tests.oracle_engine import OracleEngine
    dig = FIX["texts"][tag]
    buf = io.StringIO()
    with E.use_engine(OracleEngine()):
        Predict(inputfile=os.path.join(GOLDEN, "text", dig["inputfile"]), configfile=dig["configfile"], write_to=buf)
    with open(os.path.join(GOLDEN, "text", tag + ".txt")) as f:
        assert buf.getvalue() == f.read(), tag
