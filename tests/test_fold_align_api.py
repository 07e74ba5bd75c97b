"""CPU tests of FoldAlignment() / AlignmentResult (no GPU): the alignment results API through the test-only OracleEngine -- an
engine without the device methods, for which FoldAlignment builds the same AlignmentResult on the CPU -- against the Step lines
of the reference's own output (tests/golden/text/*.txt), a plain dict count over the rows and align.Consensus.
All comparisons are exact."""
import io
import os

import pytest

from squarna_amd import engine as E
from tests.fold_align_checks import CASES, DATA, check_against_golden, check_consensus_at, check_table
from tests.oracle_engine import OracleEngine

ALI_INPUT = os.path.join(DATA, "examples", "ali_input.afa")


def fold_alignment(**kw):
    from squarna_amd import FoldAlignment
    with E.use_engine(OracleEngine()):
        return FoldAlignment(**kw)


@pytest.fixture(scope="module")
def results():
    return {}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_steps_metrics_and_scores_equal_the_reference_text(tag, results):
    path, kw = CASES[tag]
    res = results[tag] = fold_alignment(inputfile=path, **kw)
    assert res.source == "host" and res.device.type == "cpu"
    assert tuple(res.steps.shape) == (3, res.L) and tuple(res.stem_matrix.shape) == (res.L, res.L)
    assert tuple(res.metrics.shape) == (3, 6) and tuple(res.react_scores.shape) == (3,)
    check_against_golden(res, tag)
    if res.rows is None:
        assert res.pair_cols.numel() == res.pair_count.numel() == res.pair_first.numel() == 0
        assert res.steps[1].tolist() == [-1] * res.L
        with pytest.raises(ValueError, match="step 2 was skipped"):
            res.consensus_at(0.5)


@pytest.mark.parametrize("tag", [t for t in sorted(CASES) if CASES[t][1].get("step3") != "1"])
def test_pair_table_and_consensus_at(tag, results):
    path, kw = CASES[tag]
    res = results.get(tag) or fold_alignment(inputfile=path, **kw)
    check_table(res)
    check_consensus_at(res)


def test_rows_equal_the_engines_tuples():
    """rows: the FoldResult of step 2 -- every row folded with the normalised matrix as weight -- against fold_records."""
    from squarna_amd.config import ParseConfig, builtin_config
    from tests.fold_checks import check_against_tuples
    res = fold_alignment(inputfile=ALI_INPUT)
    _, psets = ParseConfig(builtin_config("ali"))
    import contextlib
    from squarna_amd.inputs import ParseInput
    with contextlib.redirect_stdout(io.StringIO()):
        objs = list(ParseInput(None, ALI_INPUT, "qtrf")[0])            # (the default reference line is every row's)
    assert [obj[1] for obj in objs] == res.sequences and all(obj[4] for obj in objs)
    recs = [(obj[1], obj[2], obj[3], obj[4], psets, res.stem_matrix.numpy()) for obj in objs]
    tuples = OracleEngine().fold_records(recs, rankby=(2, 0, 1), levellimit=None, priority=set())
    check_against_tuples(res.rows, tuples, keep=5)
    assert res.rows.names == res.names and res.rows.source == "host"
    for r, seq in enumerate(res.sequences):                               # gap columns stay unpaired
        row = res.rows.partner[int(res.rows.cell_off[r]):int(res.rows.cell_off[r]) + len(seq)].tolist()
        assert all(row[c] == -1 for c, ch in enumerate(seq) if ch in "-.~")
    import numpy as np
    sm = res.stem_matrix.numpy()
    assert sm.max() == 5.0 and (sm == sm.T).all() and np.isfinite(sm).all()


def test_equals_predict_and_prints_nothing(capsys):
    from squarna_amd import Predict
    for kw in (dict(), dict(s3="2", fl=0.2, ll=2), dict(step3="i", freqlim=0.6)):
        res = fold_alignment(i=ALI_INPUT, **kw)
        out = capsys.readouterr()
        assert out.out == "" and out.err == ""
        buf = io.StringIO()
        with E.use_engine(OracleEngine()):
            Predict(i=ALI_INPUT, a=True, write_to=buf, **kw)
        lines = buf.getvalue().rstrip("\n").split("\n")[-3:]
        assert [res.dbn(k) for k in (1, 2, 3)] == [ln.split("\t")[0] for ln in lines]
        host = res.cpu()
        assert host.steps.tolist() == res.steps.tolist() and host.dbn(3) == res.dbn(3)
    with pytest.raises(IndexError):
        res.dbn(4)


def test_validation_messages_are_predicts():
    from squarna_amd import FoldAlignment, Predict
    with E.use_engine(OracleEngine()):
        for kw, exc, msg in ((dict(inputfile="/nonexistent/file.afa"), AssertionError, "Input file does not exist"),
                             (dict(inputfile=ALI_INPUT, freqlimit=1.5), ValueError, "Inappropriate freqlimit value"),
                             (dict(inputfile=ALI_INPUT, step3="x"), ValueError, "Inappropriate freqlimit value"),
                             (dict(inputfile=ALI_INPUT, toplim="x"), ValueError, "Inappropriate toplim value"),
                             (dict(inputfile=ALI_INPUT, rankby="q"), AssertionError, "Inappropriate rankby value"),
                             (dict(inputfile=ALI_INPUT, levellimit="x"), ValueError, "Inappropriate levellimit value"),
                             (dict(inputfile=ALI_INPUT, configfile="nope"), AssertionError, "Config file does not exist"),
                             (dict(inputfile=os.path.join(DATA, "examples", "seq_input.fas")), AssertionError, "The sequences are not aligned")):
            with pytest.raises(exc, match=msg) as mine:
                FoldAlignment(**kw)
            with pytest.raises(exc, match=msg) as theirs:
                Predict(alignment=True, write_to=io.StringIO(), **kw)
            assert str(mine.value) == str(theirs.value)
        for kw in (dict(verbose=True), dict(v=True), dict(entropy=True), dict(rfam=True), dict(g4=True), dict(rbp=True)):
            with pytest.raises(ValueError, match="FoldAlignment does not cover .*: use Predict"):
                FoldAlignment(inputfile=ALI_INPUT, **kw)


def test_fold_still_refuses_alignment_mode():
    from squarna_amd import Fold
    with E.use_engine(OracleEngine()):
        with pytest.raises(ValueError, match="Fold does not cover alignment mode: use Predict"):
            Fold(inputfile=ALI_INPUT, alignment=True)
