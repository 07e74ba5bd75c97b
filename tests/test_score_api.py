"""CPU tests of Score() / ScoreResult (no GPU): through the test-only OracleEngine -- an engine without score_tensors, for
which Score builds the same ScoreResult on the CPU -- against the values the reference returned (tests/golden/score.json)
and the reference lines of its evalonly output (tests/golden/text/seq_input_evalonly.txt).  All comparisons are exact."""
import os

import numpy as np
import pytest

from squarna_amd import Score, ScoreResult
from squarna_amd import engine as E
from tests import score_checks as SC
from tests.fold_checks import DATA
from tests.oracle_engine import OracleEngine

SEQ_INPUT = os.path.join(DATA, "examples", "seq_input.fas")


def score(**kw):
    with E.use_engine(OracleEngine()):
        return Score(**kw)


def _is_host(res):
    import torch
    assert isinstance(res, ScoreResult) and res.source == "host" and res.device.type == "cpu"
    rows = int(res.row_off[-1])
    for key, dt, shape in (("scores", torch.float64, (rows, 3)), ("metrics", torch.float64, (rows, 6)), ("status", torch.int32, (rows,)),
                           ("nstems", torch.int32, (rows,)), ("npairs", torch.int32, (rows,)), ("stem_off", torch.int64, (rows + 1,)),
                           ("ref_scores", torch.float64, (len(res), 3)), ("row_off", torch.int64, (len(res) + 1,))):
        t = getattr(res, key)
        assert t.dtype == dt and tuple(t.shape) == shape, key
    assert res.stems.dtype == torch.int32 and tuple(res.stems.shape) == (int(res.stem_off[-1]), 3)


def test_golden_cases_as_strings():
    cs = SC.cases()
    res = score(records=SC.records_of(cs), structures=SC.strings_form(cs))
    _is_host(res)
    assert res.names == [">" + c["name"] for c in cs] and res.sequences == [c["seq"] for c in cs]
    SC.check_golden(res, cs)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_golden_cases_as_padded_partners(as_tensor):
    import torch
    cs = SC.cases()
    padded, nstruct = SC.padded_form(cs, extra=3)
    res = score(records=SC.records_of(cs), structures=torch.from_numpy(padded) if as_tensor else padded, nstruct=nstruct)
    _is_host(res)
    SC.check_golden(res, cs)


def test_golden_cases_as_fold_result():
    cs = SC.cases()
    res = score(records=SC.records_of(cs), structures=SC.fold_result_form(cs))
    _is_host(res)
    SC.check_golden(res, cs)


def test_fold_result_alone_brings_its_sequences():
    cs = [c for c in SC.cases() if not c["reacts"]][:12]
    fr = SC.fold_result_form(cs)
    res = score(structures=fr)
    assert res.sequences == fr.sequences and res.names == fr.names
    SC.equal_results(res, score(records=[(">" + c["name"], c["seq"], None, None, None) for c in cs], structures=SC.strings_form(cs)))
    assert bool(np.isnan(res.metrics.numpy()).all()) and bool(np.isnan(res.ref_scores.numpy()).all())


def test_structures_none_is_evalonly():
    """Every record's known structure as its only row: the three numbers of the reference's `reference` lines."""
    want = []
    with open(os.path.join(SC.GOLDEN, "text", "seq_input_evalonly.txt")) as f:
        for line in f:
            parts = line.rstrip("\n").split("\t")
            if len(parts) == 5 and parts[1] == "reference":
                want.append([float(x) for x in parts[2:]])
    assert want
    res = score(inputfile=SEQ_INPUT)
    nrow = np.diff(res.row_off.numpy())
    assert set(nrow.tolist()) == {0, 1} and int(nrow.sum()) == len(want)
    assert SC.same(res.scores.numpy(), want)
    assert SC.same(res.ref_scores.numpy()[nrow == 1], want) and bool(np.isnan(res.ref_scores.numpy()[nrow == 0]).all())
    # a known structure against itself: everything found, nothing else
    tp = res.npairs.numpy().astype(np.float64)
    assert SC.same(res.metrics.numpy(), np.stack([tp, 0 * tp, 0 * tp, 1 + 0 * tp, 1 + 0 * tp, 1 + 0 * tp], axis=1))


def test_the_sweep_of_the_metric_ratios_is_not_blind():
    """A condition on the sweep's INPUTS (tests/score_checks.sweep; run in full by tests/test_hip_score.py): its ratios hold
    enough distinct (numerator, denominator) on which a subtly wrong round(x, 3) gives another value than the right one --
    half up on the product, e.g. 9/16 = 0.5625 -> 0.563, and ties to even on the ROUNDED product, e.g. 1/80, whose double
    lies above 0.0125 while 1000 x rounds to 12.5 exactly -> 0.012."""
    counts = SC.sweep_counts()
    assert len(counts) == 6422 and len(set(counts)) == 6422
    floor_up, product = SC.sweep_telling(SC.round3_floor), SC.sweep_telling(SC.round3_product)
    assert len(floor_up) >= 40 and len(product) >= 20, (len(floor_up), len(product))
    assert {(9, 16), (13, 16), (10, 32), (52, 64)} <= floor_up and {(1, 80), (3, 80), (7, 80)} <= product
    recs, rows, nstruct, want = SC.sweep()
    assert rows.shape == (6, 2597, 200) and rows.dtype == np.int32 and int(nstruct.sum()) == 6422 and want.shape == (6422, 6)
    flat = np.concatenate([rows[r, :k] for r, k in enumerate(nstruct)])
    assert ((flat >= 0).sum(1) == 2 * (want[:, 0] + want[:, 1])).all()                              # TP + FP pairs in every row


def test_a_thinned_sweep_of_the_metric_ratios_on_the_host():
    """Every row of the sweep that holds a ratio on which one of the two wrong roundings differs, and every thirtieth of
    the others, through the host path: TP FP FN FS PR RC equal plain Python's, bit for bit."""
    recs, rows, nstruct, want = SC.sweep()
    telling = SC.sweep_telling(SC.round3_floor) | SC.sweep_telling(SC.round3_product)
    counts = SC.sweep_counts()
    holds = np.array([any(r in telling for r in SC.sweep_ratios(*c).values()) for c in counts])
    other = np.flatnonzero(~holds)
    pick = np.sort(np.concatenate([np.flatnonzero(holds), other[::len(other) // 200]]))
    assert int(holds.sum()) > 1000 and 200 <= len(pick) - int(holds.sum()) <= 210
    first = np.concatenate([[0], np.cumsum(nstruct)])
    per_record = [pick[(pick >= first[r]) & (pick < first[r + 1])] - first[r] for r in range(len(recs))]
    thin = np.full((len(recs), max(len(p) for p in per_record), rows.shape[2]), -1, np.int32)
    for r, p in enumerate(per_record):
        thin[r, :len(p)] = rows[r, p]
    res = score(records=recs, structures=thin, nstruct=[len(p) for p in per_record])
    _is_host(res)
    assert res.status.count_nonzero().item() == 0 and res.npairs.tolist() == (want[pick, 0] + want[pick, 1]).tolist()
    got = res.metrics.numpy()
    assert got.tobytes() == want[pick].tobytes(), [(counts[q], g.tolist(), w.tolist()) for q, g, w in zip(pick, got, want[pick]) if g.tobytes() != w.tobytes()][:5]


INVALID = SC.INVALID


@pytest.mark.parametrize("name,seq,row", INVALID, ids=[x[0] for x in INVALID])
def test_invalid_rows(name, seq, row):
    good = SC.partner_row("(" + "." * (len(seq) - 2) + ")") if name != "nothing_to_score" else np.full(len(seq), -1, np.int32)
    padded = np.stack([np.asarray(row, np.int32), good])[None]
    with pytest.raises(ValueError, match=r"record 0 \(>r\), row 0"):
        score(records=[(">r", seq, None, None, None)], structures=padded)
    res = score(records=[(">r", seq, None, None, None)], structures=padded, strict=False)
    bad_too = name == "nothing_to_score"                           # (the record itself cannot be scored: every row of it)
    assert res.status.tolist() == [1, 1 if bad_too else 0]
    assert bool(np.isnan(res.scores[0].numpy()).all()) and bool(np.isnan(res.metrics[0].numpy()).all())
    assert res.nstems.tolist()[0] == 0 and res.npairs.tolist()[0] == 0
    if not bad_too:
        assert res.scores[1].tolist()[2] == 0.5
        assert res.stems_of(1) == [(0, len(seq) - 1, 1)]


def test_argument_errors():
    rec = [(">r", "GGGAAACCC", None, None, None)]
    with pytest.raises(ValueError, match="8 columns for 9"):
        score(records=rec, structures=[["(((..)))"]])
    with pytest.raises(ValueError, match="Lmax >= 9"):
        score(records=rec, structures=np.full((1, 2, 8), -1, np.int32))
    with pytest.raises(ValueError, match="nstruct"):
        score(records=rec, structures=np.full((1, 2, 9), -1, np.int32), nstruct=[3])
    with pytest.raises(ValueError, match="2 records"):
        score(records=rec * 2, structures=[["(((...)))"]])
    with pytest.raises(ValueError, match="reactivities"):
        score(records=[(">r", "GGGAAACCC", [0.5] * 8, None, None)], structures=[["(((...)))"]])
    with pytest.raises(ValueError, match="at most 32768"):
        score(records=["A" * 32769], structures=[[]])
    assert score(records=["A" * 32768], structures=[[]]).row_off.tolist() == [0, 0]


def test_ragged_rows_and_a_record_without_any():
    cs = SC.cases()
    pick = [cs[0], cs[8], cs[3], cs[20], cs[30]]
    structures = SC.strings_form(pick)
    structures[2] = []                                             # K = 0
    structures[4] = structures[4][:1]
    res = score(records=SC.records_of(pick), structures=structures)
    counts = [len(s) for s in structures]
    assert res.row_off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    trimmed = [dict(c, rows=c["rows"][:k]) for c, k in zip(pick, counts)]
    SC.check_golden(res, trimmed)
    # the same rows from the padded form, whose unused rows are not read
    padded, _ = SC.padded_form(pick)
    padded[2, :, :] = 77
    SC.equal_results(res, score(records=SC.records_of(pick), structures=padded, nstruct=counts))


def test_restraints_are_ignored_and_letters_are_normalised():
    a = score(records=[(">r", "gggaaatcc", None, "(.......)", "((.....))")], structures=[["(((...)))"]])
    b = score(records=[(">r", "GGGAAAUCC", None, None, "((.....))")], structures=[["(((...)))"]])
    assert a.sequences == ["gggaaatcc"]
    assert a.scores.tolist() == b.scores.tolist() and a.metrics.tolist() == b.metrics.tolist()
    assert a.ref_scores.tolist() == b.ref_scores.tolist()
