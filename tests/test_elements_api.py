"""CPU tests of Elements() through the tests' CPU engine (no elements_tensors: the host path): the literal table of the
specification in the three forms, random rows against the naive reference of tests/elements_checks.py, the levels against
PairsToDBN, invalid rows, degenerate shapes, the arithmetic of the result's helpers and the argument errors.  All exact."""
import numpy as np
import pytest

from tests import elements_checks as EC
from tests import score_checks as SC

INVALID = [case for case in SC.INVALID if case[0] != "nothing_to_score"]


@pytest.fixture(autouse=True)
def cpu_engine():
    from squarna_amd import engine as E
    from tests.oracle_engine import OracleEngine
    with E.use_engine(OracleEngine()):
        yield


def _elements(**kw):
    from squarna_amd import Elements
    res = Elements(**kw)
    assert res.source == "host" and res.recomputed == 0 and not res.element.is_cuda
    return res


def test_the_literal_table_in_three_forms():
    import torch
    cs = EC.table_cases()
    recs = [c["seq"] for c in cs]
    a = _elements(records=recs, structures=SC.strings_form(cs))
    padded, nstruct = SC.padded_form(cs, extra=3)
    b = _elements(records=recs, structures=padded, nstruct=nstruct)
    c = _elements(records=recs, structures=torch.from_numpy(padded).long())
    d = _elements(structures=SC.fold_result_form(cs))
    for res in (a, b, c, d):
        EC.check_table(res)
    assert a.element.dtype == torch.int8 and a.level.dtype == torch.int16 and a.loop_of.dtype == torch.int32
    assert a.loops.dtype == torch.int32 and a.loop_off.dtype == torch.int64 and a.cell_off.dtype == torch.int64
    assert a.names == [">record%d" % (k + 1) for k in range(len(cs))] and d.names == [">t%d" % k for k in range(len(cs))]


def test_known_structures_are_the_default_rows():
    seq, dbn, text, loops = EC.TABLE[3]
    res = _elements(records=[(">k", seq, None, None, dbn), (">none", "ACGU", None, None, None)])
    assert res.row_off.tolist() == [0, 1, 1] and res.text(0) == text and res.loops_of(0) == loops


@pytest.mark.parametrize("gaps,sep", [(False, False), (True, False), (False, True), (True, True)])
def test_random_rows_against_the_naive_reference(gaps, sep):
    """Also: the generator's rows stay inside what the kernels keep on the device (tests/test_hip_elements.py relies on it)."""
    from squarna_amd import device_calls as dc
    from squarna_amd.dbn import PairsToStems
    from squarna_amd.rows import row_pairs
    made = [EC.random_row(7 * w + k, w, k=k, gaps=gaps, sep=sep) for w in (5, 30, 64, 150, 263) for k in range(7)]
    recs, rows = [seq for seq, _ in made], [[row] for _, row in made]
    res = _elements(records=recs, structures=EC.padded(rows)[0])
    EC.check_naive(res, recs, rows)
    assert int(res.nlevels.max()) < dc.ELEMENTS_MAX_LEVELS and int(res.nlevels.max()) >= 3
    assert max(len(PairsToStems(row_pairs(row))) for _, row in made) < dc.ELEMENTS_MAX_STEMS
    kinds = set(res.loops[:, 0].tolist())
    assert kinds == {EC.E, EC.H, EC.B, EC.I, EC.M}, kinds            # the generator reaches every loop type


def test_mixed_records_against_the_naive_reference():
    recs, rows = EC.mixed_records()
    assert [len(r) for r in rows] == [0, 1, 2, 3, 4, 5, 6]
    res = _elements(records=recs, structures=[[EC.row_dbn(row) for row in rr] for rr in rows])
    EC.check_naive(res, recs, rows)
    pad, nstruct = EC.padded(rows, extra=2)
    EC.equal_results(res, _elements(records=recs, structures=pad, nstruct=nstruct))


def test_dbn_is_pairs_to_dbn():
    """The levels print as PairsToDBN prints the row, also with more levels than the four bracket kinds."""
    from squarna_amd.dbn import PairsToDBN
    from squarna_amd.rows import row_pairs
    made = [EC.random_row(90 + k, 120, k=k) for k in range(8)]
    ladder = np.full(60, -1, np.int32)                               # 30 pairs that all cross one another: 30 levels
    ladder[:30], ladder[30:] = np.arange(30, 60), np.arange(30)
    made.append(("A" * 60, ladder))
    res = _elements(records=[seq for seq, _ in made], structures=EC.padded([[row] for _, row in made])[0])
    assert res.nlevels.tolist()[-1] == 30
    for q, (_, row) in enumerate(made):
        assert res.dbn(q) == PairsToDBN(row_pairs(row), len(row)), q
        assert int(res.npairs[q]) == len(row_pairs(row))


@pytest.mark.parametrize("name,seq,row", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_rows(name, seq, row):
    good = np.full(len(seq), -1, np.int32)
    pad = np.stack([good, np.asarray(row, np.int32)])[None]
    with pytest.raises(ValueError, match=r"^Elements: record 0 \(>r\), row 1: not a valid structure of the record$"):
        _elements(records=[(">r", seq, None, None, None)], structures=pad)
    res = _elements(records=[(">r", seq, None, None, None)], structures=pad, strict=False)
    n = len(seq)
    assert res.status.tolist() == [0, 1] and res.nloops.tolist() == [1, 0] and res.loop_off.tolist() == [0, 1, 1]
    assert res.element[n:].tolist() == [-1] * n and res.level[n:].tolist() == [0] * n and res.loop_of[n:].tolist() == [-1] * n
    assert res.text(1) == "?" * n and res.loops_of(1) == [] and res.npairs.tolist()[1] == 0
    EC.check_naive(res, [seq], [[good, row]])


def test_a_record_with_nothing_to_score_is_valid():
    res = _elements(records=["-&-"], structures=[["..."]])
    assert res.status.tolist() == [0] and res.text(0) == "-&-" and res.loops_of(0) == [(0, -1, 3, 0, 0, 0)]


def test_widths_zero_and_one_and_no_rows():
    res = _elements(records=["", "A", "ACGU"], structures=[[""], ["."], []])
    assert res.row_off.tolist() == [0, 1, 2, 2] and res.cell_off.tolist() == [0, 0, 1]
    assert res.loops_of(0) == [(0, -1, 0, 0, 0, 0)] and res.loops_of(1) == [(0, -1, 1, 0, 1, 1)]
    assert res.text(0) == "" and res.text(1) == "E" and res.dbn(1) == "."
    none = _elements(records=["ACGU", "GG"], structures=[[], []])
    assert none.row_off.tolist() == [0, 0, 0] and tuple(none.loops.shape) == (0, 6) and none.element.numel() == 0
    assert tuple(none.to_padded().shape) == (0, 0) and tuple(none.composition().shape) == (0, 9) and tuple(none.one_hot().shape) == (0, 9)


def test_padded_one_hot_and_composition():
    import torch
    cs = EC.table_cases()
    res = _elements(records=[c["seq"] for c in cs], structures=SC.strings_form(cs))
    pad = res.to_padded()
    assert pad.dtype == torch.int8 and tuple(pad.shape) == (len(cs), 24)
    hot = res.one_hot()
    assert tuple(hot.shape) == (int(res.cell_off[-1]), 9) and hot.sum(1).tolist() == [1] * int(res.cell_off[-1])
    comp = res.composition()
    assert comp.dtype == torch.float64 and tuple(comp.shape) == (len(cs), 9)
    for q, (seq, _, text, _) in enumerate(EC.TABLE):
        codes = [EC.LETTERS.index(ch) for ch in text]
        assert pad[q].tolist() == codes + [-1] * (24 - len(seq))
        assert res.to_padded(fill=9)[q].tolist() == codes + [9] * (24 - len(seq))
        a = int(res.cell_off[q])
        assert hot[a:a + len(seq)].argmax(1).tolist() == codes
        nongap = len(seq) - text.count("-")
        assert comp[q].tolist() == [0.0 if k == 8 else codes.count(k) / nongap for k in range(9)]
    bad = _elements(records=["GGGAAACCC", "---"], structures=np.array([[SC.INVALID[0][2]], [[-1] * 9]], np.int32), strict=False)
    assert bad.one_hot()[:9].sum().item() == 0 and bool(torch.isnan(bad.composition()).all())
    assert bad.text(1) == "---" and bad.status.tolist() == [1, 0]


def test_argument_errors():
    from squarna_amd import Elements
    from squarna_amd.score import MAX_LENGTH
    with pytest.raises(ValueError, match=r"^Elements: structures for 1 records, 2 records"):
        Elements(records=["ACGU", "ACGU"], structures=[["...."]])
    with pytest.raises(ValueError, match=r"^Elements: record 0 \(>record1\), row 0: a structure of 3 columns for 4"):
        Elements(records=["ACGU"], structures=[["..."]])
    with pytest.raises(ValueError, match=r"^Elements: nstruct belongs to the padded form"):
        Elements(records=["ACGU"], structures=[["...."]], nstruct=[1])
    with pytest.raises(ValueError, match=r"^Elements: structures of shape"):
        Elements(records=["ACGU"], structures=np.full((1, 1, 3), -1, np.int32))
    with pytest.raises(ValueError, match=r"^Elements: nstruct must hold 1 numbers between 0 and 1"):
        Elements(records=["ACGU"], structures=np.full((1, 1, 4), -1, np.int32), nstruct=[2])
    with pytest.raises(ValueError, match=r"^Elements: structures of dtype"):
        Elements(records=["ACGU"], structures=np.full((1, 1, 4), -1.0))
    with pytest.raises(ValueError, match=r"^Elements: the FoldResult's records are not the given records"):
        Elements(records=["ACGU"], structures=SC.fold_result_form(EC.table_cases()[:1]))
    with pytest.raises(ValueError, match=r"^Elements: record >long has %d nt; at most %d" % (MAX_LENGTH + 1, MAX_LENGTH)):
        Elements(records=[(">long", "A" * (MAX_LENGTH + 1), None, None, None)], structures=[[]])
    with pytest.raises(AssertionError):
        Elements(records=[], structures=[])
