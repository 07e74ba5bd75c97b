"""CPU tests of Fold() / FoldResult (no GPU): the host layer of the bulk results API against the CPU oracle through the
test-only OracleEngine -- an engine without fold_tensors, for which Fold builds the same FoldResult on the CPU -- and
against the reference's own output text (tests/golden/text/*.txt).  All comparisons are exact."""
import io
import os

import numpy as np
import pytest

from squarna_amd import engine as E
from tests.fold_checks import DATA, check_against_golden, check_against_tuples, check_dense_forms
from tests.oracle_engine import OracleEngine

SEQ_INPUT = os.path.join(DATA, "examples", "seq_input.fas")
S16 = "ACGUACGUACUCGACG"


def oracle_tuples(inputfile=None, inputseq=None, configfile="nobpp", records=None, **opts):
    """What the engine returns for the same records: its SQRNdbnseq tuples, in input order."""
    from squarna_amd.config import ParseConfig, builtin_config
    from squarna_amd.inputs import ParseInput
    _, psets = ParseConfig(builtin_config(configfile))
    if records is None:
        with open(os.devnull, "w") as sink:
            import contextlib
            with contextlib.redirect_stdout(sink):
                records = list(ParseInput(inputseq, inputfile, "qtrf")[0])
    recs = [(r, None, None, None, psets, None) if isinstance(r, str) else (r[1], r[2], r[3], r[4], psets, None) for r in records]
    opts.setdefault("rankby", (2, 0, 1))                                 # Predict's default rankby="r" (SQUARNA.py:810-820)
    return OracleEngine().fold_records(recs, **opts)


def fold(**kw):
    from squarna_amd import Fold
    with E.use_engine(OracleEngine()):
        return Fold(**kw)


def test_fold_equals_engine_tuples_and_golden_text_file():
    res = fold(inputfile=SEQ_INPUT, configfile="nobpp")
    assert res.source == "host" and res.partner.device.type == "cpu"
    check_against_tuples(res, oracle_tuples(inputfile=SEQ_INPUT), keep=5)
    check_against_golden(res, "seq_input_nobpp")
    check_dense_forms(res)


def test_fold_equals_engine_tuples_and_golden_text_inputseq():
    res = fold(inputseq=S16, configfile="nobpp")
    assert res.names == [">inputseq"] and res.sequences == [S16]
    check_against_tuples(res, oracle_tuples(inputseq=S16), keep=5)
    check_against_golden(res, "s16_nobpp")
    # synonyms and the data directory's lookup as in Predict
    res2 = fold(s=S16, c="nobpp", tl=5)
    assert res2.partner.tolist() == res.partner.tolist() and res2.scores.tolist() == res.scores.tolist()


def test_fold_prints_nothing(capsys):
    fold(inputfile=SEQ_INPUT, configfile="nobpp", outplim=1)
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""


def test_gapped_and_separated_records_use_input_coordinates():
    recs = ["GGGAAA-CCC&GGG..AAACCC", ("named", "GG-GGAAAACC~CC", None, "(.-..........)", "((-((....))~))"), "CCCAAAAGGG;CCCAAAAGGG"]
    res = fold(records=recs, configfile="nobpp")
    assert res.names == [">record1", "named", ">record3"]
    tuples = oracle_tuples(records=[(None, r, None, None, None) if isinstance(r, str) else r for r in recs])
    check_against_tuples(res, tuples, keep=5)
    for r, seq in enumerate(res.sequences):
        o, n = int(res.cell_off[r]), len(seq)
        for k in range(1 + int(res.nstruct[r])):
            row = res.partner[o + k * n:o + (k + 1) * n].tolist()
            for i, ch in enumerate(seq):
                if ch in "-.~;&":
                    assert row[i] == -1 and i not in row
    assert res.consensus(0)[10] == "&" and res.consensus(2)[10] == ";"
    assert res.metrics[1, :3].tolist() == [4.0, 0.0, 0.0]                 # the known structure of the gapped record, found
    check_dense_forms(res)


class NoParamsetEngine(OracleEngine):
    """The second record folds under no paramset at all: the reference then returns no structure (SQRNdbnseq.py:1201-1236)."""

    def fold_records(self, records, **opts):
        records = [rec if k != 1 else rec[:4] + ([],) + rec[5:] for k, rec in enumerate(records)]
        return OracleEngine.fold_records(self, records, **opts)


def test_record_without_structure():
    from squarna_amd import Fold
    with E.use_engine(NoParamsetEngine()):
        res = Fold(records=["GGGAAACCC", "GGGGAAAACCCC", S16], configfile="nobpp")
    assert res.nstruct.tolist()[1] == 0 and res.nstruct.tolist()[0] > 0
    o = int(res.cell_off[1])
    assert res.partner[o:int(res.cell_off[2])].tolist() == [-1] * 12
    assert res.consensus(1) == "." * 12
    assert int(res.row_off[1]) == int(res.row_off[2])
    with pytest.raises(IndexError):
        res.pairs(1, 0)
    assert res.dbn(2, 0) == fold(inputseq=S16, configfile="nobpp").dbn(0, 0)
    check_dense_forms(res)


def test_outplim_below_and_above_the_number_of_structures():
    tuples = oracle_tuples(inputfile=SEQ_INPUT)
    most = max(len(t[1]) for t in tuples)
    assert most > 2
    low = fold(inputfile=SEQ_INPUT, configfile="nobpp", outplim=2)
    assert low.nstruct.tolist() == [min(2, len(t[1])) for t in tuples]
    check_against_tuples(low, tuples, keep=2)
    high = fold(inputfile=SEQ_INPUT, configfile="nobpp", ol=most + 50)
    assert high.nstruct.tolist() == [len(t[1]) for t in tuples]
    check_against_tuples(high, tuples)


def test_several_batches_equal_one(monkeypatch):
    from squarna_amd import api
    one = fold(inputfile=SEQ_INPUT, configfile="nobpp")
    monkeypatch.setattr(api, "BATCH_RECORDS", 3)
    many = fold(inputfile=SEQ_INPUT, configfile="nobpp")
    monkeypatch.setattr(api, "BATCH_RECORDS", 16384)
    monkeypatch.setattr(api, "BATCH_CELLS", 1)
    each = fold(inputfile=SEQ_INPUT, configfile="nobpp")
    for other in (many, each):
        assert other.names == one.names and other.sequences == one.sequences
        for key in ("lengths", "nstruct", "row_off", "cell_off", "partner", "pset_mask"):
            assert getattr(other, key).tolist() == getattr(one, key).tolist(), key
        assert other.scores.numpy().tobytes() == one.scores.numpy().tobytes()
        assert other.metrics.numpy().tobytes() == one.metrics.numpy().tobytes()


def test_join_reorders_and_moves_gap_free_tables_into_input_coordinates():
    """The assembly step of the GPU path on CPU tensors: gap-free tables of two engine calls, records interleaved."""
    import torch
    from squarna_amd.fold import _join
    seqs = ["GG-AAACC", "ACGU", "G.GGAAAC-CC", "CCAAAGG"]

    def part(idx, rows_of):
        """Tables of the records idx: rows_of[k] = the partner rows (gap-free) of record k, consensus first."""
        partner = np.concatenate([np.array(r, np.int32) for k in idx for r in rows_of[k]])
        ns = np.array([len(rows_of[k]) - 1 for k in idx], np.int64)
        ln = np.array([len(rows_of[k][0]) for k in idx], np.int64)
        first = {k: sum(len(rows_of[q]) - 1 for q in idx[:idx.index(k)]) for k in idx}
        scores = np.array([[100.0 * k + j, 0.5, 0.25] for k in idx for j in range(len(rows_of[k]) - 1)], np.float64).reshape(-1, 3)
        masks = np.array([(k << 8) | j for k in idx for j in range(len(rows_of[k]) - 1)], np.int64)
        metrics = np.array([[float(k)] * 16 for k in idx])
        assert first[idx[0]] == 0
        t = dict(partner=torch.from_numpy(partner), scores=torch.from_numpy(scores), pset_mask=torch.from_numpy(masks),
                 metrics=torch.from_numpy(metrics))
        return (t, ns, ln, idx, True)
    rows_of = {0: [[6, 5, -1, -1, -1, 1, 0]] * 2,                           # GGAAACC: (0,6) (1,5)
               1: [[-1] * 4],                                                 # no structure row at all
               2: [[8, 7, 6, -1, -1, -1, 2, 1, 0], [8, 7, 6, -1, -1, -1, 2, 1, 0], [-1, 7, 6, -1, -1, -1, 2, 1, -1]],
               3: [[6, 5, -1, -1, -1, 1, 0], [6, 5, -1, -1, -1, 1, 0]]}
    tables, nstruct, lengths = _join([part([2, 0], rows_of)[:5], part([1, 3], rows_of)[:5]], seqs)
    assert nstruct.tolist() == [1, 0, 2, 1] and lengths.tolist() == [8, 4, 11, 7]
    exp = ([7, 6, -1, -1, -1, -1, 1, 0] * 2 + [-1] * 4 +
           [10, -1, 9, 7, -1, -1, -1, 3, -1, 2, 0] * 2 + [-1, -1, 9, 7, -1, -1, -1, 3, -1, 2, -1] + [6, 5, -1, -1, -1, 1, 0] * 2)
    assert tables["partner"].tolist() == exp
    assert tables["scores"][:, 0].tolist() == [0.0, 200.0, 201.0, 300.0]
    assert tables["pset_mask"].tolist() == [0, 512, 513, 768]
    assert tables["metrics"][:, 0].tolist() == [0.0, 1.0, 2.0, 3.0]


def test_tables_of_consecutive_batches_are_joined_with_rebased_offsets():
    """engine._join_runs (the sub-batches of HipEngine.fold_tensors) on CPU tensors."""
    import torch
    from squarna_amd.engine import _TensorRun, _join_runs

    def run(nstruct, lengths, source, tag):
        ns, ln = np.array(nstruct, np.int64), np.array(lengths, np.int64)
        rows, cells = int(ns.sum()), int(((1 + ns) * ln).sum())
        row_off, cell_off = np.zeros(len(ns) + 1, np.int64), np.zeros(len(ns) + 1, np.int64)
        np.cumsum(ns, out=row_off[1:])
        np.cumsum((1 + ns) * ln, out=cell_off[1:])
        t = dict(partner=torch.arange(cells, dtype=torch.int32) + 1000 * tag, scores=torch.full((rows, 3), float(tag), dtype=torch.float64),
                 pset_mask=torch.full((rows,), tag, dtype=torch.int64), metrics=torch.full((len(ns), 16), float(tag), dtype=torch.float64),
                 row_off=torch.from_numpy(row_off), cell_off=torch.from_numpy(cell_off))
        return _TensorRun(t, ns, ln, source)
    a, b, c = run([2, 0], [5, 3], "device", 1), run([1], [4], "device", 2), run([3, 1], [2, 6], "host", 3)
    one = _join_runs([a])
    assert one["source"] == "device" and one["row_off"].tolist() == [0, 2, 2] and one["cell_off"].tolist() == [0, 15, 18]
    out = _join_runs([a, b, c])
    assert out["source"] == "mixed" and _join_runs([a, b])["source"] == "device" and _join_runs([c])["source"] == "host"
    assert out["nstruct"].tolist() == [2, 0, 1, 3, 1] and out["lengths"].tolist() == [5, 3, 4, 2, 6]
    assert out["row_off"].tolist() == [0, 2, 2, 3, 6, 7]
    assert out["cell_off"].tolist() == [0, 15, 18, 26, 34, 46]
    assert out["partner"].tolist() == a.tables["partner"].tolist() + b.tables["partner"].tolist() + c.tables["partner"].tolist()
    assert out["pset_mask"].tolist() == [1, 1, 2, 3, 3, 3, 3] and out["scores"][:, 0].tolist() == [1, 1, 2, 3, 3, 3, 3]
    assert out["metrics"][:, 0].tolist() == [1, 1, 2, 3, 3]


def test_packed_records_to_pair_tables():
    """The conversion a batch whose tail ran on the host takes (engine.fold_tensors): bracket levels -> partners."""
    import struct
    from squarna_amd.results import packed_pair_tables
    lev = {"(": 1, ")": -1, "[": 2, "]": -2, "{": 3, "}": -3, ".": 0}
    recs = [["((..[[..))..]]", "((..[[..))..]]", "(.[.{.).].}..."], ["....."], ["(())", "(())", "()()", "...."]]
    buf, off = b"", [0]
    for rows in recs:
        ns, n = len(rows) - 1, len(rows[0])
        rec = struct.pack("<4q", ns, n, 0, 7) + struct.pack("<16d", *range(16))
        rec += b"".join(struct.pack("<3d", k, 2 * k, 0.5) for k in range(ns)) + b"".join(struct.pack("<Q", 1 << k) for k in range(ns))
        rec += b"".join(struct.pack("<%dh" % n, *[lev[c] for c in row]) for row in rows)
        buf += rec + b"\0" * (-len(rec) % 8)
        off.append(len(buf))
    t, nstruct, lengths = packed_pair_tables(np.frombuffer(buf, np.uint8), np.array(off, np.int64))
    from squarna_amd.dbn import DBNToPairs
    assert nstruct.tolist() == [2, 0, 3] and lengths.tolist() == [14, 5, 4]
    assert t["row_off"].tolist() == [0, 2, 2, 5] and t["cell_off"].tolist() == [0, 42, 47, 63]
    flat = [row for rows in recs for row in rows]
    pos = 0
    for row in flat:
        exp = [-1] * len(row)
        for v, w in DBNToPairs(row):
            exp[v], exp[w] = w, v
        assert t["partner"][pos:pos + len(row)].tolist() == exp
        pos += len(row)
    assert t["scores"].tolist() == [[0, 0, 0.5], [1, 2, 0.5], [0, 0, 0.5], [1, 2, 0.5], [2, 4, 0.5]]
    assert t["pset_mask"].tolist() == [1, 2, 1, 2, 4] and t["metrics"][2].tolist() == list(range(16))


def test_rejected_modes_and_validation():
    from squarna_amd import Fold
    with E.use_engine(OracleEngine()):
        for kw in (dict(alignment=True), dict(a=True), dict(evalonly=True), dict(entropy=True), dict(rfam=True), dict(g4=True),
                   dict(rbp=True)):
            with pytest.raises(ValueError, match="Fold does not cover"):
                Fold(inputseq=S16, configfile="nobpp", **kw)
        with pytest.raises(AssertionError, match="Input file does not exist"):
            Fold(inputfile="/nonexistent/file.fas")
        with pytest.raises(ValueError, match="Inappropriate toplim value"):
            Fold(inputseq=S16, configfile="nobpp", toplim="x")
        with pytest.raises(AssertionError, match="Inappropriate rankby value"):
            Fold(inputseq=S16, configfile="nobpp", rankby="q")
        with pytest.raises(AssertionError, match="Config file does not exist"):
            Fold(inputseq=S16, configfile="nope")


def test_predict_text_is_unchanged_beside_fold():
    """Fold shares Predict's parsers and batching limits: Predict's text for the same input stays the golden one."""
    from squarna_amd import Predict
    buf = io.StringIO()
    with E.use_engine(OracleEngine()):
        fold(inputfile=SEQ_INPUT, configfile="nobpp")
        Predict(inputfile=SEQ_INPUT, configfile="nobpp", write_to=buf)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text", "seq_input_nobpp.txt")) as f:
        assert buf.getvalue() == f.read()
