"""``Score``: scores and metrics of GIVEN structures as data.

``Predict(evalonly=True)`` prints one line of text per record for its one known structure; ``Score`` takes any number of
structures per record -- dot-bracket strings, a padded tensor of partners such as ``FoldResult.to_padded()`` returns, or a
``FoldResult`` -- and returns a :class:`ScoreResult`: for every structure what the reference computes for a ``reference``
line, ``ReferenceScores`` (SQRNdbnseq.py:958-970) = ``ScoreStruct`` of ``PairsToStems(sorted(pairs))`` on the gap-free
sequence, its stems, and TP FP FN FS PR RC against the record's known structure (:1249-1258).  With the GPU engine the rows
are scored by a kernel (``sq_score_structs_dev``), one wave per row, and a tensor of partners that is on the device already
is read where it is; an engine without ``score_tensors`` (the tests' CPU engine) gets the same object built on the CPU.
"""
import os

import numpy as np

from . import engine as _engine
from .align import PairMetrics
from .config import DATA_DIR
from .core import ScoreStruct
from .dbn import DBNToPairs, PairsToStems, ProcessReacts, ReactDict, SEPS, UnAlign, encode_seq, gap_mask
from .options import input_records
from .results import TensorResult
from .rows import offsets, partner_row

#: the ranking tail's position limit (its LDS bitmap of paired positions)
MAX_LENGTH = 32768

class ScoreRecord:
    """One record of ``Score`` after the host's pre-processing, done once per record however many rows it has: the sequence
    after upper() and T -> U (``seq``), its gap-free form (``short``, ``n`` positions, letter ``codes``), ``colmap`` (the
    gap-free position of every input column, -1 for a gap column), ``gfcol`` (the input column of every position),
    ``sepcol`` (input columns that hold a separator), ``nsep``, ``reacts`` (gap-free floats, or None: all 0.5), and the known
    structure: ``known`` (its gap-free pairs, sorted; None without one) and ``known_partner`` (int32[n], -1 unpaired)."""
    __slots__ = ("name", "given", "seq", "short", "n", "codes", "colmap", "gfcol", "has_gap", "sepcol", "nsep", "reacts", "known",
                 "known_partner")

    def __init__(self, name, seq, reacts=None, reference=None):
        self.name, self.given = name, seq
        up = seq.upper().replace("T", "U")                           # SQRNdbnseq.py:1004
        if len(up) != len(seq):
            raise ValueError("Score: record {}: a letter changes the sequence's length in upper case".format(name))
        self.seq = up
        gaps = gap_mask(up)
        self.has_gap = bool(gaps.any())
        self.gfcol = np.flatnonzero(~gaps).astype(np.int32)
        self.n = len(self.gfcol)
        if self.n > MAX_LENGTH:
            raise ValueError("Score: record {} has {} nt; at most {} are scored".format(name, self.n, MAX_LENGTH))
        self.colmap = np.where(gaps, -1, np.cumsum(~gaps) - 1).astype(np.int32)
        self.short = ''.join(up[c] for c in self.gfcol.tolist()) if self.has_gap else up
        self.codes = np.frombuffer(encode_seq(self.short), np.uint8)
        self.sepcol = np.fromiter((ch in SEPS for ch in up), bool, len(up))
        self.nsep = int(self.sepcol.sum())
        if reacts is not None and len(reacts):
            if len(reacts) != len(seq):
                raise ValueError("Score: record {}: {} reactivities for {} columns".format(name, len(reacts), len(seq)))
            if isinstance(reacts, str):                              # :1019-1020
                reacts = ProcessReacts([ReactDict[ch] for ch in reacts])
            self.reacts = np.asarray(reacts, np.float64)[~gaps].tolist()
        else:
            self.reacts = None
        self.known = None
        self.known_partner = partner_row((), self.n)
        if reference:
            if len(reference) != len(seq):
                raise ValueError("Score: record {}: a known structure of {} columns for {}".format(name, len(reference), len(seq)))
            self.known = DBNToPairs(UnAlign(up, reference)[1])       # :965-967
            self.known_partner = partner_row(self.known, self.n)

    def score(self, pairs):
        """ScoreStruct of gap-free sorted pairs under this record, or None where the reference divides by zero."""
        if self.n - self.nsep <= 0:
            return None
        return ScoreStruct(self.short, PairsToStems(pairs), self.reacts if self.reacts is not None else [0.5] * self.n)


def score_row_host(rec, row):
    """One partner row (input columns of ``rec``; longer rows: their first columns) on the CPU: (status, scores or None,
    metrics or None, stems [(i, j, len)] in input columns, number of pairs).  Status 1: a partner outside the record,
    p[p[i]] != i, p[i] == i, a pair on a separator, or a record without a position to score."""
    lin = len(rec.seq)
    row = np.asarray(row[:lin], np.int64)
    idx = np.flatnonzero(row != -1)
    p = row[idx]
    if ((p < 0) | (p >= lin) | (p == idx)).any() or (row[p] != idx).any() or rec.sepcol[idx].any() or rec.n - rec.nsep <= 0:
        return 1, None, None, [], 0
    up = idx[p > idx]
    v, w = rec.colmap[up], rec.colmap[row[up]]
    keep = (v >= 0) & (w >= 0)                                       # a pair that touches a gap column is dropped (:243-249)
    pairs = list(zip(v[keep].tolist(), w[keep].tolist()))
    stems = [(int(rec.gfcol[st[0][0][0]]), int(rec.gfcol[st[0][0][1]]), st[1]) for st in PairsToStems(pairs)]
    return 0, rec.score(pairs), (PairMetrics(rec.known, pairs) if rec.known is not None else None), stems, len(pairs)


def _score_host(recs, partner, row_start, row_rec):
    """The tables of ScoreResult on the CPU, as numpy arrays."""
    rows = len(row_rec)
    out = dict(scores=np.full((rows, 3), np.nan), metrics=np.full((rows, 6), np.nan), status=np.zeros(rows, np.int32),
               nstems=np.zeros(rows, np.int32), npairs=np.zeros(rows, np.int32), ref_scores=np.full((len(recs), 3), np.nan))
    stems = []
    for q in range(rows):
        rec = recs[row_rec[q]]
        st, sc, met, ss, npairs = score_row_host(rec, partner[row_start[q]:row_start[q] + len(rec.seq)])
        out["status"][q], out["nstems"][q], out["npairs"][q] = st, len(ss), npairs
        if sc is not None:
            out["scores"][q] = sc
        if met is not None:
            out["metrics"][q] = met
        stems.extend(ss)
    for r, rec in enumerate(recs):
        sc = rec.score(rec.known) if rec.known is not None else None
        if sc is not None:
            out["ref_scores"][r] = sc
    out["stems"] = np.array(stems, np.int32).reshape(-1, 3)
    out["stem_off"] = offsets(out["nstems"])
    return out


class ScoreResult(TensorResult):
    """Scores of ``Score`` for the structure rows of R records.

    Host lists: ``names``, ``sequences`` (as given).  Torch tensors (``device``: where they live): ``row_off`` int64[R + 1]
    -- record r's rows are row_off[r] .. row_off[r + 1]; per row ``scores`` float64[rows, 3] (total, structure, reactivity),
    ``metrics`` float64[rows, 6] (TP FP FN FS PR RC against the record's known structure; NaN without one), ``status``
    int32[rows] (0; 1: an invalid row, whose scores and metrics are NaN), ``npairs`` and ``nstems`` int32[rows] (after the
    pairs that touch a gap column are dropped); ``stems`` int32[S, 3] = (i, j, len) in columns of the sequence AS GIVEN, row
    q's from ``stem_off``[q] on (int64[rows + 1]); ``ref_scores`` float64[R, 3]: the known structure's scores, NaN without
    one.  ``source``: "device" or "host" -- where the rows were scored.  ``recomputed``: how many rows and known structures the
    device handed back to the host (beyond the exact range of its rounding; 0 for every record below 32,768 nt)."""

    _TENSORS = ("scores", "metrics", "status", "nstems", "npairs", "stems", "stem_off", "ref_scores", "row_off")

    def __init__(self, names, sequences, tables, source, recomputed=0):
        self.names, self.sequences, self.source, self.recomputed = names, sequences, source, recomputed
        for k in self._TENSORS:
            setattr(self, k, tables[k])

    def __len__(self):
        return len(self.names)

    def stems_of(self, q):
        """[(i, j, len)] of row q."""
        a, b = (int(x) for x in self.stem_off[q:q + 2])
        return [tuple(s) for s in self.stems[a:b].tolist()]


def _partner_rows(structures, nstruct, recs, on_device):
    """(partner, row_start, row_rec, row_off): the structures as ONE flat int32 array of partners (a torch tensor, on the GPU
    when on_device; a tensor that is there already is used where it is), where every row starts in it, the row's record, and
    the records' first rows."""
    import torch
    from .fold import FoldResult
    R = len(recs)
    lens = np.array([len(rec.seq) for rec in recs], np.int64)
    if isinstance(structures, FoldResult):
        if len(structures) != R or (structures._lengths != lens).any():
            raise ValueError("Score: the FoldResult's records are not the given records")
        count = 1 + structures._nstruct
        partner, first, stride = structures.partner, structures._cell_off[:-1], lens
    elif hasattr(structures, "shape") and len(structures.shape) == 3:
        if structures.shape[0] != R or (R and structures.shape[2] < lens.max()):
            raise ValueError("Score: structures of shape %s; [%d, K, Lmax] with Lmax >= %d is needed" % (tuple(structures.shape), R, lens.max()))
        K, Lmax = int(structures.shape[1]), int(structures.shape[2])
        count = np.full(R, K, np.int64) if nstruct is None else np.asarray(nstruct.cpu() if hasattr(nstruct, "cpu") else nstruct, np.int64)
        if count.shape != (R,) or (count < 0).any() or (count > K).any():
            raise ValueError("Score: nstruct must hold %d numbers between 0 and %d" % (R, K))
        partner = structures if hasattr(structures, "is_cuda") else torch.from_numpy(np.ascontiguousarray(structures))
        if partner.dtype != torch.int32:
            if partner.dtype not in (torch.int64, torch.int16):
                raise ValueError("Score: structures of dtype %s; int32 is needed" % partner.dtype)
            partner = partner.to(torch.int32)
        partner = partner.contiguous().view(-1)
        first, stride = np.arange(R, dtype=np.int64) * K * Lmax, np.full(R, Lmax, np.int64)
    else:
        if nstruct is not None:
            raise ValueError("Score: nstruct belongs to the padded form of structures")
        if len(structures) != R:
            raise ValueError("Score: structures for %d records, %d records" % (len(structures), R))
        count = np.array([len(s) for s in structures], np.int64)
        first, stride = np.zeros(R, np.int64), lens
        np.cumsum((count * lens)[:-1], out=first[1:])
        flat = np.full(int((count * lens).sum()), -1, np.int32)
        at = 0
        for r, (rec, rows) in enumerate(zip(recs, structures)):
            for k, dbn in enumerate(rows):
                if len(dbn) != lens[r]:
                    raise ValueError("Score: record %d (%s), row %d: a structure of %d columns for %d" % (r, rec.name, k, len(dbn), lens[r]))
                for v, w in DBNToPairs(dbn):
                    flat[at + v], flat[at + w] = w, v
                at += int(lens[r])
        partner = torch.from_numpy(flat)
    row_off = offsets(count)
    row_rec = np.repeat(np.arange(R, dtype=np.int32), count)
    k = np.arange(int(row_off[-1]), dtype=np.int64) - row_off[:-1][row_rec]
    row_start = np.asarray(first, np.int64)[row_rec] + k * stride[row_rec]
    if on_device and not partner.is_cuda:
        partner = partner.to(torch.device("cuda", torch.cuda.current_device()))
    elif not on_device and partner.is_cuda:
        partner = partner.cpu()
    return partner, row_start, row_rec, row_off


def Score(records=None, structures=None, inputfile=None, inputseq=None, inputformat="qtrf", fileformat="unknown", ignorewarn=False,
          M=1.8, B=-0.6, strict=True, nstruct=None):
    """Score the given structures of every record and return a :class:`ScoreResult`.

    The records come as for ``Fold``: ``records`` holds sequences or (name, sequence, reactivities, restraints, reference)
    tuples with None for what a record lacks, or ``inputfile`` / ``inputseq`` go through the input parser.  Restraints are
    ignored; reactivities are floats per column or an encoded string.

    ``structures``: a list per record of dot-bracket strings; or one int32 tensor or array ``[R, K, Lmax]`` of partners (the
    partner's column, -1 unpaired and as padding -- the shape of ``FoldResult.to_padded()``), of which record r's first
    ``nstruct[r]`` rows (default: K) are scored, a CUDA tensor where it is; or a ``FoldResult``: its 1 + nstruct[r] rows per
    record, the consensus first (without ``records``, its sequences are the records).  None: every record's known structure
    is its only row -- ``Predict(evalonly=True)`` as data.

    Coordinates are columns of the sequence as given.  Gap columns are removed first and a pair that touches one is dropped;
    stacking is decided on the gap-free sequence.  An invalid row -- a partner outside the record, p[p[i]] != i, p[i] == i, a
    pair on a separator, a record without a position to score -- raises ValueError under ``strict``; else its status is 1 and
    its scores and metrics are NaN.  Records longer than 32,768 nt raise ValueError."""
    import torch
    from .fold import FoldResult
    if records is None and inputfile is None and not inputseq and isinstance(structures, FoldResult):
        records = [(name, seq, None, None, None) for name, seq in zip(structures.names, structures.sequences)]
    if records is None:
        if inputfile is not None and not os.path.exists(inputfile) and os.path.exists(os.path.join(DATA_DIR, inputfile)):
            inputfile = os.path.join(DATA_DIR, inputfile)            # (as Fold: a name inside the package's data directory)
        assert inputseq or os.path.exists(str(inputfile)), "Input file does not exist."
        M, B = float(M), float(B)
    inputs = input_records(records, inputseq, inputfile, inputformat, fileformat, ignorewarn, None, M, B)
    recs = [ScoreRecord(rec[0], rec[1], rec[2], rec[4]) for rec in inputs]
    if structures is None:
        structures = [[rec[4]] if rec[4] else [] for rec in inputs]
    eng = _engine.get_engine()
    on_device = hasattr(eng, "score_tensors")
    partner, row_start, row_rec, row_off = _partner_rows(structures, nstruct, recs, on_device)
    recomputed = 0
    if on_device:
        tables = eng.score_tensors(recs, partner, row_start, row_rec)
        dev = tables["scores"].device
        status = tables["status"].cpu().numpy()
        redo_ref = np.flatnonzero(tables.pop("ref_status").cpu().numpy() == 2).tolist()
        recomputed = int((status == 2).sum()) + len(redo_ref)
        for q in np.flatnonzero(status == 2).tolist():               # beyond the exact range of the kernel's rounding
            rec, a = recs[row_rec[q]], int(row_start[q])
            st, sc, met, _, _ = score_row_host(rec, partner[a:a + len(rec.seq)].cpu().numpy())
            tables["status"][q] = st
            if sc is not None:
                tables["scores"][q] = torch.tensor(sc, dtype=torch.float64, device=dev)
            if met is not None:
                tables["metrics"][q] = torch.tensor(met, dtype=torch.float64, device=dev)
            status[q] = st
        for r in redo_ref:
            tables["ref_scores"][r] = torch.tensor(recs[r].score(recs[r].known), dtype=torch.float64, device=dev)
        tables["row_off"] = torch.from_numpy(row_off).to(dev)
    else:
        host = _score_host(recs, partner.numpy(), row_start, row_rec)
        status = host["status"]
        tables = {k: torch.from_numpy(v) for k, v in host.items()}
        tables["row_off"] = torch.from_numpy(row_off)
    if strict and status.any():
        q = int(np.flatnonzero(status)[0])
        r = int(row_rec[q])
        raise ValueError("Score: record %d (%s), row %d: not a valid structure of the record" % (r, recs[r].name, q - int(row_off[r])))
    return ScoreResult([rec[0] for rec in inputs], [rec[1] for rec in inputs], tables, "device" if on_device else "host", recomputed)
