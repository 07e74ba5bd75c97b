"""``Covariation``: how the rows of an alignment support pairs of its columns.

``FoldAlignment`` states which columns pair and in how many rows.  ``Covariation`` states what the alignment itself says about
a pair of columns v < w: how many rows hold each of the six canonical pair types there (``AU UA GC CG GU UG``), how many hold
a gap in both columns, how many are incompatible with the pair, and ``cov`` -- the sum, over the unordered pairs of rows that
both hold a canonical pair, of the Hamming distance of their two pairs (the numerator of RNAalifold's covariance term).  A
pair with G-C in one row and A-U in another covaries; a pair that is G-C in every row is conserved and has cov 0.  All
numbers are integers.

With the GPU engine the rows go to the device once as bytes, are bit-sliced there, and either every cell is scanned
(``sq_covariation_scan``: AND + popcount on 64 rows at a time, the cells that pass the thresholds are emitted) or the given
pairs are looked up (``sq_covariation_pairs``); nothing of size rows x L or L^2 comes back, only the two status words.  An
engine without the device methods (the tests' CPU engine, the sharded one) gets the same object built with numpy from one-hot
matrices.  ``Covariation`` prints nothing.
"""
import contextlib
import io

import numpy as np

from . import engine as _engine
from .dbn import DBNToPairs, GAPS
from .inputs import ParseInput
from .options import check_input
from .results import TensorResult

_DEVICE_METHODS = ("covariation_scan", "covariation_pairs")
#: the six canonical pair types: columns 0..5 of ``CovariationResult.counts`` (column 6: the rows with a gap in both columns)
TYPES = ("AU", "UA", "GC", "CG", "GU", "UG")
#: d(t, t'): the Hamming distance of two pair types as two-letter strings
_D = np.array([[sum(x != y for x, y in zip(s, t)) for t in TYPES] for s in TYPES], np.int64)
_FIELDS = ("cov", "bp_rows", "both_gap", "incompatible", "types")


def _classes(rows):
    """uint8[R, L]: 0..3 = A C G U (either case, T as U), 4 = a gap, 5 = anything else; rows = uint8[R, L] of bytes."""
    lut = np.full(256, 5, np.uint8)
    for k, ch in enumerate("ACGU"):
        lut[ord(ch)] = lut[ord(ch.lower())] = k
    lut[ord("T")] = lut[ord("t")] = 3
    for g in GAPS:
        lut[ord(g)] = 4
    return lut[rows]


def _cov_of(c):
    """cov int64[...] of the type counts c int64[..., 6]."""
    return sum(c[..., s] * c[..., t] * int(_D[s, t]) for s in range(6) for t in range(s + 1, 6))


def _host_cells(cls):
    """(c int64[L, L, 7], cov int64[L, L]) of every pair of columns of the class bytes cls uint8[R, L] with numpy: per pair type
    one int64 matrix product of the two letters' one-hot matrices (deliberately not the kernel's bit-plane form)."""
    hot = [(cls == k).astype(np.int64) for k in range(5)]
    c = np.stack([hot["ACGU".index(t[0])].T @ hot["ACGU".index(t[1])] for t in TYPES] + [hot[4].T @ hot[4]], -1)
    return c, _cov_of(c)


def _host_scan(rows, minspan, min_rows, min_cov):
    """(pair_cols int32[P, 2] sorted by (v, w), counts int32[P, 7], cov int64[P]) with numpy (_host_cells)."""
    c, cov = _host_cells(_classes(rows))
    L = rows.shape[1]
    v, w = np.indices((L, L))
    keep = (w > v) & (w - v >= minspan) & (c[..., :6].sum(-1) >= min_rows) & (cov >= min_cov)
    at = np.nonzero(keep)                                            # (row-major: sorted by (v, w))
    return np.stack(at, 1).astype(np.int32), c[at].astype(np.int32), cov[at]


def _host_pairs(rows, pairs):
    """(counts int32[P, 7], cov int64[P]) of the given pairs with numpy."""
    cls = _classes(rows)
    a, b = cls[:, pairs[:, 0]], cls[:, pairs[:, 1]]                  # [R, P]
    c = np.stack([((a == "ACGU".index(t[0])) & (b == "ACGU".index(t[1]))).sum(0) for t in TYPES] + [((a == 4) & (b == 4)).sum(0)], -1)
    c = c.astype(np.int64).reshape(len(pairs), 7)
    return c.astype(np.int32), _cov_of(c).reshape(len(pairs))


class CovariationResult(TensorResult):
    """What ``Covariation`` computes for an alignment of R rows and L columns.

    Host attributes: ``names``, ``sequences`` (as given), ``R``, ``L``, ``mode`` ("scan": every cell that passed the
    thresholds; "pairs": the given pairs) and ``source`` ("device" or "host": where the numbers were formed).  Torch tensors on
    ``device``: ``pair_cols`` int32[P, 2] -- the column pairs (v, w), v < w, sorted by (v, w) in scan mode and in the given
    order otherwise --, ``counts`` int32[P, 7] -- the rows that hold each pair type of ``TYPES`` at (v, w) and, last, the rows
    with a gap in both columns --, ``cov`` int64[P].  Derived with torch ops: ``bp_rows`` (the rows that hold a canonical
    pair), ``both_gap``, ``incompatible`` (R - bp_rows - both_gap), ``types`` (the pair types that occur)."""

    TYPES = TYPES
    _TENSORS = ("cov", "pair_cols", "counts")

    def __init__(self, names, sequences, mode, source, pair_cols, counts, cov):
        self.names, self.sequences, self.R, self.L = names, sequences, len(sequences), len(sequences[0])
        self.mode, self.source = mode, source
        self.pair_cols, self.counts, self.cov = pair_cols, counts, cov

    def __len__(self):
        return int(self.cov.numel())

    @property
    def bp_rows(self):
        return self.counts[:, :6].sum(1, dtype=self.counts.dtype)

    @property
    def both_gap(self):
        return self.counts[:, 6]

    @property
    def incompatible(self):
        return self.R - self.bp_rows - self.both_gap

    @property
    def types(self):
        return (self.counts[:, :6] > 0).sum(1, dtype=self.counts.dtype)

    def covarying(self, min_types=2):
        """bool[P]: the pairs at which at least `min_types` pair types occur."""
        return self.types >= int(min_types)

    def score(self, phi=1.0):
        """float64[P]: cov / C(R, 2) - phi * incompatible / R, the first term 0 for a single row."""
        import torch
        cov, bad = self.cov.double(), self.incompatible.double()
        # (divided by tensors: by a Python number the device form multiplies with the reciprocal, which is not the quotient
        # in the last bit -- as AlignmentResult.pair_frequency)
        first = cov / torch.full_like(cov, self.R * (self.R - 1) // 2) if self.R > 1 else torch.zeros_like(cov)
        return first - torch.full_like(bad, float(phi)) * bad / torch.full_like(bad, self.R)

    def _field(self, field):
        if field in _FIELDS:
            return getattr(self, field)
        if field in TYPES:
            return self.counts[:, TYPES.index(field)]
        raise ValueError("CovariationResult: field is one of {} or a pair type of {}: {!r}".format(", ".join(_FIELDS), " ".join(TYPES), field))

    def to_matrix(self, field="cov"):
        """int64[L, L] on the tensors' device, symmetric: `field` ("cov", "bp_rows", "both_gap", "incompatible", "types" or a
        pair type such as "GC", counted at (v, w) with v < w) of every pair of the result, 0 elsewhere."""
        import torch
        val = self._field(field).long()
        out = torch.zeros((self.L, self.L), dtype=torch.int64, device=self.device)
        v, w = self.pair_cols[:, 0].long(), self.pair_cols[:, 1].long()
        out[v, w] = val
        out[w, v] = val
        return out

    def of(self, v, w):
        """The record of columns (v, w) (or (w, v)) as a dict of host ints: the pair types' counts by name, both_gap, bp_rows,
        incompatible, types and cov; KeyError when the result has no such pair."""
        v, w = (int(v), int(w)) if v < w else (int(w), int(v))
        at = ((self.pair_cols[:, 0] == v) & (self.pair_cols[:, 1] == w)).nonzero()
        if not at.numel():
            raise KeyError((v, w))
        k = int(at[0, 0])
        c = self.counts[k].tolist()
        rec = dict(zip(TYPES, c[:6]))
        rec.update(both_gap=c[6], bp_rows=sum(c[:6]), incompatible=self.R - sum(c), types=sum(x > 0 for x in c[:6]), cov=int(self.cov[k]))
        return rec


def _read_alignment(inputfile, fileformat, inputformat, ignorewarn):
    """(names, sequences) of an alignment file, parsed as FoldAlignment parses it."""
    inputfile = check_input(None, inputfile, None, fileformat)[0]
    with contextlib.redirect_stdout(io.StringIO()):                  # (the parser announces a guessed file format)
        objs = [obj for obj in ParseInput(None, inputfile, inputformat, fmt=fileformat, ignore=ignorewarn)[0]]
    assert objs, "No input records."
    return [obj[0] for obj in objs], [obj[1] for obj in objs]


def _pair_list(pairs, alignment, L, who="Covariation"):
    """None for a scan, else the pairs as an int32 array [P, 2] (or a torch tensor, taken as given)."""
    if pairs is None:
        pairs = "scan" if alignment is None else "steps"
    if isinstance(pairs, str):
        if pairs == "scan":
            return None
        if pairs in ("steps", "table"):
            if alignment is None:
                raise ValueError("{}: pairs={!r} needs alignment=".format(who, pairs))
            if pairs == "table":
                return alignment.pair_cols
            found = sorted(set(p for step in (1, 2, 3) for p in alignment.pairs(step)))
        elif len(pairs) == L:
            found = DBNToPairs(pairs)
        else:
            raise ValueError("{}: pairs is 'scan', 'steps', 'table', a dot-bracket line of the alignment's {} columns, a list "
                             "of (v, w) or an int tensor [P, 2]: {!r}".format(who, L, pairs))
        return np.array(found, np.int32).reshape(-1, 2)
    if hasattr(pairs, "dim"):                                        # a torch tensor
        if pairs.dim() != 2 or int(pairs.shape[1]) != 2 or pairs.is_floating_point():
            raise ValueError("{}: a pairs tensor is an int tensor [P, 2]".format(who))
        return pairs
    try:
        arr = np.array([tuple(p) for p in pairs]).reshape(-1, 2)
        assert arr.dtype.kind in "iu" or not arr.size
    except Exception:
        raise ValueError("{}: pairs must be a list of (v, w) pairs of 0-based integers".format(who))
    return arr.astype(np.int32)


def _open(who, inputfile, fileformat, inputformat, sequences, names, alignment, pairs, minspan, min_rows, min_cov, ignorewarn):
    """The opening of Covariation and CovariationSignificance (`who` names the entry in messages): the input choice, the
    thresholds and the pairs.  Returns (names, sequences, (minspan, min_rows, min_cov), the pairs as _pair_list gives them,
    the rows as bytes uint8[R, L])."""
    if sum(x is not None for x in (inputfile, sequences, alignment)) != 1:
        raise ValueError("{}: exactly one of inputfile, sequences and alignment is needed".format(who))
    if alignment is not None:
        names, seqs = list(alignment.names), list(alignment.sequences)
    elif inputfile is not None:
        names, seqs = _read_alignment(inputfile, fileformat, inputformat, ignorewarn)
    else:
        seqs = [str(s) for s in sequences]
        names = list(names) if names is not None else [">record%d" % (k + 1) for k in range(len(seqs))]
        if len(names) != len(seqs):
            raise ValueError("{}: {} names for {} sequences".format(who, len(names), len(seqs)))
    assert seqs and len(seqs[0]), "No input records."
    L = len(seqs[0])
    assert all(len(s) == L for s in seqs), 'The sequences are not aligned'
    try:
        minspan, min_rows, min_cov = int(minspan), int(min_rows), int(min_cov)
        assert min(minspan, min_rows, min_cov) >= 0
    except Exception:
        raise ValueError("{}: minspan, min_rows and min_cov are non-negative integers".format(who))
    given = _pair_list(pairs, alignment, L, who)
    # one byte per character; a character beyond latin-1 is no base and no gap ('?')
    rows = np.frombuffer("".join(seqs).encode("latin-1", "replace"), np.uint8).reshape(len(seqs), L)
    return names, seqs, (minspan, min_rows, min_cov), given, rows


def _device_engine(eng, methods):
    """Does the engine form the numbers on the device?  (The sharded engine and the tests' CPU engine do not.)"""
    return all(hasattr(eng, m) for m in methods) and not hasattr(eng, "reduce_matrix")


def _observe(who, eng, names, seqs, thresholds, given, rows, alignment):
    """(CovariationResult, the rows on the result's device or None when it was formed on the host) of an opening."""
    import torch
    minspan, min_rows, min_cov = thresholds
    L = rows.shape[1]
    on_device, d_rows = _device_engine(eng, _DEVICE_METHODS), None
    if on_device:
        if alignment is not None and alignment.device.type == "cuda":
            dev = alignment.device
        elif hasattr(given, "is_cuda") and given.is_cuda:
            dev = given.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
        d_rows = torch.from_numpy(rows.copy()).to(dev)
        if given is None:
            flat, counts, cov = eng.covariation_scan(d_rows, minspan, min_rows, min_cov)
            flat, order = torch.sort(flat)
            cols, counts, cov = torch.stack((flat // L, flat % L), 1).to(torch.int32), counts[order], cov[order]
        else:
            cols = (given if hasattr(given, "dim") else torch.from_numpy(given)).to(device=dev, dtype=torch.int32).contiguous()
            counts, cov = eng.covariation_pairs(d_rows, cols)
    elif given is None:
        cols, counts, cov = (torch.from_numpy(a) for a in _host_scan(rows, minspan, min_rows, min_cov))
    else:
        cols = (given.cpu() if hasattr(given, "dim") else torch.from_numpy(given)).to(torch.int32).contiguous()
        p = cols.numpy()
        if len(p) and not ((p[:, 0] >= 0) & (p[:, 0] < p[:, 1]) & (p[:, 1] < L)).all():
            raise RuntimeError("%s: a pair is not 0 <= v < w < %d columns" % (who, L))
        counts, cov = (torch.from_numpy(a) for a in _host_pairs(rows, p))
    res = CovariationResult(names, seqs, "scan" if given is None else "pairs", "device" if on_device else "host", cols, counts, cov)
    return res, d_rows


def Covariation(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None, alignment=None, pairs=None,
                minspan=4, min_rows=1, min_cov=1, ignorewarn=False):
    """Covariation evidence for pairs of columns of an alignment, returned as a :class:`CovariationResult`.

    Exactly one input: ``inputfile`` (parsed as ``FoldAlignment`` parses it), ``sequences`` (aligned strings, with ``names``
    or numbered) or ``alignment`` (an :class:`AlignmentResult`: its sequences).  Rows are read upper-cased with T as U; a
    byte is A, C, G, U, a gap (``- . ~``) or "other".

    ``pairs``: None or "scan" -- every cell v < w with ``w - v >= minspan`` whose rows hold at least ``min_rows`` canonical
    pairs and whose ``cov >= min_cov`` (the default without ``alignment``); "steps" -- the distinct pairs of the alignment's
    three step lines, sorted (the default with ``alignment``); "table" -- the alignment's ``pair_cols``; a dot-bracket line
    of L characters; a list of (v, w); an int tensor [P, 2].  Given pairs are taken as they are, in their order, whatever
    the thresholds; one that is not 0 <= v < w < L raises RuntimeError."""
    names, seqs, thresholds, given, rows = _open("Covariation", inputfile, fileformat, inputformat, sequences, names, alignment, pairs,
                                                 minspan, min_rows, min_cov, ignorewarn)
    return _observe("Covariation", _engine.get_engine(), names, seqs, thresholds, given, rows, alignment)[0]
