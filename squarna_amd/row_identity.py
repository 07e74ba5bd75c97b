"""``RowIdentity``: how alike the rows of an alignment are, how many rows lie near each row, and which rows a redundancy
filter keeps.

``Covariation`` and ``CovariationSignificance`` count every row of an alignment once.  Real alignments are redundant, and the
usual remedies compare rows with rows: the greedy filter at 97 % pairwise identity (Easel's, the one R-scape applies) and the
weights ``1 / (rows within 80 % identity)`` (RNAalifold, the DCA family).  ``RowIdentity`` gives both.  For rows a, b:
``same[a, b]`` = the columns where both hold the same base, ``both[a, b]`` = the columns where both hold a residue (any
non-gap), ``len[a] = both[a, a]``, ``bases[a] = same[a, a]``.  The identity is ``same / den`` with den the shorter row's
residues (``denominator="shorter"``, Easel's pairwise identity), ``both`` ("aligned") or L ("columns"), 0 when den is 0; rows
a != b are neighbours at T = round(threshold * 10000) basis points iff ``den > 0 and same * 10000 >= T * den``, in integers.
``neighbours[a]`` counts a and its neighbours; ``keep[a]`` is the greedy filter in row order: row 0 is kept, row a is kept iff
no kept row below it is its neighbour.  All numbers are integers.

With the GPU engine the rows go to the device once as bytes, are bit-sliced along the rows there and compared in tiles of
64 x 64 rows (``sq_row_identity``); the R x R matrices are written only when wanted, so that 20,000 rows cost the neighbour
bit matrix and four vectors.  An engine without the device method (the tests' CPU engine, the sharded one) gets the same
object built with numpy from one-hot matrix products.  ``RowIdentity`` prints nothing.
"""
import numpy as np

from . import engine as _engine
from .covariation import _classes, _device_engine, _open
from .device_calls import IDENTITY_DENOMINATORS, IDENTITY_MAX_COLS, IDENTITY_MAX_ROWS
from .results import TensorResult

_DEVICE_METHODS = ("row_identity",)
#: matrix=None materialises same / both up to this many rows
MATRIX_ROWS = 4096


def _host_counts(cls):
    """(same, both) int64[R, R] of the class bytes cls uint8[R, L] with numpy: one int64 matrix product per base of the rows'
    one-hot matrices, and one of the residue matrices (deliberately not the kernel's bit-plane form)."""
    same = sum(h @ h.T for h in ((cls == k).astype(np.int64) for k in range(4)))
    res = (cls != 4).astype(np.int64)
    return same, res @ res.T


def _den(denominator, same, both, length, L):
    """The denominators int64[R, R] (numpy arrays or torch tensors alike)."""
    if denominator == "shorter":
        return np.minimum(length[:, None], length[None, :]) if isinstance(length, np.ndarray) else length[:, None].minimum(length[None, :])
    return both if denominator == "aligned" else both * 0 + L


def _near(same, den, T):
    """The neighbour test of every cell, the diagonal included (numpy arrays or torch tensors alike)."""
    return (den > 0) & (same * 10000 >= T * den)


def _host_identity(rows, denominator, T, matrix):
    """The six arrays of a result with numpy; the filter is a plain loop over the rows."""
    same, both = _host_counts(_classes(rows))
    R, L = rows.shape
    length = np.diagonal(both).copy()
    near = _near(same, _den(denominator, same, both, length, L), T)
    near[np.arange(R), np.arange(R)] = False
    keep = np.zeros(R, bool)
    for a in range(R):
        keep[a] = not (near[a, :a] & keep[:a]).any()
    cast = lambda m: m.astype(np.int32)
    return dict(len=cast(length), bases=cast(np.diagonal(same)), neighbours=cast(1 + near.sum(1)), keep=keep,
                same=cast(same) if matrix else None, both=cast(both) if matrix else None)


class IdentityResult(TensorResult):
    """What ``RowIdentity`` computes for an alignment of R rows and L columns.

    Host attributes: ``names``, ``sequences`` (as given), ``R``, ``L``, ``threshold_bp`` (the threshold in basis points),
    ``denominator`` and ``source`` ("device" or "host": where the numbers were formed).  Torch tensors on ``device``: ``len``,
    ``bases``, ``neighbours`` int32[R], ``keep`` bool[R] and, when the matrices were asked for, ``same`` and ``both`` int32[R, R]
    (else None).  Derived with torch ops: ``weights``, ``neff``, ``kept``, ``identity``, ``neighbours_at``, ``nearest``,
    ``mean_identity``; ``filtered`` and ``identity_of`` give host values."""

    _TENSORS = ("len", "bases", "neighbours", "keep", "same", "both")

    def __init__(self, names, sequences, threshold_bp, denominator, source, tensors):
        self.names, self.sequences, self.R, self.L = names, sequences, len(sequences), len(sequences[0])
        self.threshold_bp, self.denominator, self.source = threshold_bp, denominator, source
        for k in self._TENSORS:
            setattr(self, k, tensors[k])

    def __len__(self):
        return self.R

    def _matrices(self, what):
        if self.same is None:
            raise ValueError("IdentityResult.%s needs the matrices: call RowIdentity with matrix=True" % what)
        return self.same.long(), self.both.long()

    def weights(self):
        """float64[R]: 1 / neighbours, the weight of a row among the rows within the threshold of it."""
        import torch
        n = self.neighbours.double()
        # (divided by a tensor: by a Python number the device form multiplies with the reciprocal -- CovariationResult.score)
        return torch.ones_like(n) / n

    def neff(self):
        """The effective number of rows: the sum of the weights, as a 0-dim float64 tensor."""
        return self.weights().sum()

    def kept(self):
        """int64[K]: the indices of the rows the greedy filter keeps, ascending."""
        return self.keep.nonzero().reshape(-1)

    def filtered(self):
        """(names, sequences) of the kept rows, as ``Covariation(sequences=, names=)`` and ``FoldAlignment`` take them."""
        at = self.kept().tolist()
        return [self.names[k] for k in at], [self.sequences[k] for k in at]

    def _denominators(self, same, both):
        return _den(self.denominator, same, both, self.len.long(), self.L)

    def identity(self):
        """float64[R, R]: same / den, 0 where den is 0 (the diagonal: bases / len under "shorter" and "aligned")."""
        import torch
        same, both = self._matrices("identity")
        den = self._denominators(same, both)
        return torch.where(den > 0, same.double() / den.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=same.device))

    def identity_of(self, a, b):
        """The record of rows a and b as a dict of host values: same, both, len_a, len_b, den, identity (a float, 0.0 when den
        is 0) and neighbours (bool: a != b and within the threshold)."""
        same, both = self._matrices("identity_of")
        a, b = int(a), int(b)
        s, bo, la, lb = int(same[a, b]), int(both[a, b]), int(self.len[a]), int(self.len[b])
        den = min(la, lb) if self.denominator == "shorter" else bo if self.denominator == "aligned" else self.L
        return dict(same=s, both=bo, len_a=la, len_b=lb, den=den, identity=s / den if den else 0.0,
                    neighbours=a != b and den > 0 and s * 10000 >= self.threshold_bp * den)

    def neighbours_at(self, threshold):
        """int32[R]: ``neighbours`` at another threshold, recomputed from the matrices with the integer test."""
        same, both = self._matrices("neighbours_at")
        near = _near(same, self._denominators(same, both), _basis_points(threshold, "IdentityResult.neighbours_at"))
        near.fill_diagonal_(False)
        return (1 + near.sum(1)).to(self.neighbours.dtype)

    def nearest(self):
        """(float64[R], int64[R]): per row the largest identity to another row and that row's index (the lowest such row;
        0.0 and -1 for a single row)."""
        import torch
        ident = self.identity()
        if self.R < 2:
            return torch.zeros(self.R, dtype=torch.float64, device=ident.device), torch.full((self.R,), -1, dtype=torch.int64, device=ident.device)
        ident.fill_diagonal_(-1.0)
        first = ident.argmax(1)                                      # (argmax gives the first of equal values; max(1) promises no such thing)
        return ident.gather(1, first[:, None]).reshape(-1), first

    def mean_identity(self):
        """The mean identity of the R (R - 1) / 2 pairs of different rows, as a 0-dim float64 tensor (0 for a single row)."""
        import torch
        ident = self.identity()
        if self.R < 2:
            return torch.zeros((), dtype=torch.float64, device=ident.device)
        total = torch.triu(ident, 1).sum()
        return total / torch.full_like(total, self.R * (self.R - 1) // 2)


def _basis_points(threshold, who):
    try:
        T = int(round(float(threshold) * 10000))
        assert 0 <= T <= 10000
    except Exception:
        raise ValueError("{}: threshold is a number from 0 to 1: {!r}".format(who, threshold))
    return T


def RowIdentity(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None, alignment=None, threshold=0.8,
                denominator="shorter", matrix=None, ignorewarn=False):
    """Row identities, neighbour counts and the greedy redundancy filter of an alignment, returned as an
    :class:`IdentityResult`.

    Exactly one input: ``inputfile`` (parsed as ``FoldAlignment`` parses it), ``sequences`` (aligned strings, with ``names``
    or numbered) or ``alignment`` (an :class:`AlignmentResult`: its sequences).  Rows are read as ``Covariation`` reads them.

    ``threshold``: rows at this identity or above are neighbours (0.8: the weights of RNAalifold and the DCA family; 0.97:
    R-scape's filter), taken as round(threshold * 10000) basis points.  ``denominator``: "shorter" (the residues of the
    shorter row), "aligned" (the columns where both rows hold a residue) or "columns" (L).  ``matrix``: whether the R x R
    tensors ``same`` and ``both`` are formed; None: up to 4096 rows."""
    who = "RowIdentity"
    names, seqs, _, _, rows = _open(who, inputfile, fileformat, inputformat, sequences, names, alignment, "scan", 0, 0, 0, ignorewarn)
    T = _basis_points(threshold, who)
    if denominator not in IDENTITY_DENOMINATORS:
        raise ValueError("{}: denominator is one of {}: {!r}".format(who, ", ".join(IDENTITY_DENOMINATORS), denominator))
    if matrix not in (None, True, False):
        raise ValueError("{}: matrix is None, True or False: {!r}".format(who, matrix))
    R, L = rows.shape
    matrix = R <= MATRIX_ROWS if matrix is None else bool(matrix)
    import torch
    eng = _engine.get_engine()
    on_device = _device_engine(eng, _DEVICE_METHODS)
    if on_device:
        if R > IDENTITY_MAX_ROWS or L > IDENTITY_MAX_COLS:
            raise ValueError("{}: at most {} rows of {} columns on the device: {} x {}".format(who, IDENTITY_MAX_ROWS, IDENTITY_MAX_COLS, R, L))
        dev = alignment.device if alignment is not None and alignment.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        tensors = eng.row_identity(torch.from_numpy(rows.copy()).to(dev), IDENTITY_DENOMINATORS.index(denominator), T, matrix)
    else:
        tensors = {k: None if v is None else torch.from_numpy(v) for k, v in _host_identity(rows, denominator, T, matrix).items()}
    return IdentityResult(names, seqs, T, denominator, "device" if on_device else "host", tensors)
