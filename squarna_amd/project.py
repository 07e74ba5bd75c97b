"""``Project`` and ``Lift``: structures between the columns of an alignment and the residues of its rows.

The alignment entries (``FoldAlignment``, ``Covariation*``, ``RowIdentity``) work in alignment columns; the structure entries
(``Fold``, ``Score``, ``Elements``, ``Distances``, ``FoldMutants``) take ungapped sequences with partners in residue
coordinates.  ``Project`` takes structure lines over the L columns and gives, for every row, the line in that row's residue
coordinates -- gap columns removed, pairs that touch a gap opened: ``dbn.UnAlign`` of every row, as partners -- together with
the class of every pair in that row (which canonical type it holds there, two residues that do not pair, a gap in one or in
both columns) and the counts of the classes.  ``Lift`` goes back: structure lines over the residues of a row become partners
over the columns (``dbn.ReAlign``, as partners).  All numbers are integers.

With the GPU engine the rows go to the device once as bytes; one block per row keeps the row's gap map in LDS as 64-column
ballot words (``sq_project_rows``, ``sq_lift_rows``), and a tensor of partners that is on the device already is read where it
is.  An engine without the device methods (the tests' CPU engine, the sharded one) gets the same objects built with numpy
from ``np.cumsum`` of the residue mask and fancy indexing.  Neither entry prints anything.
"""
import numpy as np

from . import engine as _engine
from .covariation import TYPES, _classes, _device_engine, _open
from .dbn import DBNToPairs, GAPS, PairsToDBN
from .device_calls import PROJECT_COUNTS, PROJECT_MAX_COLS, PROJECT_MAX_ROWS
from .results import TensorResult
from .rows import offsets, row_pairs

_DEVICE_METHODS = ("project_rows", "lift_rows")
#: the class codes of ``ProjectResult.cls`` by name: 1..6 = ``Covariation.TYPES`` read as (letter at v, letter at w), 7 = two
#: residues that are not a canonical pair, 8 = a gap in exactly one of the two columns, 9 = a gap in both; 0 = no pair opens
CLASSES = ("none",) + TYPES + ("noncanonical", "one_gap", "both_gap")
_NONCANONICAL, _ONE_GAP, _BOTH_GAP = 7, 8, 9
#: the class of the pair (v, w) from the class bytes at v and w (covariation._classes: 0..3 = A C G U, 4 = a gap, 5 = other)
_PAIR_CLASS = np.full((6, 6), _NONCANONICAL, np.uint8)
_PAIR_CLASS[4, :] = _PAIR_CLASS[:, 4] = _ONE_GAP
_PAIR_CLASS[4, 4] = _BOTH_GAP
for _k, _t in enumerate(TYPES):
    _PAIR_CLASS["ACGU".index(_t[0]), "ACGU".index(_t[1])] = _k + 1
_INT_DTYPES = ("int16", "int32", "int64")


def _line_partners(line, width, who, what):
    """int32[width]: the partners of one dot-bracket line."""
    if len(line) != width:
        raise ValueError("{}: {} has {} characters for {}".format(who, what, len(line), width))
    row = np.full(width, -1, np.int32)
    for v, w in DBNToPairs(line):
        row[v], row[w] = w, v
    return row


def _int_tensor(t, who):
    """A tensor or array of partners as an int32 torch tensor (a CUDA int32 tensor: itself)."""
    import torch
    t = t if hasattr(t, "is_cuda") else torch.from_numpy(np.ascontiguousarray(t))
    if str(t.dtype).replace("torch.", "") not in _INT_DTYPES:
        raise ValueError("{}: structures of dtype {}; int16, int32 or int64 is needed".format(who, t.dtype))
    return t if t.dtype == torch.int32 else t.to(torch.int32)


def _bad_lines(P, width):
    """bool[...]: the partner rows P int[..., W] that are no valid structure of `width` columns (int or int[...]: only the
    first `width` entries of a row are read) under Distances' rule."""
    W = P.shape[-1]
    idx = np.arange(W)
    inside = idx < np.asarray(width)[..., None]
    inrange = (P >= -1) & (P < np.asarray(width)[..., None])
    back = np.take_along_axis(P, np.clip(P, 0, max(W - 1, 0)), -1) if W else P
    return (inside & (~inrange | (P == idx) | ((P >= 0) & inrange & (back != idx)))).any(-1)


def _gap_maps(rows):
    """(cls uint8[R, L], res bool[R, L], rank int64[R, L], length, col_of int32[R, Lmax], pos_of int32[R, L]) of the rows' bytes."""
    cls = _classes(rows)
    res = cls != 4
    rank = np.cumsum(res, 1) - 1                                     # the residue of a residue column
    length = res.sum(1).astype(np.int32)
    Lmax = int(max(length.max(initial=0), 1))
    pos_of = np.where(res, rank, -1).astype(np.int32)
    col_of = np.full((len(rows), Lmax), -1, np.int32)
    rr, cc = np.nonzero(res)
    col_of[rr, rank[rr, cc]] = cc
    return cls, res, rank, length, col_of, pos_of


def _host_project(rows, structs, shared, canonical_only, min_loop):
    """The tensors of a ProjectResult with numpy: the gap map from np.cumsum of the residue mask, the pairs by fancy indexing
    -- deliberately not the kernel's ballot-word form.  structs int[K, L] (shared) or int[R, K, L]."""
    R, L = rows.shape
    K = structs.shape[-2]
    cls, res, rank, length, col_of, pos_of = _gap_maps(rows)
    Lmax = col_of.shape[1]
    partner = np.full((R, K, Lmax), -1, np.int32)
    out_cls = np.zeros((R, K, L), np.uint8)
    counts = np.zeros((R, K, PROJECT_COUNTS), np.int32)
    status = np.zeros((R, K), np.int32)
    idx = np.arange(L)
    for k in range(K):
        P = (np.broadcast_to(structs[k], (R, L)) if shared else structs[:, k]).astype(np.int64)
        bad = _bad_lines(P, L)
        status[:, k] = bad
        rr, vv = np.nonzero((P > idx) & ~bad[:, None])               # every pair once, at its opening column
        ww = P[rr, vv]
        pc = _PAIR_CLASS[cls[rr, vv], cls[rr, ww]]
        out_cls[rr, k, vv] = pc
        admitted = (pc <= 6) | ((pc == _NONCANONICAL) & (not canonical_only))
        inner = rank[rr, ww] - rank[rr, vv] - 1                      # (read for admitted pairs only: both ends are residues)
        keep, drop = admitted & (inner >= min_loop), admitted & (inner < min_loop)
        partner[rr[keep], k, rank[rr[keep], vv[keep]]] = rank[rr[keep], ww[keep]]
        partner[rr[keep], k, rank[rr[keep], ww[keep]]] = rank[rr[keep], vv[keep]]
        counts[:, k, 0] = np.bincount(rr, minlength=R)
        for c in range(1, 10):
            counts[:, k, c] = np.bincount(rr[pc == c], minlength=R)
        counts[:, k, 10] = np.bincount(rr[drop], minlength=R)
        counts[:, k, 11] = np.bincount(rr[keep], minlength=R)
    return dict(length=length, col_of=col_of, pos_of=pos_of, partner=partner, cls=out_cls, counts=counts, status=status)


def _host_lift(rows, short, start, stride, nstruct, K):
    """The tensors of a LiftResult with numpy.  short: a flat int array; line k < nstruct[r] of row r starts at
    short[start[r] + k * stride[r]]."""
    R, L = rows.shape
    cls, res, rank, length, col_of, pos_of = _gap_maps(rows)
    partner = np.full((R, K, L), -1, np.int32)
    status = np.zeros((R, K), np.int32)
    for r in range(R):
        n, w, first, step = int(nstruct[r]), int(length[r]), int(start[r]), int(stride[r])
        if not n:
            continue
        if first < 0 or step < w or first + n * step > len(short):
            status[r, :n] = 2
            continue
        block = short[first:first + n * step].reshape(n, step)[:, :w].astype(np.int64)
        bad = _bad_lines(block, w)
        status[r, :n] = bad
        cols = col_of[r, :w]
        lifted = np.where(block >= 0, cols[np.clip(block, 0, max(w - 1, 0))] if w else block, -1)
        lifted[bad] = -1
        partner[r, :n, cols] = lifted.T                              # (an advanced index beside a slice: the columns lead)
    return dict(length=length, col_of=col_of, pos_of=pos_of, partner=partner, status=status, nstruct=np.asarray(nstruct, np.int32))


class _RowsResult(TensorResult):
    """What ProjectResult and LiftResult share: the rows and their gap maps."""

    def __len__(self):
        return self.R

    def sequence(self, r):
        """The ungapped string of row r."""
        return "".join(ch for ch in self.sequences[r] if ch not in GAPS)

    def records(self):
        """(names, ungapped sequences): the records ``Score`` and ``Fold`` take."""
        return list(self.names), [self.sequence(r) for r in range(self.R)]

    def to_padded(self):
        """``partner`` itself: the padded form ``Score``, ``Elements`` and ``Distances`` take."""
        return self.partner


class ProjectResult(_RowsResult):
    """What ``Project`` computes for R rows of L columns and K structure lines.

    Host attributes: ``names``, ``sequences`` (as given), ``R``, ``L``, ``K``, ``shared`` (the K lines are the same for all
    rows), ``source`` ("device" or "host": where the numbers were formed) and the keywords used (``canonical_only``,
    ``min_loop``, ``strict``).  Torch tensors on ``device``, Lmax = the most residues of a row (at least 1): ``length``
    int32[R], ``col_of`` int32[R, Lmax] (the column of residue i, -1 padding), ``pos_of`` int32[R, L] (the residue of column
    c, -1 at a gap), ``partner`` int32[R, K, Lmax] (the projected partners in residue coordinates, -1 unpaired and as
    padding), ``cls`` uint8[R, K, L] (at the opening column v of every pair (v, w), v < w, its class in that row:
    ``project.CLASSES``; 0 elsewhere), ``counts`` int32[R, K, 12] and ``status`` int32[R, K] (1: an invalid line; its partner
    is all -1, its cls and counts 0).

    ``counts``: [0] the pairs of the line, [1..9] the pairs per class, [10] the pairs of class 1..7 that ``min_loop`` alone
    drops, [11] the pairs kept.  So ``counts[0] == sum(counts[1..9])`` and ``counts[11] == sum(counts[1..6]) + (counts[7]
    unless canonical_only) - counts[10]``."""

    CLASSES = CLASSES
    _TENSORS = ("partner", "length", "col_of", "pos_of", "cls", "counts", "status")

    def __init__(self, names, sequences, shared, source, canonical_only, min_loop, strict, tensors):
        self.names, self.sequences, self.R, self.L = names, sequences, len(sequences), len(sequences[0])
        self.shared, self.source, self.canonical_only, self.min_loop, self.strict = shared, source, canonical_only, min_loop, strict
        for k in self._TENSORS:
            setattr(self, k, tensors[k])
        self.K = int(self.partner.shape[1])

    def dbn(self, r, k=0):
        """The dot-bracket line of line k projected onto row r."""
        n = int(self.length[r])
        return PairsToDBN(row_pairs(self.partner[r, k, :n].cpu().numpy()), n)

    def kept_fraction(self):
        """float64[R, K]: counts[11] / (counts[0] - counts[9]) -- of the pairs that do not lie in two gaps, the share kept --,
        1 where the denominator is 0."""
        import torch
        kept, den = self.counts[..., 11].double(), (self.counts[..., 0] - self.counts[..., 9]).double()
        return torch.where(den > 0, kept / den.clamp(min=1), torch.ones_like(den))

    def _shared_line(self, k, what):
        if not self.shared:
            raise ValueError("ProjectResult.{}: the structures are per row; a column count needs shared structures".format(what))
        if not 0 <= int(k) < self.K:
            raise IndexError("line %d of %d" % (k, self.K))
        return self.cls[:, int(k)]

    def support(self, k=0):
        """int64[L]: at every opening column of shared line k, the rows that hold a canonical pair there
        (``Covariation(pairs=line).bp_rows``)."""
        c = self._shared_line(k, "support")
        return ((c >= 1) & (c <= 6)).sum(0)

    def contradicting(self, k=0):
        """int64[L]: at every opening column of shared line k, the rows of class 7 or 8 there
        (``Covariation(pairs=line).incompatible``)."""
        c = self._shared_line(k, "contradicting")
        return ((c == _NONCANONICAL) | (c == _ONE_GAP)).sum(0)

    def worst_rows(self, k=0, n=5):
        """int64[<= n]: the rows with the lowest ``kept_fraction`` of line k, the lowest index first on ties."""
        import torch
        if not 0 <= int(k) < self.K:
            raise IndexError("line %d of %d" % (k, self.K))
        return torch.sort(self.kept_fraction()[:, int(k)], stable=True)[1][:max(int(n), 0)]


class LiftResult(_RowsResult):
    """What ``Lift`` computes for R rows of L columns with up to K structure lines each.

    Host attributes: ``names``, ``sequences`` (as given), ``R``, ``L``, ``K``, ``source`` and ``strict``.  Torch tensors on
    ``device``: ``partner`` int32[R, K, L] (the lines over the columns; -1 at gaps, unpaired, and on the lines beyond
    nstruct[r]), ``nstruct`` int32[R], ``length``, ``col_of``, ``pos_of`` as in :class:`ProjectResult`, ``status`` int32[R, K]
    (1: a line that is invalid against the row's residues; it is all -1)."""

    _TENSORS = ("partner", "nstruct", "length", "col_of", "pos_of", "status")

    def __init__(self, names, sequences, source, strict, tensors):
        self.names, self.sequences, self.R, self.L = names, sequences, len(sequences), len(sequences[0])
        self.source, self.strict = source, strict
        for k in self._TENSORS:
            setattr(self, k, tensors[k])
        self.K = int(self.partner.shape[1])

    def dbn(self, r, k=0):
        """The dot-bracket line over the columns of line k of row r."""
        return PairsToDBN(row_pairs(self.partner[r, k].cpu().numpy()), self.L)

    def pair_frequency(self, k=0):
        """float64[L, L] on the tensors' device, symmetric: the share of rows whose line k pairs columns v and w."""
        import torch
        if not 0 <= int(k) < self.K:
            raise IndexError("line %d of %d" % (k, self.K))
        P = self.partner[:, int(k)].long()
        v = torch.arange(self.L, dtype=torch.int64, device=P.device)[None, :].expand_as(P)
        opens = P > v
        flat = v[opens] * self.L + P[opens]
        c = torch.bincount(flat, minlength=self.L * self.L).view(self.L, self.L).double()
        # (divided by a tensor: by a Python number the device form multiplies with the reciprocal, which is not count / rows
        # in the last bit -- as AlignmentResult.pair_frequency)
        f = c / torch.full_like(c, self.R)
        return f + f.T


def _device_of(alignment, *tensors):
    """The device the rows go to: the alignment's, a given CUDA tensor's, else the current one."""
    import torch
    if alignment is not None and alignment.device.type == "cuda":
        return alignment.device
    for t in tensors:
        if hasattr(t, "is_cuda") and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _check_size(who, R, L):
    if R > PROJECT_MAX_ROWS or L > PROJECT_MAX_COLS:
        raise ValueError("{}: at most {} rows of {} columns on the device: {} x {}".format(who, PROJECT_MAX_ROWS, PROJECT_MAX_COLS, R, L))


def _column_structures(who, structures, step, alignment, R, L):
    """(the lines as an int32 torch tensor [K, L] or [R, K, L] wherever they are, shared) of Project's `structures`."""
    import torch
    from .fold_align import AlignmentResult
    if structures is None:
        structures = alignment
    if structures is None:
        raise ValueError("{}: structures is needed (or alignment=, whose step lines are then taken)".format(who))
    if isinstance(structures, AlignmentResult):
        if structures.L != L:
            raise ValueError("{}: the AlignmentResult has {} columns, the rows {}".format(who, structures.L, L))
        if step is None:
            return structures.steps, True
        if isinstance(step, bool) or step not in (1, 2, 3):
            raise ValueError("{}: step is None, 1, 2 or 3: {!r}".format(who, step))
        return structures.steps[step - 1:step], True
    if step is not None:
        raise ValueError("{}: step belongs to an AlignmentResult as structures".format(who))
    if isinstance(structures, str):
        return torch.from_numpy(_line_partners(structures, L, who, "the structure line")[None, :]), True
    if isinstance(structures, (list, tuple)):
        if structures and all(isinstance(s, str) for s in structures):
            return torch.from_numpy(np.stack([_line_partners(s, L, who, "line %d" % k) for k, s in enumerate(structures)])), True
        if len(structures) == R and all(isinstance(rows, (list, tuple)) and len(rows) and all(isinstance(s, str) for s in rows)
                                        for rows in structures):
            if len(set(len(rows) for rows in structures)) != 1:
                raise ValueError("{}: every row needs the same number of structure lines".format(who))
            return torch.from_numpy(np.stack([np.stack([_line_partners(s, L, who, "row %d, line %d" % (r, k)) for k, s in enumerate(rows)])
                                              for r, rows in enumerate(structures)])), False
    elif hasattr(structures, "shape") and 1 <= len(structures.shape) <= 3:
        t = _int_tensor(structures, who)
        shape = tuple(int(x) for x in t.shape)
        if shape[-1] != L or (len(shape) == 3 and shape[0] != R) or 0 in shape:
            raise ValueError("{}: structures of shape {}; [{L}], [K, {L}] or [{R}, K, {L}] is needed".format(who, shape, L=L, R=R))
        return (t if len(shape) > 1 else t[None, :]), len(shape) < 3
    raise ValueError("{}: structures is a dot-bracket line of the {} columns, a list of such lines, a list per row of such lines, an int "
                     "tensor [L], [K, L] or [R, K, L], or an AlignmentResult".format(who, L))


def Project(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None, alignment=None, structures=None,
            step=None, canonical_only=False, min_loop=0, strict=True, ignorewarn=False):
    """Structure lines over the columns of an alignment projected onto every row, returned as a :class:`ProjectResult`.

    Exactly one input, read as ``Covariation`` reads it: ``inputfile``, ``sequences`` (aligned strings, with ``names`` or
    numbered) or ``alignment`` (an :class:`AlignmentResult`: its sequences).  A byte is A, C, G, U (either case, T as U), a gap
    (``- . ~``) or "other"; a separator column is a column like any other, of class "other".

    ``structures``: partners over the L columns -- one dot-bracket line of L characters; a list of K such lines, shared by
    all rows; a list per row of K lines; an int16 / int32 / int64 tensor or array ``[L]``, ``[K, L]`` (shared) or ``[R, K, L]``
    (per row) with -1 for unpaired, a CUDA tensor where it is; or an ``AlignmentResult``: its ``steps`` (K = 3, shared), or
    with ``step=1|2|3`` that one line.  None with ``alignment=``: the alignment's steps.

    A pair (v, w) of a line is kept in row r's ``partner`` iff its class there is 1..6, or 7 unless ``canonical_only``, and
    at least ``min_loop`` residues of the row lie strictly between its ends.  With the defaults the result is
    ``dbn.UnAlign`` of every row.  ``counts``: [0] the pairs of the line, [1..9] the pairs per class, [10] the pairs of class
    1..7 that min_loop alone drops, [11] the pairs kept; counts[0] == sum(counts[1..9]) and counts[11] == sum(counts[1..6]) +
    (counts[7] unless canonical_only) - counts[10].  An invalid line -- a partner outside [-1, L), p[p[i]] != i, p[i] == i --
    raises ValueError under ``strict``; else its status is 1, its partner all -1, its cls and counts 0."""
    import torch
    who = "Project"
    names, seqs, _, _, rows = _open(who, inputfile, fileformat, inputformat, sequences, names, alignment, "scan", 0, 0, 0, ignorewarn)
    R, L = rows.shape
    if isinstance(min_loop, bool) or not isinstance(min_loop, (int, np.integer)) or min_loop < 0 or min_loop >= 2 ** 31:
        raise ValueError("{}: min_loop is an int >= 0: {!r}".format(who, min_loop))
    if canonical_only not in (True, False):
        raise ValueError("{}: canonical_only is True or False: {!r}".format(who, canonical_only))
    structs, shared = _column_structures(who, structures, step, alignment, R, L)
    eng = _engine.get_engine()
    on_device = _device_engine(eng, _DEVICE_METHODS)
    if on_device:
        _check_size(who, R, L)
        dev = _device_of(alignment, structs)
        Lmax = int(max((_classes(rows) != 4).sum(1).max(), 1))
        tensors = eng.project_rows(torch.from_numpy(rows.copy()).to(dev), structs.to(dev).contiguous(), shared, Lmax, bool(canonical_only),
                                   int(min_loop))
    else:
        host = _host_project(rows, structs.cpu().numpy(), shared, bool(canonical_only), int(min_loop))
        tensors = {k: torch.from_numpy(v) for k, v in host.items()}
    if strict and bool(tensors["status"].any()):
        r, k = tensors["status"].nonzero()[0].tolist()
        raise ValueError("{}: row {} ({}), line {}: not a valid structure".format(who, r, names[r], k))
    return ProjectResult(names, seqs, shared, "device" if on_device else "host", bool(canonical_only), int(min_loop), bool(strict), tensors)


def _residue_structures(who, structures, nstruct, names, length, on_device, dev):
    """(short, start, stride, nstruct, K) of Lift's `structures`: a flat int32 torch tensor of partners in residue
    coordinates (on `dev` when on_device, a tensor that is there already as it is; else in host memory) and, per row, where
    its lines start, their stride and their number."""
    import torch
    from .fold import FoldResult
    R, lens = len(length), length.astype(np.int64)
    if isinstance(structures, FoldResult):
        if nstruct is not None:
            raise ValueError("{}: nstruct belongs to the padded form of structures".format(who))
        if len(structures) != R or (structures._lengths != lens).any():
            raise ValueError("{}: the FoldResult's records are not the ungapped rows (their lengths differ)".format(who))
        short, start, stride, count = structures.partner, structures._cell_off[:-1], lens, 1 + structures._nstruct
    elif hasattr(structures, "shape") and len(structures.shape) == 3:
        short = _int_tensor(structures, who)
        if int(short.shape[0]) != R or int(short.shape[1]) < 1 or int(short.shape[2]) < max(int(lens.max()), 1):
            raise ValueError("{}: structures of shape {}; [{}, K, Lmax] with Lmax >= {} is needed".format(who, tuple(short.shape), R,
                                                                                                     max(int(lens.max()), 1)))
        K, width = int(short.shape[1]), int(short.shape[2])
        count = np.full(R, K, np.int64) if nstruct is None else np.asarray(nstruct.cpu() if hasattr(nstruct, "cpu") else nstruct, np.int64)
        if count.shape != (R,) or (count < 0).any() or (count > K).any():
            raise ValueError("{}: nstruct must hold {} numbers between 0 and {}".format(who, R, K))
        short, start, stride = short.contiguous().view(-1), np.arange(R, dtype=np.int64) * K * width, np.full(R, width, np.int64)
    elif isinstance(structures, (list, tuple)) and len(structures) == R and all(
            isinstance(rows, (list, tuple)) and all(isinstance(s, str) for s in rows) for rows in structures):
        if nstruct is not None:
            raise ValueError("{}: nstruct belongs to the padded form of structures".format(who))
        count = np.array([len(rows) for rows in structures], np.int64)
        start, stride = offsets(count * lens)[:-1], lens
        parts = [_line_partners(s, int(lens[r]), who, "row %d (%s), line %d" % (r, names[r], k))
                 for r, rows in enumerate(structures) for k, s in enumerate(rows)]
        short = torch.from_numpy(np.concatenate(parts + [np.zeros(0, np.int32)]))
    else:
        raise ValueError("{}: structures is a list per row of dot-bracket strings of the row's residues, an [R, K, Lmax] int tensor of "
                         "partners or a FoldResult of the ungapped rows".format(who))
    if not short.numel():
        short = torch.full((1,), -1, dtype=torch.int32, device=short.device)
    short = short.to(dev) if on_device else short.cpu()
    return short, np.asarray(start, np.int64), stride.astype(np.int32), count.astype(np.int32), int(max(count.max(initial=0), 1))


def Lift(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None, alignment=None, structures=None,
         nstruct=None, strict=True, ignorewarn=False):
    """Structure lines over the residues of the rows of an alignment put over its columns, returned as a :class:`LiftResult`.

    The rows: exactly one of ``inputfile``, ``sequences`` and ``alignment``, as for ``Project``.  ``structures``, in residue
    coordinates of the ungapped rows, in the forms ``Score`` takes: a list per row of dot-bracket strings, each of that row's
    residues; an int16 / int32 / int64 tensor or array ``[R, K, Lmax]`` of partners (-1 unpaired and as padding; a CUDA
    tensor where it is) of which row r's first ``nstruct[r]`` lines (default: K) are taken; or a ``FoldResult`` whose records
    are the R ungapped rows: its 1 + nstruct[r] rows, the consensus first (other lengths: ValueError).

    ``partner[r, k]`` is ``dbn.ReAlign`` of line k of row r, as partners: -1 at gap columns.  A line that is invalid against
    the row's residues -- a partner outside [-1, length), p[p[i]] != i, p[i] == i -- raises ValueError under ``strict``; else
    its status is 1 and it is all -1.  ``Project(structures=Lift(...).partner)`` with the defaults gives the lines back."""
    import torch
    who = "Lift"
    names, seqs, _, _, rows = _open(who, inputfile, fileformat, inputformat, sequences, names, alignment, "scan", 0, 0, 0, ignorewarn)
    R, L = rows.shape
    if structures is None:
        raise ValueError("{}: structures is needed".format(who))
    eng = _engine.get_engine()
    on_device = _device_engine(eng, _DEVICE_METHODS)
    length = (_classes(rows) != 4).sum(1)
    dev = None
    if on_device:
        _check_size(who, R, L)
        dev = _device_of(alignment, getattr(structures, "partner", structures))
    short, start, stride, count, K = _residue_structures(who, structures, nstruct, names, length, on_device, dev)
    if on_device:
        tensors = eng.lift_rows(torch.from_numpy(rows.copy()).to(dev), short, start, stride, count, K, int(max(length.max(), 1)))
    else:
        host = _host_lift(rows, short.numpy(), start, stride, count, K)
        tensors = {k: torch.from_numpy(v) for k, v in host.items()}
    if strict and bool(tensors["status"].any()):
        r, k = tensors["status"].nonzero()[0].tolist()
        raise ValueError("{}: row {} ({}), line {}: not a valid structure of the row's {} residues".format(who, r, names[r], k, int(length[r])))
    return LiftResult(names, seqs, "device" if on_device else "host", bool(strict), tensors)
