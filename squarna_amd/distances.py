"""``Distances``: how different structures are from each other, which of them are really distinct, and which structure each
one stands for.

Every ``Fold*`` entry returns many structures; ``Distances`` compares them with each other.  A structure row is a row of
partners p of ``width`` columns (p[i] = the partner of column i, or -1); its pair set is ``{(i, p[i]) : p[i] > i}`` in the
columns as given -- no sequence is read, and gap columns and separators are columns like any other.  For rows a, b of one
group: ``npairs[a]`` = the pairs of a, ``common[a, b]`` = the pairs both hold, and the base-pair distance is
``d(a, b) = npairs[a] + npairs[b] - 2 common[a, b]``.  Rows a != b of a group are neighbours iff ``d <= radius`` or, under
``relative=t`` with T = round(t * 10000) basis points, iff ``d * 10000 <= T * (npairs[a] + npairs[b])`` (that is 1 - F1 <= t;
two empty structures are neighbours), in integers.  ``neighbours[a]`` counts a and its neighbours; ``keep[a]`` is the greedy
filter in row order within the group -- the first row is kept, row a is kept iff no kept row below it is its neighbour: with
``Fold``'s rank order, the best-ranked structures that differ by more than the radius -- and ``leader[a]`` is a itself when
kept, else the lowest kept neighbour below it.  All numbers are integers.

With the GPU engine the rows are bit-sliced along the rows on the device (a plane of the opening columns and the planes of
the bits of the span p[i] - i) and compared in tiles of 64 x 64 rows (``sq_structure_distances``); a tensor of partners that
is on the device already is read where it is.  An engine without the device method (the tests' CPU engine, the sharded one)
gets the same object built with numpy from an incidence product over pair keys.  ``Distances`` prints nothing.
"""
import numpy as np

from . import engine as _engine
from .covariation import _device_engine
from .device_calls import DISTANCES_MAX_COLS, DISTANCES_MAX_ROWS, DISTANCES_TILE
from .results import TensorResult
from .rows import offsets
from .score import _partner_rows

_DEVICE_METHODS = ("structure_distances",)
#: matrix=None materialises common while the groups' cells sum to at most this many
MATRIX_CELLS = 1 << 24
GROUPS = ("record", "all")


class _Record:
    """What ``score._partner_rows`` reads of a record: a name and something with the record's number of columns."""
    __slots__ = ("name", "seq")

    def __init__(self, name, width):
        self.name, self.seq = name, range(int(width))


def plan_tiles(group_off):
    """int32[T, 2]: the upper-triangle tiles (ta, tb) of 64 x 64 rows, over the global row index, that hold a cell of one group
    -- ta == tb, or the last row of tile ta and the first row of tile tb lie in one group --, row after row
    (``SqDistances::plan_tiles``, csrc/sq_distances.h).  group_off [G + 1]: the groups' first rows, from 0 to S."""
    group_off = np.asarray(group_off, np.int64)
    S, TL = int(group_off[-1]), DISTANCES_TILE
    nT = (S + TL - 1) // TL
    ta = np.arange(nT, dtype=np.int64)
    last = ta * TL + TL - 1
    inside = last < S                                                # (else tile ta is the last one)
    group = np.searchsorted(group_off, np.minimum(last, max(S - 1, 0)), side="right") - 1
    reach = np.where(inside, (group_off[np.minimum(group + 1, len(group_off) - 1)] - 1) // TL, ta)   # the last tile of that row's group
    count = np.maximum(reach, ta) - ta + 1
    first = offsets(count)
    a = np.repeat(ta, count)
    b = a + np.arange(int(first[-1]), dtype=np.int64) - np.repeat(first[:-1], count)
    return np.stack((a, b), 1).astype(np.int32)


def _near(mode, threshold, na, nb, common):
    """The neighbour test of cells (numpy arrays or torch tensors alike, int64), the diagonal included."""
    d = na + nb - 2 * common
    return d <= threshold if mode == 0 else d * 10000 <= threshold * (na + nb)


def _row_pairs(row):
    """(status, i, j) of one partner row: its pairs i < j as int64 arrays; status 1 and no pairs for an invalid row."""
    row = np.asarray(row, np.int64)
    w = len(row)
    idx = np.flatnonzero(row != -1)
    p = row[idx]
    none = np.zeros(0, np.int64)
    if ((p < 0) | (p >= w) | (p == idx)).any() or (row[p] != idx).any():
        return 1, none, none
    up = p > idx
    return 0, idx[up], p[up]


def _host_distances(partner, row_start, row_width, group_off, mode, threshold, matrix):
    """The tensors of a result with numpy.  Every pair (i, j) is the key i * W + j; per group the rows' keys become the
    columns of a 0 / 1 incidence matrix whose product with its transpose is common (float32: a sum of at most 2^14 ones is
    exact there) -- deliberately not the kernels' bit-plane form.  The cells are int32 (a distance is at most 2^15, so the
    products of the relative test stay below 2^29).  The filter is a plain loop over the rows."""
    S, G = len(row_start), len(group_off) - 1
    W = int(max(row_width.max(initial=0), 1))
    status, npairs, keys = np.zeros(S, np.int32), np.zeros(S, np.int32), []
    for q in range(S):
        status[q], i, j = _row_pairs(partner[row_start[q]:row_start[q] + row_width[q]])
        keys.append(i * W + j)
        npairs[q] = len(i)
    n = np.diff(group_off)
    mat_off = offsets(n * n)
    neighbours, leader, keep = np.zeros(S, np.int32), np.full(S, -1, np.int32), np.zeros(S, bool)
    common = np.zeros(int(mat_off[-1]), np.int32) if matrix else None
    for g in range(G):
        first, ng = int(group_off[g]), int(n[g])
        if not ng:
            continue
        mine = keys[first:first + ng]
        uniq, col = np.unique(np.concatenate(mine), return_inverse=True)
        inc = np.zeros((ng, max(len(uniq), 1)), np.float32)
        inc[np.repeat(np.arange(ng), [len(k) for k in mine]), col] = 1
        c = np.rint(inc @ inc.T).astype(np.int32)
        na = npairs[first:first + ng]
        valid = status[first:first + ng] == 0
        near = _near(mode, threshold, na[:, None], na[None, :], c) & valid[:, None] & valid[None, :]
        near[np.arange(ng), np.arange(ng)] = False
        neighbours[first:first + ng] = np.where(valid, 1 + near.sum(1), 0)
        kept = np.zeros(ng, bool)
        for a in np.flatnonzero(valid).tolist():
            hits = np.flatnonzero(near[a, :a] & kept[:a])
            kept[a] = not len(hits)
            leader[first + a] = first + (a if kept[a] else int(hits[0]))
        keep[first:first + ng] = kept
        if matrix:
            common[mat_off[g]:mat_off[g + 1]] = c.reshape(-1)
    return dict(status=status, npairs=npairs, neighbours=neighbours, leader=leader, keep=keep, common=common)


def _segment_sums(values, off):
    """int64[n]: the sums of values[off[k] : off[k + 1]] (torch; off ascends)."""
    import torch
    run = torch.cat((torch.zeros(1, dtype=torch.int64, device=values.device), torch.cumsum(values.long(), 0)))
    return run[off[1:]] - run[off[:-1]]


class DistancesResult(TensorResult):
    """What ``Distances`` computes for S structure rows in G groups.

    Host attributes: ``names`` (the records'), ``S``, ``G``, ``groups`` ("record" or "all"), ``radius`` and ``relative_bp``
    (the one in force, the other None) and ``source`` ("device" or "host": where the numbers were formed).  Torch tensors on
    ``device``: ``row_off`` int64[G + 1] -- group g has the rows row_off[g] .. row_off[g + 1] - 1; row indices are global
    everywhere --, ``mat_off`` int64[G + 1] -- the cell (a, b) of group g of n rows is ``common[mat_off[g] + (a - first) * n +
    (b - first)]`` --, ``status`` (1: an invalid row), ``npairs``, ``neighbours``, ``leader`` int32[S], ``keep`` bool[S] and,
    when the matrix was asked for, ``common`` int32, flat (else None).  Derived with torch ops on the result's device:
    ``common_of``, ``distance``, ``f1``, ``nearest``, ``mean_distance``, ``medoid``, ``neighbours_at``, ``kept``, ``clusters``;
    ``distance_of`` gives host values."""

    _TENSORS = ("status", "npairs", "neighbours", "leader", "keep", "common", "row_off", "mat_off")

    def __init__(self, names, groups, radius, relative_bp, source, tensors):
        self.names, self.groups, self.radius, self.relative_bp, self.source = names, groups, radius, relative_bp, source
        for k in self._TENSORS:
            setattr(self, k, tensors[k])
        self.S, self.G = int(self.status.numel()), int(self.row_off.numel()) - 1
        self._off = tensors["row_off"].tolist()                      # (host copies of the offsets: G + 1 numbers each)
        self._moff = tensors["mat_off"].tolist()

    def __len__(self):
        return self.S

    def _matrix(self, what):
        if self.common is None:
            raise ValueError("DistancesResult.%s needs the matrix: call Distances with matrix=True" % what)
        return self.common

    def rows_of(self, g):
        """(first, n): the first row of group g and its number of rows."""
        return self._off[g], self._off[g + 1] - self._off[g]

    def group_of(self, a):
        """The group of row a."""
        if not 0 <= int(a) < self.S:
            raise IndexError("row %d of %d" % (a, self.S))
        return int(np.searchsorted(np.asarray(self._off), int(a), side="right")) - 1

    def common_of(self, g):
        """int64[n, n]: the pairs every two rows of group g share."""
        first, n = self.rows_of(g)
        return self._matrix("common_of")[self._moff[g]:self._moff[g + 1]].view(n, n).long()

    def distance(self, g):
        """int64[n, n]: the base-pair distances of group g."""
        self._matrix("distance")
        c = self.common_of(g)
        first, n = self.rows_of(g)
        na = self.npairs[first:first + n].long()
        return na[:, None] + na[None, :] - 2 * c

    def f1(self, g):
        """float64[n, n]: 2 common / (npairs[a] + npairs[b]), 1 for two empty structures."""
        import torch
        self._matrix("f1")
        c = self.common_of(g)
        first, n = self.rows_of(g)
        na = self.npairs[first:first + n].long()
        total = na[:, None] + na[None, :]
        return torch.where(total > 0, (2 * c).double() / total.clamp(min=1).double(), torch.ones((), dtype=torch.float64, device=c.device))

    def distance_of(self, a, b):
        """The record of rows a and b of one group as a dict of host values: common, npairs_a, npairs_b, distance, f1 (a
        float, 1.0 for two empty structures) and neighbours (bool, under the result's threshold)."""
        self._matrix("distance_of")
        a, b, g = int(a), int(b), self.group_of(a)
        if self.group_of(b) != g:
            raise ValueError("DistancesResult.distance_of: rows %d and %d are not of one group" % (a, b))
        first, n = self.rows_of(g)
        c = int(self.common[self._moff[g] + (a - first) * n + (b - first)])
        na, nb = int(self.npairs[a]), int(self.npairs[b])
        mode, threshold = (0, self.radius) if self.relative_bp is None else (1, self.relative_bp)
        valid = not int(self.status[a]) and not int(self.status[b])
        return dict(common=c, npairs_a=na, npairs_b=nb, distance=na + nb - 2 * c, f1=2 * c / (na + nb) if na + nb else 1.0,
                    neighbours=bool(a != b and valid and _near(mode, threshold, na, nb, c)))

    def nearest(self, g):
        """(int64[n], int64[n]): per row of group g the smallest distance to another row of the group and that row's global
        index (the lowest such row; 0 and -1 for a single row)."""
        import torch
        d = self.distance(g)
        first, n = self.rows_of(g)
        if n < 2:
            return torch.zeros(n, dtype=torch.int64, device=d.device), torch.full((n,), -1, dtype=torch.int64, device=d.device)
        key = d * n + torch.arange(n, dtype=torch.int64, device=d.device)[None, :]    # (the lowest index wins a tie whatever min does)
        key.fill_diagonal_(torch.iinfo(torch.int64).max)
        best = key.min(1).values
        return best // n, best % n + first

    def _cell_rows(self):
        """int64[S + 1]: where the cells of every row start in the flat matrix."""
        import torch
        n = self.row_off[1:] - self.row_off[:-1]
        group = torch.repeat_interleave(torch.arange(self.G, dtype=torch.int64, device=n.device), n, output_size=self.S)
        rows = torch.arange(self.S, dtype=torch.int64, device=n.device)
        start = self.mat_off[:-1][group] + (rows - self.row_off[:-1][group]) * n[group]
        return torch.cat((start, self.mat_off[-1:])), group, n

    def mean_distance(self):
        """float64[G]: the mean distance of the n (n - 1) / 2 pairs of different rows of every group (0 below two rows)."""
        import torch
        common = self._matrix("mean_distance")
        n = self.row_off[1:] - self.row_off[:-1]
        # the ordered pairs of a group sum to 2 n sum(npairs) - 2 sum(common); the diagonal adds nothing to it
        total = n * _segment_sums(self.npairs, self.row_off) - _segment_sums(common, self.mat_off)
        pairs = n * (n - 1) // 2
        return torch.where(pairs > 0, total.double() / pairs.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=n.device))

    def medoid(self):
        """int64[G]: per group the valid row with the smallest sum of distances to the group's rows, the lowest such row
        (a global index); -1 for a group without a valid row.  (An invalid row has no pair: in the sums of the others it
        counts as an empty structure.)"""
        import torch
        common = self._matrix("medoid")
        cell_rows, group, n = self._cell_rows()
        na = self.npairs.long()
        total = n[group] * na + _segment_sums(na, self.row_off)[group] - 2 * _segment_sums(common, cell_rows)
        rows = torch.arange(self.S, dtype=torch.int64, device=na.device)
        none = torch.iinfo(torch.int64).max
        key = torch.where(self.status == 0, total * (self.S + 1) + rows, torch.full_like(total, none))
        best = torch.full((self.G,), none, dtype=torch.int64, device=na.device).scatter_reduce(0, group, key, "amin")
        return torch.where(best == none, torch.full_like(best, -1), best % (self.S + 1))

    def neighbours_at(self, radius=None, relative=None):
        """int32[S]: ``neighbours`` at another threshold, recomputed from the matrix with the integer test."""
        import torch
        common = self._matrix("neighbours_at").long()
        mode, threshold = _threshold(radius, relative, "DistancesResult.neighbours_at")
        cell_rows, group, n = self._cell_rows()
        a = torch.repeat_interleave(torch.arange(self.S, dtype=torch.int64, device=common.device), n[group], output_size=int(common.numel()))
        b = torch.arange(int(common.numel()), dtype=torch.int64, device=common.device) - cell_rows[:-1][a] + self.row_off[:-1][group][a]
        na, valid = self.npairs.long(), self.status == 0
        near = _near(mode, threshold, na[a], na[b], common) & (a != b) & valid[a] & valid[b]
        return torch.where(valid, 1 + _segment_sums(near, cell_rows), torch.zeros((), dtype=torch.int64, device=common.device)).to(self.neighbours.dtype)

    def kept(self):
        """int64[K]: the global indices of the rows the greedy filter keeps, ascending."""
        return self.keep.nonzero().reshape(-1)

    def clusters(self):
        """(int64[K], int64[K]): the kept rows and how many rows each of them leads, itself included."""
        import torch
        leaders = self.kept()
        led = self.leader[self.leader >= 0].long()
        return leaders, torch.bincount(led, minlength=max(self.S, 1))[leaders]


def _threshold(radius, relative, who):
    """(mode, threshold) of the two keywords: (0, k) under radius=k, (1, T basis points) under relative=t; radius 0 by default."""
    if radius is not None and relative is not None:
        raise ValueError("{}: give radius or relative, not both".format(who))
    if relative is not None:
        try:
            T = int(round(float(relative) * 10000))
            assert 0 <= T <= 10000 and not isinstance(relative, bool)
        except Exception:
            raise ValueError("{}: relative is a number from 0 to 1: {!r}".format(who, relative))
        return 1, T
    if radius is None:
        return 0, 0
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius < 0 or radius >= 2 ** 31:
        raise ValueError("{}: radius is an int >= 0: {!r}".format(who, radius))
    return 0, int(radius)


def Distances(structures, nstruct=None, names=None, groups="record", radius=None, relative=None, matrix=None, strict=True):
    """Base-pair distances, neighbour counts and the greedy filter of given structures, returned as a
    :class:`DistancesResult`.

    ``structures`` comes in the forms ``Score`` takes: a list per record of dot-bracket strings, all of one width within a
    record; or one int16 / int32 / int64 tensor or array ``[R, K, Lmax]`` of partners (-1 unpaired and as padding) of which
    record r's first ``nstruct[r]`` rows (default: K) are taken with width Lmax, a CUDA tensor where it is; or a
    ``FoldResult``: its 1 + nstruct[r] rows per record, the consensus first.  ``names``: the records' names (a FoldResult's
    own, else numbered).

    ``groups``: rows are compared within a group only -- "record": the rows of one record; "all": all rows are one group
    (widths may differ: the columns beyond a row's width are unpaired).  ``radius=k`` (an int >= 0; the default is 0:
    identical structures) or ``relative=t`` (0..1) sets the neighbour test.  ``matrix``: whether ``common`` is formed; None:
    while the groups' cells sum to at most 2^24.  An invalid row -- a partner outside [-1, width), p[p[i]] != i, p[i] == i --
    raises ValueError under ``strict``; else its status is 1, it has no pair, is nobody's neighbour, and has neighbours 0,
    keep False, leader -1."""
    import torch
    from .fold import FoldResult
    who = "Distances"
    mode, threshold = _threshold(radius, relative, who)
    if groups not in GROUPS:
        raise ValueError("{}: groups is one of {}: {!r}".format(who, ", ".join(GROUPS), groups))
    if matrix not in (None, True, False):
        raise ValueError("{}: matrix is None, True or False: {!r}".format(who, matrix))
    if isinstance(structures, FoldResult):
        widths, own = structures._lengths.tolist(), list(structures.names)
    elif hasattr(structures, "shape") and len(structures.shape) == 3:
        widths, own = [int(structures.shape[2])] * int(structures.shape[0]), None
    elif isinstance(structures, (list, tuple)) and all(isinstance(rows, (list, tuple)) and all(isinstance(s, str) for s in rows) for rows in structures):
        widths, own = [len(rows[0]) if len(rows) else 0 for rows in structures], None
    else:
        raise ValueError("{}: structures is a list per record of dot-bracket strings, an [R, K, Lmax] tensor of partners or a FoldResult".format(who))
    R = len(widths)
    if names is None:
        names = own if own is not None else [">record%d" % (k + 1) for k in range(R)]
    if len(names) != R:
        raise ValueError("{}: {} names for {} records".format(who, len(names), R))
    names = list(names)
    recs = [_Record(name, w) for name, w in zip(names, widths)]
    eng = _engine.get_engine()
    on_device = _device_engine(eng, _DEVICE_METHODS)
    try:
        partner, row_start, row_rec, row_off = _partner_rows(structures, nstruct, recs, on_device)
    except ValueError as err:
        raise ValueError(str(err).replace("Score:", who + ":", 1))
    S = len(row_rec)
    row_width = np.asarray(widths, np.int32).reshape(-1)[row_rec]
    group_off = np.asarray(row_off, np.int64) if groups == "record" else np.array([0, S], np.int64)
    n = np.diff(group_off)
    mat_off = offsets(n * n)
    matrix = int(mat_off[-1]) <= MATRIX_CELLS if matrix is None else bool(matrix)
    if S == 0:
        on_device = on_device and partner.is_cuda
        empty = lambda dt: torch.zeros(0, dtype=dt, device=partner.device)
        tensors = dict(status=empty(torch.int32), npairs=empty(torch.int32), neighbours=empty(torch.int32), leader=empty(torch.int32),
                       keep=empty(torch.bool), common=empty(torch.int32) if matrix else None)
    elif on_device:
        if S > DISTANCES_MAX_ROWS or int(row_width.max()) > DISTANCES_MAX_COLS:
            raise ValueError("{}: at most {} rows of {} columns on the device: {} x {}".format(who, DISTANCES_MAX_ROWS, DISTANCES_MAX_COLS, S,
                                                                                            int(row_width.max())))
        if int(row_width.max()) < 1:
            raise ValueError("{}: no row has a column".format(who))
        tensors = eng.structure_distances(partner, row_start, row_width, group_off.astype(np.int32), plan_tiles(group_off), mode, threshold, matrix)
    else:
        host = _host_distances(partner.numpy(), row_start, row_width, group_off, mode, threshold, matrix)
        tensors = {k: None if v is None else torch.from_numpy(v) for k, v in host.items()}
    dev = tensors["status"].device
    tensors["row_off"], tensors["mat_off"] = torch.from_numpy(group_off).to(dev), torch.from_numpy(mat_off).to(dev)
    if strict and S and bool(tensors["status"].any()):
        q = int(tensors["status"].nonzero()[0])
        r = int(row_rec[q])
        raise ValueError("{}: record {} ({}), row {}: not a valid structure".format(who, r, names[r], q - int(row_off[r])))
    return DistancesResult(names, groups, threshold if mode == 0 else None, threshold if mode == 1 else None,
                           "device" if on_device else "host", tensors)
