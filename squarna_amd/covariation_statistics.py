"""``CovariationStatistics``: mutual information, the G-test and chi-square of pairs of alignment columns, with APC or ASC.

``Covariation`` counts the six canonical pair types of two columns.  ``CovariationStatistics`` states the numbers people judge
a predicted pair by: for columns v < w the full joint table ``n[a * 4 + b]`` (a, b in ``A C G U``) of the rows with residue a
at v and residue b at w -- a row with a gap or any other byte at either column takes part in nothing --, a raw statistic S of
that table and its background-corrected form C.  With N the sum of n and na, nb its marginals:

  ``mi``   the sum over n > 0 of (n / N) * ln(n * N / (na * nb)), in nats
  ``gt``   2 * the sum over n > 0 of n * ln(n * N / (na * nb))                         (the G-test)
  ``chi``  the sum over na * nb > 0 of (n - e)^2 / e, e = na * nb / N

(S = 0 when N = 0.)  The corrections use the means of S over every pair of distinct columns, whatever ``minspan`` and the
thresholds: ``mean[c]`` = the mean of S(c, c') over c' != c, ``mean_all`` = the mean of S over v < w.  ``apc``:
C = S - mean[v] * mean[w] / mean_all (S when mean_all is 0); ``asc``: C = S - (mean[v] + mean[w] - mean_all); None: C = S.
``statistic="gt", correction="apc"`` is R-scape's default "GTp".

With the GPU engine the rows go to the device once as bytes and are bit-sliced there (the planes of ``Covariation``); a first
pass forms S of every cell for the column means, a second forms it again with C and emits the cells that pass the thresholds
(``sq_covariation_stat_scan``), or the given pairs are looked up (``sq_covariation_stat_pairs``).  No L x L matrix is stored
and the sums have a fixed order: two calls give the same bits.  An engine without the device methods (the tests' CPU engine,
the sharded one) gets the same object built with numpy from one-hot matrix products.  ``CovariationStatistics`` prints nothing.

``weights=`` gives every row a weight (``RowIdentity(...).weights()``: near-duplicate rows share one vote).  A weight is
quantised once to a multiple of 2^-20, q = round(w * 2^20); the joint table is then the sum of q over a cell's rows, an
integer, and n, na, nb and N above are those sums divided by 2^20, exact doubles (``csrc/sq_covar_wstat.h``;
``sq_covariation_wstat_scan`` / ``sq_covariation_wstat_pairs`` on the device).  The sums do not depend on the order of the
rows, two calls give the same bits, and integer weights give the bits of the unweighted call on the repeated rows.
"""
import math

import numpy as np

from . import engine as _engine
from .covariation import TYPES, _classes, _device_engine, _open
from .results import TensorResult

_DEVICE_METHODS = ("covariation_stat_scan", "covariation_stat_pairs")
_DEVICE_METHODS_W = ("covariation_wstat_scan", "covariation_wstat_pairs")
#: the fixed point of the row weights, the largest weight and the most weighted rows (csrc/sq_covar_wstat.h)
WEIGHT_ONE = 1 << 20
MAX_WEIGHT = 2048.0
MAX_WEIGHTED_ROWS = 1 << 22
STATISTICS = ("mi", "gt", "chi")
CORRECTIONS = (None, "apc", "asc")
#: the residues of the joint table's two axes: ``joint[:, a * 4 + b]`` counts LETTERS[a] at v with LETTERS[b] at w
LETTERS = "ACGU"
#: the joint table's cells by name, in its order
CELLS = tuple(a + b for a in LETTERS for b in LETTERS)
#: where the six canonical pair types of ``Covariation.TYPES`` lie in the joint table
_CANONICAL = [CELLS.index(t) for t in TYPES]
_FIELDS = ("value", "raw", "rows")
#: With min_stat=None nearly every cell in scope is a record (88 bytes each).  Up to this many cells in scope (92 MB of
#: result buffers) the device scan makes room for all of them and runs once; beyond it the first scan has the entry's default
#: room (1 << 16 records) and only counts, and the second allocates the true number: two scans, no buffer that is not needed.
_SCAN_CAP = 1 << 20


def _host_tables(cls):
    """int64[L, L, 16]: the joint table of every pair of columns of the class bytes cls uint8[R, L] with numpy: per cell of
    the table one int64 matrix product of the two letters' one-hot matrices (deliberately not the kernel's bit-plane form)."""
    hot = [(cls == k).astype(np.int64) for k in range(4)]
    return np.stack([hot[a].T @ hot[b] for a in range(4) for b in range(4)], -1)


def _host_raw(n, statistic):
    """S float64[...] of the joint tables n int64[..., 16], the terms added in the table's order."""
    N = n.sum(-1)
    sq = n.reshape(n.shape[:-1] + (4, 4))
    margins = (sq.sum(-1)[..., :, None] * sq.sum(-2)[..., None, :]).reshape(n.shape)
    S = np.zeros(n.shape[:-1], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(16):
            nk, mk = n[..., k], margins[..., k]
            if statistic == "chi":
                e = mk / N
                S = S + np.where(mk > 0, (nk - e) * (nk - e) / e, 0.0)
            else:
                weight = nk / N if statistic == "mi" else nk.astype(np.float64)
                S = S + np.where(nk > 0, weight * np.log((nk * N) / mk), 0.0)
    S = np.where(N > 0, S, 0.0)
    return 2.0 * S if statistic == "gt" else S


def _host_means(S):
    """(mean float64[L], mean_all) of the raw statistic of every pair of columns, S float64[L, L] (its upper triangle is read)."""
    L = S.shape[0]
    if L < 2:
        return np.zeros(L, np.float64), 0.0
    upper = np.triu(S, 1)
    return (upper + upper.T).sum(1) / (L - 1), float(upper.sum() / (L * (L - 1) // 2))


def _host_corrected(S, mean_v, mean_w, mean_all, correction):
    if correction == "apc":
        return S - mean_v * mean_w / mean_all if mean_all != 0 else S.copy()
    if correction == "asc":
        return S - (mean_v + mean_w - mean_all)
    return S.copy()


def _host_statistics(rows, given, statistic, correction, minspan, min_rows, min_stat):
    """(pair_cols int32[P, 2], joint int32[P, 16], raw, value float64[P], col_mean float64[L] or None, mean_all or None) with
    numpy: every cell for a scan (given None, sorted by (v, w)) and for the means, the given pairs otherwise."""
    L = rows.shape[1]
    n = _host_tables(_classes(rows))
    S = _host_raw(n, statistic)
    mean, mean_all = _host_means(S) if correction is not None else (np.zeros(L), 0.0)
    C = _host_corrected(S, mean[:, None], mean[None, :], mean_all, correction)
    if given is None:
        v, w = np.indices((L, L))
        keep = (w > v) & (w - v >= minspan) & (n.sum(-1) >= min_rows)
        if min_stat is not None:
            keep &= C >= min_stat
        at = np.nonzero(keep)                                        # (row-major: sorted by (v, w))
        cols = np.stack(at, 1).astype(np.int32)
    else:
        at, cols = (given[:, 0], given[:, 1]), given.astype(np.int32)
    means = (mean, np.float64(mean_all)) if correction is not None else (None, None)
    return (cols.reshape(-1, 2), n[at].astype(np.int32).reshape(-1, 16), S[at].reshape(-1), C[at].reshape(-1)) + means


def _two_product(a, b):
    """(p, e) float64 with p = fl(a * b) and p + e = a * b exactly (Dekker's product; numpy has no fma), |a|, |b| < 2^53."""
    def split(x):
        t = x * 134217729.0                                          # 2^27 + 1
        hi = t - (t - x)
        return hi, x - hi
    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _host_ratio(a, b, c, d):
    """a * b / (c * d) of integers below 2^53 held as float64, rounded once (SqCovarWstat::ratio, csrc/sq_covar_wstat.h): the two
    products exact as a double and its residual each, the quotient of the leading parts corrected by the division's own
    residual -- or left as it is where both products are exact doubles: the quotient _host_raw forms."""
    num, num_lo = _two_product(a, b)
    den, den_lo = _two_product(c, d)
    q = num / den
    head, tail = _two_product(q, den)
    rest = ((num - head) - tail) + (num_lo - q * den_lo)
    return np.where((num_lo == 0) & (den_lo == 0), q, q + rest / den)


def _host_raw_w(Q, statistic):
    """S float64[...] of the weighted joint tables Q int64[..., 16] (sums of quantised weights): the margins and N are summed as
    int64, everything becomes a double once, x = Q / 2^20, and the formulas of _host_raw follow on the doubles, the terms added
    in the table's order; the quotient under the logarithm is _host_ratio's."""
    one = float(WEIGHT_ONE)
    sq = Q.reshape(Q.shape[:-1] + (4, 4))
    N, x = Q.sum(-1) / one, Q / one
    Qa, Qb = sq.sum(-1).astype(np.float64), sq.sum(-2).astype(np.float64)
    margins = ((Qa / one)[..., :, None] * (Qb / one)[..., None, :]).reshape(Q.shape)
    S = np.zeros(Q.shape[:-1], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(16):
            xk, mk = x[..., k], margins[..., k]
            if statistic == "chi":
                e = mk / N
                S = S + np.where(mk > 0, (xk - e) * (xk - e) / e, 0.0)
            else:
                weight = xk / N if statistic == "mi" else xk
                ratio = _host_ratio(Q[..., k].astype(np.float64), Q.sum(-1).astype(np.float64), Qa[..., k >> 2], Qb[..., k & 3])
                S = S + np.where(xk > 0, weight * np.log(ratio), 0.0)
    S = np.where(N > 0, S, 0.0)
    return 2.0 * S if statistic == "gt" else S


def _host_tables_w(cls, q):
    """int64[L, L, 16]: _host_tables with the quantised row weights q int64[R]: per cell of the table one int64 matrix product
    of the first letter's one-hot matrix and the second's times q."""
    hot = [(cls == k).astype(np.int64) for k in range(4)]
    return np.stack([hot[a].T @ (hot[b] * q[:, None]) for a in range(4) for b in range(4)], -1)


def _host_statistics_w(rows, q, given, statistic, correction, minspan, min_rows, min_stat):
    """_host_statistics with the quantised row weights q int64[R]: the joint table is Q int64[P, 16] (_host_tables_w), and
    min_rows is compared with the sum of Q / 2^20."""
    L = rows.shape[1]
    Q = _host_tables_w(_classes(rows), q)
    S = _host_raw_w(Q, statistic)
    mean, mean_all = _host_means(S) if correction is not None else (np.zeros(L), 0.0)
    C = _host_corrected(S, mean[:, None], mean[None, :], mean_all, correction)
    if given is None:
        v, w = np.indices((L, L))
        keep = (w > v) & (w - v >= minspan) & (Q.sum(-1) / float(WEIGHT_ONE) >= min_rows)
        if min_stat is not None:
            keep &= C >= min_stat
        at = np.nonzero(keep)                                        # (row-major: sorted by (v, w))
        cols = np.stack(at, 1).astype(np.int32)
    else:
        at, cols = (given[:, 0], given[:, 1]), given.astype(np.int32)
    means = (mean, np.float64(mean_all)) if correction is not None else (None, None)
    return (cols.reshape(-1, 2), Q[at].reshape(-1, 16), S[at].reshape(-1), C[at].reshape(-1)) + means


def _row_weights(who, weights, R):
    """weights= as a float64 torch tensor [R] on the device it came on (a sequence or a numpy array: the host); ValueError
    when it is not R finite numbers in 0 .. MAX_WEIGHT."""
    import torch
    try:
        w = weights.detach() if hasattr(weights, "detach") else torch.from_numpy(np.array(weights, dtype=np.float64))
        w = w.to(torch.float64).reshape(-1).contiguous()
    except Exception:
        raise ValueError("{}: weights is a sequence, an array or a tensor of numbers, one per row".format(who))
    if int(w.numel()) != R:
        raise ValueError("{}: weights has {} entries for {} rows".format(who, int(w.numel()), R))
    if R > MAX_WEIGHTED_ROWS:
        raise ValueError("{}: weights takes at most 2^22 rows: {}".format(who, R))
    if not bool((torch.isfinite(w) & (w >= 0) & (w <= MAX_WEIGHT)).all()):         # (one flag comes to the host, not the weights)
        raise ValueError("{}: weights are finite numbers from 0 to {:g}".format(who, MAX_WEIGHT))
    return w


class CovariationStatisticsResult(TensorResult):
    """What ``CovariationStatistics`` computes for an alignment of R rows and L columns.

    Host attributes: ``names``, ``sequences`` (as given), ``R``, ``L``, ``statistic``, ``correction``, ``mode`` ("scan": every
    cell that passed the thresholds; "pairs": the given pairs) and ``source`` ("device" or "host").  Torch tensors on
    ``device``: ``pair_cols`` int32[P, 2] -- the column pairs (v, w), v < w, sorted by (v, w) in scan mode and in the given order
    otherwise --, ``joint`` int32[P, 16] -- the joint table, cell ``a * 4 + b`` (``CELLS``) = the rows with ``LETTERS[a]`` at v
    and ``LETTERS[b]`` at w --, ``raw`` float64[P] = S, ``value`` float64[P] = C, and with a correction ``col_mean`` float64[L]
    and ``mean_all`` (a 0-dim float64 tensor); both are None without one.  Derived with torch ops: ``rows`` (N),
    ``marginals()``, ``canonical()``, ``to_matrix()``, ``top()``.

    With ``weights=``: ``weights`` float64[R], the weights as given, on ``device`` (None without), and ``joint`` is
    float64[P, 16], the sum of the rows' quantised weights per cell (multiples of 2^-20, exact); ``rows``, ``marginals()``,
    ``canonical()``, ``of()`` and ``to_matrix()`` of a cell or of "rows" are then float64 as well."""

    LETTERS, CELLS, TYPES = LETTERS, CELLS, TYPES
    _TENSORS = ("value", "pair_cols", "joint", "raw", "col_mean", "mean_all", "weights")

    def __init__(self, names, sequences, statistic, correction, mode, source, pair_cols, joint, raw, value, col_mean, mean_all,
                 weights=None):
        self.names, self.sequences, self.R, self.L = names, sequences, len(sequences), len(sequences[0])
        self.statistic, self.correction, self.mode, self.source = statistic, correction, mode, source
        self.pair_cols, self.joint, self.raw, self.value, self.col_mean, self.mean_all = pair_cols, joint, raw, value, col_mean, mean_all
        self.weights = weights

    def __len__(self):
        return int(self.value.numel())

    @property
    def rows(self):
        """int32[P]: N, the rows that hold a residue in both columns (float64[P] with weights: their weights' sum)."""
        return self.joint.sum(1, dtype=self.joint.dtype)

    def marginals(self):
        """(na int32[P, 4], nb int32[P, 4]): the rows with each residue of ``LETTERS`` at v and at w, among the N rows (float64 with
        weights)."""
        sq = self.joint.reshape(-1, 4, 4)
        return sq.sum(2, dtype=self.joint.dtype), sq.sum(1, dtype=self.joint.dtype)

    def canonical(self):
        """int32[P, 6]: the joint table's six canonical entries in the order of ``TYPES`` (``Covariation``'s counts[:, :6])."""
        return self.joint[:, _CANONICAL]

    def _field(self, field):
        if field in _FIELDS:
            return getattr(self, field)
        if field in CELLS:
            return self.joint[:, CELLS.index(field)]
        raise ValueError("CovariationStatisticsResult: field is one of {} or a cell of the joint table such as 'GC': {!r}".format(
            ", ".join(_FIELDS), field))

    def to_matrix(self, field="value"):
        """[L, L] on the tensors' device, symmetric: `field` of every pair of the result, 0 elsewhere -- float64 for "value" and
        "raw", int64 for "rows" and a cell of the joint table such as "GC" (counted at (v, w) with v < w)."""
        import torch
        val = self._field(field)
        val = val if val.is_floating_point() else val.long()
        out = torch.zeros((self.L, self.L), dtype=val.dtype, device=self.device)
        v, w = self.pair_cols[:, 0].long(), self.pair_cols[:, 1].long()
        out[v, w] = val
        out[w, v] = val
        return out

    def of(self, v, w):
        """The record of columns (v, w) (or (w, v)) as a dict of host numbers: the joint table's cells by name, rows, raw and
        value; KeyError when the result has no such pair."""
        v, w = (int(v), int(w)) if v < w else (int(w), int(v))
        at = ((self.pair_cols[:, 0] == v) & (self.pair_cols[:, 1] == w)).nonzero()
        if not at.numel():
            raise KeyError((v, w))
        k = int(at[0, 0])
        n = self.joint[k].tolist()
        rec = dict(zip(CELLS, n))
        rec.update(rows=sum(n), raw=float(self.raw[k]), value=float(self.value[k]))
        return rec

    def top(self, k):
        """The result of the `k` pairs with the largest ``value``, largest first (equal values in the result's order)."""
        import torch
        import copy
        order = torch.sort(self.value, descending=True, stable=True)[1][:max(int(k), 0)]
        new = copy.copy(self)
        for key in ("pair_cols", "joint", "raw", "value"):
            setattr(new, key, getattr(self, key)[order])
        return new


def CovariationStatistics(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None, alignment=None, pairs=None,
                          statistic="gt", correction="apc", minspan=4, min_rows=1, min_stat=None, ignorewarn=False, weights=None):
    """Covariation statistics of pairs of columns of an alignment, returned as a :class:`CovariationStatisticsResult`.

    The inputs and ``pairs`` mean what they mean in ``Covariation``.  ``statistic``: "mi", "gt" or "chi"; ``correction``:
    "apc", "asc" or None (the module's text has the definitions).  A scan keeps the cells v < w with ``w - v >= minspan``,
    at least ``min_rows`` rows that hold a residue in both columns and a corrected value ``>= min_stat`` (None: any value).
    Given pairs are taken as they are, in their order, whatever the thresholds; one that is not 0 <= v < w < L raises
    RuntimeError.  The column means are those of every pair of distinct columns in both modes.

    A record is 88 bytes on the device.  With ``min_stat=None`` a scan returns nearly every cell in scope, about 44 L^2 bytes
    (1.1 GB at 5,000 columns): up to 2^20 cells in scope the result buffers are sized for all of them at once, beyond that a
    first scan counts and a second stores (``_SCAN_CAP``).  Set ``min_stat`` to get the pairs that matter.

    ``weights``: None, or one weight per row as a sequence, a numpy array or a torch tensor on any device, taken as float64
    (``RowIdentity(...).weights()`` goes in as it is and stays on its device).  A weight is a finite number from 0 to 2048;
    a row of weight 0 takes part in nothing.  The joint table, N and the statistics are then those of the weighted rows (the
    module's text), ``min_rows`` may be a float and is compared with the weighted N, and the result has ``weights`` and a
    float64 ``joint``.  ValueError for a wrong length, a NaN, an infinite or negative weight or one above 2048."""
    import torch
    who = "CovariationStatistics"
    if statistic not in STATISTICS:
        raise ValueError("{}: statistic is one of {}: {!r}".format(who, ", ".join(STATISTICS), statistic))
    if correction is not None and correction not in CORRECTIONS:
        raise ValueError("{}: correction is 'apc', 'asc' or None: {!r}".format(who, correction))
    if min_stat is not None:
        if isinstance(min_stat, bool) or not isinstance(min_stat, (int, float, np.integer, np.floating)) or math.isnan(min_stat):
            raise ValueError("{}: min_stat is a number or None: {!r}".format(who, min_stat))
        min_stat = float(min_stat)
    if weights is not None:                                          # (a float is allowed: _open takes the other thresholds)
        if isinstance(min_rows, bool) or not isinstance(min_rows, (int, float, np.integer, np.floating)) or not min_rows >= 0:
            raise ValueError("{}: with weights min_rows is a non-negative number: {!r}".format(who, min_rows))
        weighted_rows, min_rows = float(min_rows), 0
    names, seqs, (minspan, min_rows, _), given, rows = _open(who, inputfile, fileformat, inputformat, sequences, names, alignment, pairs,
                                                            minspan, min_rows, 0, ignorewarn)
    L = rows.shape[1]
    eng = _engine.get_engine()
    if weights is not None:
        return _weighted(who, eng, names, seqs, rows, given, alignment, _row_weights(who, weights, rows.shape[0]), statistic, correction,
                         minspan, weighted_rows, min_stat)
    on_device = _device_engine(eng, _DEVICE_METHODS)
    if on_device:
        if alignment is not None and alignment.device.type == "cuda":
            dev = alignment.device
        elif hasattr(given, "is_cuda") and given.is_cuda:
            dev = given.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
        d_rows = torch.from_numpy(rows.copy()).to(dev)
        if given is None:
            span = L - max(minspan, 1)                               # the cells in scope: span * (span + 1) / 2
            cap = max(span * (span + 1) // 2, 1) if min_stat is None and span * (span + 1) // 2 <= _SCAN_CAP else None
            flat, joint, raw, value, mean = eng.covariation_stat_scan(d_rows, statistic, correction, minspan, min_rows, min_stat, cap=cap)
            flat, order = torch.sort(flat)
            cols, joint, raw, value = torch.stack((flat // L, flat % L), 1).to(torch.int32), joint[order], raw[order], value[order]
        else:
            cols = (given if hasattr(given, "dim") else torch.from_numpy(given)).to(device=dev, dtype=torch.int32).contiguous()
            joint, raw, value, mean = eng.covariation_stat_pairs(d_rows, cols, statistic, correction)
        col_mean, mean_all = (mean[:L], mean[L]) if mean is not None else (None, None)
    else:
        if given is not None:
            given = (given.cpu() if hasattr(given, "dim") else torch.from_numpy(given)).to(torch.int64).numpy().reshape(-1, 2)
            if len(given) and not ((given[:, 0] >= 0) & (given[:, 0] < given[:, 1]) & (given[:, 1] < L)).all():
                raise RuntimeError("%s: a pair is not 0 <= v < w < %d columns" % (who, L))
        cols, joint, raw, value, col_mean, mean_all = (
            None if a is None else torch.from_numpy(np.array(a))     # (np.array: mean_all stays 0-dim)
            for a in _host_statistics(rows, given, statistic, correction, minspan, min_rows, min_stat))
    return CovariationStatisticsResult(names, seqs, statistic, correction, "scan" if given is None else "pairs",
                                       "device" if on_device else "host", cols, joint, raw, value, col_mean, mean_all)


def _weighted(who, eng, names, seqs, rows, given, alignment, weights, statistic, correction, minspan, min_rows, min_stat):
    """CovariationStatistics with weights= (a float64 tensor [R] from _row_weights): the device entries of the weighted
    statistics when the engine has both, numpy otherwise."""
    import torch
    L = rows.shape[1]
    on_device = _device_engine(eng, _DEVICE_METHODS_W)
    if on_device:
        if weights.is_cuda:
            dev = weights.device
        elif alignment is not None and alignment.device.type == "cuda":
            dev = alignment.device
        elif hasattr(given, "is_cuda") and given.is_cuda:
            dev = given.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
        d_rows, weights = torch.from_numpy(rows.copy()).to(dev), weights.to(dev)
        if given is None:
            span = L - max(minspan, 1)                               # the cells in scope: span * (span + 1) / 2
            cap = max(span * (span + 1) // 2, 1) if min_stat is None and span * (span + 1) // 2 <= _SCAN_CAP else None
            flat, Q, raw, value, mean = eng.covariation_wstat_scan(d_rows, weights, statistic, correction, minspan, min_rows, min_stat, cap=cap)
            flat, order = torch.sort(flat)
            cols, Q, raw, value = torch.stack((flat // L, flat % L), 1).to(torch.int32), Q[order], raw[order], value[order]
        else:
            cols = (given if hasattr(given, "dim") else torch.from_numpy(given)).to(device=dev, dtype=torch.int32).contiguous()
            Q, raw, value, mean = eng.covariation_wstat_pairs(d_rows, weights, cols, statistic, correction)
        col_mean, mean_all = (mean[:L], mean[L]) if mean is not None else (None, None)
    else:
        if given is not None:
            given = (given.cpu() if hasattr(given, "dim") else torch.from_numpy(given)).to(torch.int64).numpy().reshape(-1, 2)
            if len(given) and not ((given[:, 0] >= 0) & (given[:, 0] < given[:, 1]) & (given[:, 1] < L)).all():
                raise RuntimeError("%s: a pair is not 0 <= v < w < %d columns" % (who, L))
        weights = weights.cpu()
        q = np.rint(weights.numpy() * float(WEIGHT_ONE)).astype(np.int64)    # (the product is exact; ties to even)
        cols, Q, raw, value, col_mean, mean_all = (
            None if a is None else torch.from_numpy(np.array(a))     # (np.array: mean_all stays 0-dim)
            for a in _host_statistics_w(rows, q, given, statistic, correction, minspan, min_rows, min_stat))
    joint = Q.double() * (1.0 / WEIGHT_ONE)                          # (a power of two: exact)
    return CovariationStatisticsResult(names, seqs, statistic, correction, "scan" if given is None else "pairs",
                                       "device" if on_device else "host", cols, joint, raw, value, col_mean, mean_all, weights)
