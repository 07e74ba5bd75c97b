"""``CovariationSignificance``: is the ``cov`` of a pair of alignment columns remarkable?

``Covariation`` reports ``cov`` per pair of columns; two G/A-rich and C/U-rich columns reach a high value by chance.  The
answer here is an empirical null, as the tools that report covariation evidence give it: destroy the association between the
columns, keep every column's composition, and see how often the statistic gets that high.  Sample k of ``samples`` permutes
the rows of every column on its own -- gaps and other bytes move like letters (a null that keeps the gap pattern is not
offered) -- and the covs of all in-scope cells (v < w, ``w - v >= minspan``) of the shuffled alignment are one sample of the
null.  ``min_rows`` and ``min_cov`` filter the observed pairs only, never the null.  The shuffle is a fixed function of
``seed``, the sample, the column and the row (``csrc/sq_covar_null.h``): the same seed gives the same numbers on every engine.

With the GPU engine nothing but two status words comes back: the shuffled alignments exist only as bit planes on the device
(``sq_covariation_null``: a sort per column in LDS, the all-pairs scan of ``Covariation`` reduced to a histogram, a lookup per
pair).  An engine without the device method gets the same object with numpy.  All numbers are integers.
"""
import numpy as np

from . import engine as _engine
from .covariation import _DEVICE_METHODS, _classes, _device_engine, _host_cells, _observe, _open
from .results import TensorResult

_NULL_METHODS = _DEVICE_METHODS + ("covariation_null",)
_MASK = (1 << 64) - 1
_FIELDS = ("null_ge", "own_ge", "evalue", "pvalue", "pvalue_max")


def _sortkeys(R, L, k, seed):
    """uint64[R, L]: the sort key of row r of column c of sample k (csrc/sq_covar_null.h), every product mod 2^64."""
    r = np.arange(R, dtype=np.uint64)[:, None]
    c = np.arange(L, dtype=np.uint64)[None, :]
    z = (np.uint64((k * L) & _MASK) + c) * np.uint64(R) + r
    z = (z + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.full((1, 1), seed, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(_MASK ^ 0xFFFF)) | r


def _shuffled_classes(cls, k, seed):
    """The class bytes uint8[R, L] of sample k: row j of a column holds the class of the row with the j-th smallest key."""
    R, L = cls.shape
    assert R <= 65535, "the sort keys hold at most 65,535 rows"
    return np.take_along_axis(cls, np.argsort(_sortkeys(R, L, k, seed), axis=0), 0)


def scope_cells(L, minspan):
    """The in-scope cells of one sample: the (v, w) with v < w < L and w - v >= minspan."""
    m = max(int(minspan), 1)
    return 0 if m >= L else (L - m) * (L - m + 1) // 2


def _host_null(rows, pairs, cov, minspan, samples, seed):
    """(null_ge int64[P], own_ge int32[P], null_max int64[samples]) with numpy: per sample an argsort of the sort keys and the
    one-hot matrix products of Covariation's numpy path (deliberately not the kernels' form)."""
    cls = _classes(rows)
    L, P = cls.shape[1], len(cov)
    thresholds = np.unique(cov)
    hist = np.zeros(len(thresholds) + 1, np.int64)
    own_ge, null_max = np.zeros(P, np.int32), np.zeros(samples, np.int64)
    v, w = np.indices((L, L))
    scope = (w > v) & (w - v >= minspan)
    for k in range(samples):
        null = _host_cells(_shuffled_classes(cls, k, seed))[1]
        cells = null[scope]
        hist += np.bincount(np.searchsorted(thresholds, cells, side="right"), minlength=len(hist))
        null_max[k] = cells.max(initial=0)
        if P:
            own_ge += null[pairs[:, 0], pairs[:, 1]] >= cov
    from_bin = np.cumsum(hist[::-1])[::-1]
    return from_bin[np.searchsorted(thresholds, cov) + 1] if P else np.zeros(0, np.int64), own_ge, null_max


class SignificanceResult(TensorResult):
    """What ``CovariationSignificance`` computes for the P observed pairs of ``observed`` (a :class:`CovariationResult`).

    Host attributes: ``samples`` (K), ``seed``, ``null_cells`` (K x the in-scope cells of one sample: the size of the pooled
    null) and ``source`` ("device" or "host": where the null was formed).  Torch tensors on ``device``: ``null_ge`` int64[P] --
    over all samples and in-scope cells, the null cells with ``cov_null >= cov[p]`` (the pooled null) --, ``own_ge`` int32[P]
    -- the samples in which the same cell (v, w) has ``cov_null >= cov[p]`` (the per-pair permutation test) --, ``null_max``
    int64[K] -- the largest ``cov_null`` of a sample's in-scope cells, 0 without one (the max-statistic, family-wise test)."""

    _TENSORS = ("null_ge", "own_ge", "null_max")
    _NESTED = ("observed",)

    def __init__(self, observed, samples, seed, null_cells, source, null_ge, own_ge, null_max):
        self.observed, self.samples, self.seed, self.null_cells, self.source = observed, samples, seed, null_cells, source
        self.null_ge, self.own_ge, self.null_max = null_ge, own_ge, null_max

    def __len__(self):
        return int(self.null_ge.numel())

    # (divided by tensors, as CovariationResult.score: by a Python number the device form multiplies with the reciprocal)
    def evalue(self):
        """float64[P]: null_ge / samples, the expected number of null pairs per alignment that score at least cov[p]."""
        import torch
        n = self.null_ge.double()
        return n / torch.full_like(n, self.samples)

    def pvalue(self):
        """float64[P]: (1 + own_ge) / (samples + 1), the permutation p-value of the pair's own cell."""
        import torch
        n = (self.own_ge.long() + 1).double()
        return n / torch.full_like(n, self.samples + 1)

    def max_ge(self):
        """int64[P]: the samples whose largest null cov reaches cov[p]."""
        import torch
        below = torch.searchsorted(torch.sort(self.null_max)[0], self.observed.cov.contiguous())     # the samples with null_max < cov[p]
        return self.samples - below

    def pvalue_max(self):
        """float64[P]: (1 + the samples whose largest null cov reaches cov[p]) / (samples + 1), family-wise over the cells."""
        import torch
        n = (self.max_ge() + 1).double()
        return n / torch.full_like(n, self.samples + 1)

    def significant(self, evalue=0.05):
        """bool[P]: the pairs whose evalue() is at most `evalue`."""
        return self.evalue() <= float(evalue)

    def to_matrix(self, field="evalue"):
        """[L, L] on the tensors' device, symmetric: `field` of every pair of the result, 0 elsewhere -- int64 for "null_ge" and
        "own_ge", float64 for "evalue", "pvalue" and "pvalue_max"; any other field is the observed result's."""
        import torch
        if field not in _FIELDS:
            return self.observed.to_matrix(field)
        val = getattr(self, field)
        val = val() if callable(val) else val.long()
        out = torch.zeros((self.observed.L, self.observed.L), dtype=val.dtype, device=self.device)
        v, w = self.observed.pair_cols[:, 0].long(), self.observed.pair_cols[:, 1].long()
        out[v, w] = val
        out[w, v] = val
        return out

    def of(self, v, w):
        """The observed record of columns (v, w) (CovariationResult.of) with null_ge, own_ge, evalue, pvalue and pvalue_max."""
        rec = self.observed.of(v, w)
        v, w = (int(v), int(w)) if v < w else (int(w), int(v))
        cols = self.observed.pair_cols
        k = int(((cols[:, 0] == v) & (cols[:, 1] == w)).nonzero()[0, 0])
        rec.update(null_ge=int(self.null_ge[k]), own_ge=int(self.own_ge[k]), evalue=float(self.evalue()[k]), pvalue=float(self.pvalue()[k]),
                   pvalue_max=float(self.pvalue_max()[k]))
        return rec


def CovariationSignificance(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None, alignment=None, pairs=None,
                            minspan=4, min_rows=1, min_cov=1, samples=100, seed=0, ignorewarn=False):
    """The observed covariation of pairs of columns of an alignment against a shuffled-column null, returned as a
    :class:`SignificanceResult`.

    The inputs, ``pairs`` and the thresholds mean what they mean in ``Covariation``, whose result is ``.observed``.  The
    null: ``samples`` (an int >= 1) shuffled alignments, each with the rows of every column permuted on its own by a fixed
    function of ``seed`` (an int in [0, 2^64)); its cells are the v < w with ``w - v >= minspan``, whatever ``min_rows`` and
    ``min_cov``.  Gaps and other bytes move like letters.  At most 65,535 rows; on the device at most
    ``device_calls.COVAR_NULL_MAX_ROWS``."""
    import torch
    who = "CovariationSignificance"
    names, seqs, thresholds, given, rows = _open(who, inputfile, fileformat, inputformat, sequences, names, alignment, pairs,
                                                 minspan, min_rows, min_cov, ignorewarn)
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError("{}: samples is an integer >= 1: {!r}".format(who, samples))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= _MASK:
        raise ValueError("{}: seed is an integer in [0, 2^64): {!r}".format(who, seed))
    samples, seed, (R, L) = int(samples), int(seed), rows.shape
    if R > 65535:
        raise ValueError("{}: {} rows; the shuffle's sort keys hold at most 65,535".format(who, R))
    eng = _engine.get_engine()
    on_device = _device_engine(eng, _NULL_METHODS)
    if on_device:
        from .device_calls import COVAR_NULL_MAX_ROWS
        if R > COVAR_NULL_MAX_ROWS:
            raise ValueError("{}: {} rows; the device shuffles at most COVAR_NULL_MAX_ROWS = {}".format(who, R, COVAR_NULL_MAX_ROWS))
    observed, d_rows = _observe(who, eng, names, seqs, thresholds, given, rows, alignment)
    if on_device:
        null_ge, own_ge, null_max = eng.covariation_null(d_rows, observed.pair_cols, observed.cov, thresholds[0], samples, seed)
    else:
        host = observed.cpu()
        null_ge, own_ge, null_max = (torch.from_numpy(np.ascontiguousarray(a)).to(observed.device) for a in _host_null(
            rows, host.pair_cols.numpy().astype(np.int64), host.cov.numpy(), thresholds[0], samples, seed))
    return SignificanceResult(observed, samples, seed, samples * scope_cells(L, thresholds[0]), "device" if on_device else "host",
                              null_ge, own_ge, null_max)
