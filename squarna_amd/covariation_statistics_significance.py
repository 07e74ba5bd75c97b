"""``CovariationStatisticsSignificance``: is the MI, G-test or chi-square value of a pair of alignment columns remarkable?

``CovariationStatistics`` states the numbers a pair of columns is judged by -- ``statistic="gt", correction="apc"`` is R-scape's
GTp --, and such a number means little without a null: R-scape reports E-values for exactly that reason.  The null here is that
of ``CovariationSignificance``: sample k of ``samples`` permutes the rows of every column on its own (the fixed function of
``seed``, the sample, the column and the row of ``csrc/sq_covar_null.h``; gaps and other bytes move like letters), and the
values of all in-scope cells (v < w, ``w - v >= minspan``) of the shuffled alignment are one sample of the null.  A null
cell's value is C of the chosen statistic and correction with the column means of that shuffled sample over every pair of its
distinct columns: what ``CovariationStatistics`` returns for the shuffled alignment.  ``min_rows`` and ``min_stat`` filter the
observed pairs only, never the null.

With the GPU engine nothing but two status words comes back (``sq_covariation_stat_null``: the shuffled alignments exist only
as bit planes on the device, each sample's means are formed by the first pass of ``sq_covariation_stat_scan``, and the second
pass is reduced to a histogram against the observed values; no record and no L x L matrix is stored).  An engine without the
device method (the tests' CPU engine, the sharded one) gets the same object with numpy; its counts can differ from the
device's only where a null value lies within the float bound of an observed one.

``weights=`` gives the null of the weighted statistics (``CovariationStatistics(weights=)``).  The weights belong to the row
slots, not to the letters: sample k permutes the rows of every column exactly as without weights, and row r of the shuffled
alignment keeps weight r.  A null cell's value is then what ``CovariationStatistics(weights=weights)`` returns for the
shuffled alignment (``sq_covariation_wstat_null`` on the device: the bits of ``sq_covariation_wstat_scan`` on the shuffled
rows).  A row of weight 0 takes part in the shuffle -- its letters move -- and counts nothing.  The shuffle keeps each
column's letter counts; it does not keep each column's weighted composition: that is the plain meaning of "the same analysis
on a shuffled alignment", and what a hand-written loop over shuffled alignments would do.
"""
import numpy as np

from . import engine as _engine
from .covariation import _classes, _device_engine
from .covariation_significance import _MASK, SignificanceResult, _shuffled_classes, scope_cells
from .covariation_statistics import (_DEVICE_METHODS, _DEVICE_METHODS_W, WEIGHT_ONE, CovariationStatistics, _host_corrected, _host_means,
                                     _host_raw, _host_raw_w, _host_tables, _host_tables_w)

_NULL_METHODS = _DEVICE_METHODS + ("covariation_stat_null",)
_NULL_METHODS_W = _DEVICE_METHODS_W + ("covariation_wstat_null",)


def _host_stat_null(rows, pairs, value, statistic, correction, minspan, samples, seed):
    """(null_ge int64[P], own_ge int32[P], null_max float64[samples]) with numpy: per sample an argsort of the sort keys and
    the one-hot matrix products, means and corrections of CovariationStatistics' numpy path (deliberately not the kernels'
    form)."""
    return _host_null(_classes(rows), lambda cls: _host_raw(_host_tables(cls), statistic), pairs, value, correction, minspan, samples, seed)


def _host_stat_null_w(rows, q, pairs, value, statistic, correction, minspan, samples, seed):
    """_host_stat_null with the quantised row weights q int64[R]: row r of every shuffled sample keeps q[r], and S is that of
    CovariationStatistics(weights=)'s numpy path on the weighted tables."""
    return _host_null(_classes(rows), lambda cls: _host_raw_w(_host_tables_w(cls, q), statistic), pairs, value, correction, minspan, samples,
                      seed)


def _host_null(cls, raw_of, pairs, value, correction, minspan, samples, seed):
    """What the two numpy nulls share: cls uint8[R, L] the class bytes of the rows, raw_of(class bytes) = S float64[L, L] of an
    alignment."""
    L, P = cls.shape[1], len(value)
    thresholds = np.unique(value)
    hist = np.zeros(len(thresholds) + 1, np.int64)
    own_ge, null_max = np.zeros(P, np.int32), np.full(samples, -np.inf, np.float64)
    v, w = np.indices((L, L))
    scope = (w > v) & (w - v >= minspan)
    for k in range(samples):
        S = raw_of(_shuffled_classes(cls, k, seed))
        mean, mean_all = _host_means(S) if correction is not None else (np.zeros(L), 0.0)
        null = _host_corrected(S, mean[:, None], mean[None, :], mean_all, correction)
        cells = null[scope]
        hist += np.bincount(np.searchsorted(thresholds, cells, side="right"), minlength=len(hist))
        null_max[k] = cells.max(initial=-np.inf)
        if P:
            own_ge += null[pairs[:, 0], pairs[:, 1]] >= value
    from_bin = np.cumsum(hist[::-1])[::-1]
    return from_bin[np.searchsorted(thresholds, value) + 1] if P else np.zeros(0, np.int64), own_ge, null_max


class StatisticsSignificanceResult(SignificanceResult):
    """What ``CovariationStatisticsSignificance`` computes for the P observed pairs of ``observed`` (a
    :class:`CovariationStatisticsResult`); ``evalue()``, ``pvalue()``, ``max_ge()``, ``pvalue_max()``, ``significant()``,
    ``to_matrix()`` and ``of()`` are :class:`SignificanceResult`'s, with ``observed.value`` in the place of ``cov``.

    Host attributes: ``samples`` (K), ``seed``, ``null_cells`` (K x the in-scope cells of one sample: the size of the pooled
    null) and ``source`` ("device" or "host": where the null was formed).  Torch tensors on ``device``: ``null_ge`` int64[P] --
    over all samples and in-scope cells, the null cells with ``C_null >= value[p]`` (the pooled null) --, ``own_ge`` int32[P]
    -- the samples in which the same cell (v, w) has ``C_null >= value[p]`` (the per-pair permutation test) --, ``null_max``
    float64[K] -- the largest ``C_null`` of a sample's in-scope cells, ``-inf`` without one (the max-statistic, family-wise
    test).  All comparisons are IEEE ``>=`` on doubles; no value is NaN.  ``weights``: that of ``observed`` (float64[R], or None
    without ``weights=``)."""

    @property
    def weights(self):
        return self.observed.weights

    def max_ge(self):
        """int64[P]: the samples whose largest null value reaches value[p]."""
        import torch
        below = torch.searchsorted(torch.sort(self.null_max)[0], self.observed.value.contiguous())    # the samples with null_max < value[p]
        return self.samples - below


def CovariationStatisticsSignificance(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None,
                                      alignment=None, pairs=None, statistic="gt", correction="apc", minspan=4, min_rows=1,
                                      min_stat=None, samples=100, seed=0, ignorewarn=False, weights=None):
    """The observed covariation statistic of pairs of columns of an alignment against a shuffled-column null, returned as a
    :class:`StatisticsSignificanceResult`.

    The inputs, ``pairs``, ``statistic``, ``correction`` and the thresholds mean what they mean in ``CovariationStatistics``,
    whose result is ``.observed``.  The null: ``samples`` (an int >= 1) shuffled alignments, each with the rows of every
    column permuted on its own by a fixed function of ``seed`` (an int in [0, 2^64)); its cells are the v < w with
    ``w - v >= minspan``, whatever ``min_rows`` and ``min_stat``, and a cell's value is C with the column means of its own
    shuffled sample.  Gaps and other bytes move like letters.  At most 65,535 rows; on the device at most
    ``device_calls.COVAR_NULL_MAX_ROWS``.

    ``weights``: None, or one weight per row as ``CovariationStatistics`` takes them (finite, 0 to 2048; ``min_rows`` may then
    be a float and is compared with the weighted N; weights on a CUDA device decide the device).  ``.observed`` is
    ``CovariationStatistics(..., weights=weights)`` and the null is that of the weighted statistic: the rows of every column
    are permuted exactly as without weights and row r keeps weight r, so a null cell's value is what
    ``CovariationStatistics(weights=weights)`` returns for the shuffled alignment.  A row of weight 0 is shuffled and counts
    nothing.  The shuffle keeps each column's letter counts, not its weighted composition.  The result has ``weights``."""
    import torch
    who = "CovariationStatisticsSignificance"
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError("{}: samples is an integer >= 1: {!r}".format(who, samples))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= _MASK:
        raise ValueError("{}: seed is an integer in [0, 2^64): {!r}".format(who, seed))
    samples, seed = int(samples), int(seed)
    eng = _engine.get_engine()
    on_device = _device_engine(eng, _NULL_METHODS if weights is None else _NULL_METHODS_W)
    rows_cap = 65535
    if on_device:
        from .device_calls import COVAR_NULL_MAX_ROWS as rows_cap
    if sequences is not None and len(sequences) > rows_cap:        # (before anything is computed; any other input: below)
        _refuse_rows(who, len(sequences))
    observed = CovariationStatistics(inputfile, fileformat, inputformat, sequences, names, alignment, pairs, statistic, correction, minspan,
                                     min_rows, min_stat, ignorewarn, weights)
    R, L, minspan = observed.R, observed.L, int(minspan)
    if R > rows_cap:
        _refuse_rows(who, R)
    # one byte per character, as CovariationStatistics read them
    rows = np.frombuffer("".join(observed.sequences).encode("latin-1", "replace"), np.uint8).reshape(R, L)
    if on_device:
        d_rows = torch.from_numpy(rows.copy()).to(observed.device)
        if weights is None:
            null_ge, own_ge, null_max = eng.covariation_stat_null(d_rows, observed.pair_cols, observed.value, statistic, correction, minspan,
                                                                  samples, seed)
        else:
            null_ge, own_ge, null_max = eng.covariation_wstat_null(d_rows, observed.weights, observed.pair_cols, observed.value, statistic,
                                                                   correction, minspan, samples, seed)
    else:
        host = observed.cpu()
        given = (rows, host.pair_cols.numpy().astype(np.int64), host.value.numpy(), statistic, correction, minspan, samples, seed)
        if weights is None:
            null = _host_stat_null(*given)
        else:
            q = np.rint(host.weights.numpy() * float(WEIGHT_ONE)).astype(np.int64)  # (as CovariationStatistics quantised them)
            null = _host_stat_null_w(rows, q, *given[1:])
        null_ge, own_ge, null_max = (torch.from_numpy(np.ascontiguousarray(a)).to(observed.device) for a in null)
    return StatisticsSignificanceResult(observed, samples, seed, samples * scope_cells(L, minspan), "device" if on_device else "host",
                                        null_ge, own_ge, null_max)


def _refuse_rows(who, R):
    if R > 65535:
        raise ValueError("{}: {} rows; the shuffle's sort keys hold at most 65,535".format(who, R))
    from .device_calls import COVAR_NULL_MAX_ROWS
    raise ValueError("{}: {} rows; the device shuffles at most COVAR_NULL_MAX_ROWS = {}".format(who, R, COVAR_NULL_MAX_ROWS))
