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
"""
import numpy as np

from . import engine as _engine
from .covariation import _classes, _device_engine
from .covariation_significance import _MASK, SignificanceResult, _shuffled_classes, scope_cells
from .covariation_statistics import (_DEVICE_METHODS, CovariationStatistics, _host_corrected, _host_means, _host_raw, _host_tables)

_NULL_METHODS = _DEVICE_METHODS + ("covariation_stat_null",)


def _host_stat_null(rows, pairs, value, statistic, correction, minspan, samples, seed):
    """(null_ge int64[P], own_ge int32[P], null_max float64[samples]) with numpy: per sample an argsort of the sort keys and
    the one-hot matrix products, means and corrections of CovariationStatistics' numpy path (deliberately not the kernels'
    form)."""
    cls = _classes(rows)
    L, P = cls.shape[1], len(value)
    thresholds = np.unique(value)
    hist = np.zeros(len(thresholds) + 1, np.int64)
    own_ge, null_max = np.zeros(P, np.int32), np.full(samples, -np.inf, np.float64)
    v, w = np.indices((L, L))
    scope = (w > v) & (w - v >= minspan)
    for k in range(samples):
        S = _host_raw(_host_tables(_shuffled_classes(cls, k, seed)), statistic)
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
    test).  All comparisons are IEEE ``>=`` on doubles; no value is NaN."""

    def max_ge(self):
        """int64[P]: the samples whose largest null value reaches value[p]."""
        import torch
        below = torch.searchsorted(torch.sort(self.null_max)[0], self.observed.value.contiguous())    # the samples with null_max < value[p]
        return self.samples - below


def CovariationStatisticsSignificance(inputfile=None, fileformat="unknown", inputformat="qtrf", sequences=None, names=None,
                                      alignment=None, pairs=None, statistic="gt", correction="apc", minspan=4, min_rows=1,
                                      min_stat=None, samples=100, seed=0, ignorewarn=False):
    """The observed covariation statistic of pairs of columns of an alignment against a shuffled-column null, returned as a
    :class:`StatisticsSignificanceResult`.

    The inputs, ``pairs``, ``statistic``, ``correction`` and the thresholds mean what they mean in ``CovariationStatistics``,
    whose result is ``.observed``.  The null: ``samples`` (an int >= 1) shuffled alignments, each with the rows of every
    column permuted on its own by a fixed function of ``seed`` (an int in [0, 2^64)); its cells are the v < w with
    ``w - v >= minspan``, whatever ``min_rows`` and ``min_stat``, and a cell's value is C with the column means of its own
    shuffled sample.  Gaps and other bytes move like letters.  At most 65,535 rows; on the device at most
    ``device_calls.COVAR_NULL_MAX_ROWS``.  Row weights (``CovariationStatistics(weights=)``) are not taken here: ``.observed``
    and the null count every row once."""
    import torch
    who = "CovariationStatisticsSignificance"
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError("{}: samples is an integer >= 1: {!r}".format(who, samples))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= _MASK:
        raise ValueError("{}: seed is an integer in [0, 2^64): {!r}".format(who, seed))
    samples, seed = int(samples), int(seed)
    eng = _engine.get_engine()
    on_device = _device_engine(eng, _NULL_METHODS)
    rows_cap = 65535
    if on_device:
        from .device_calls import COVAR_NULL_MAX_ROWS as rows_cap
    if sequences is not None and len(sequences) > rows_cap:        # (before anything is computed; any other input: below)
        _refuse_rows(who, len(sequences))
    observed = CovariationStatistics(inputfile, fileformat, inputformat, sequences, names, alignment, pairs, statistic, correction, minspan,
                                     min_rows, min_stat, ignorewarn)
    R, L, minspan = observed.R, observed.L, int(minspan)
    if R > rows_cap:
        _refuse_rows(who, R)
    # one byte per character, as CovariationStatistics read them
    rows = np.frombuffer("".join(observed.sequences).encode("latin-1", "replace"), np.uint8).reshape(R, L)
    if on_device:
        d_rows = torch.from_numpy(rows.copy()).to(observed.device)
        null_ge, own_ge, null_max = eng.covariation_stat_null(d_rows, observed.pair_cols, observed.value, statistic, correction, minspan,
                                                              samples, seed)
    else:
        host = observed.cpu()
        null_ge, own_ge, null_max = (torch.from_numpy(np.ascontiguousarray(a)).to(observed.device) for a in _host_stat_null(
            rows, host.pair_cols.numpy().astype(np.int64), host.value.numpy(), statistic, correction, minspan, samples, seed))
    return StatisticsSignificanceResult(observed, samples, seed, samples * scope_cells(L, minspan), "device" if on_device else "host",
                                        null_ge, own_ge, null_max)


def _refuse_rows(who, R):
    if R > 65535:
        raise ValueError("{}: {} rows; the shuffle's sort keys hold at most 65,535".format(who, R))
    from .device_calls import COVAR_NULL_MAX_ROWS
    raise ValueError("{}: {} rows; the device shuffles at most COVAR_NULL_MAX_ROWS = {}".format(who, R, COVAR_NULL_MAX_ROWS))
