"""GPU tests of CovariationStatisticsSignificance() and its device entry (sq_covariation_stat_null).

Exactly, against the existing device entries composed by the test: sample k of the null is formed as strings by shuffled() of
tests/covariation_null_checks.py and fed to HipEngine.covariation_stat_scan / covariation_stat_pairs, and the counts and the
maxima are taken with torch -- the entry states that it forms the bits those entries form for the shuffled alignment.  Under the
bracket of tests/covariation_stat_null_checks.py against the plain-Python reference, and against the result built under the
OracleEngine."""
import ctypes
import random

import numpy as np
import pytest

from squarna_amd.covariation_significance import scope_cells
from tests.covariation_checks import random_rows
from tests.covariation_null_checks import PLANTED, SEEDS, planted_rows, shuffled
from tests.covariation_stat_checks import CORRECTIONS, STATISTICS
from tests.covariation_stat_null_checks import Bracket, check_bracket, sharp_enough

pytestmark = pytest.mark.gpu

COMBOS = [(s, c) for s in STATISTICS for c in CORRECTIONS]


def consts():
    from squarna_amd import device_calls as dc
    return dc.COVAR_STAT_TILE, dc.COVAR_STAT_WORD_CHUNK, dc.COVAR_STAT_MAX_BLOCKS, dc.COVAR_NULL_MAX_ROWS, dc.COVAR_STAT_NULL_LDS_BINS


def engine():
    from squarna_amd.engine import HipEngine
    return HipEngine()


def on_device(rows):
    import torch
    return torch.from_numpy(np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), len(rows[0])).copy()).cuda()


def some_pairs(seed, L, many=70):
    """`many` pairs v < w of L columns in any order, with repeats and with pairs below every minspan; none when L == 1."""
    rng = random.Random(seed)
    out = []
    while L > 1 and len(out) < many:
        v, w = sorted(rng.sample(range(L), 2))
        out += [(v, w)] * rng.choice((1, 1, 2))
    return out[:many]


class Composed:
    """The null of `rows` from the existing entries: per sample the scan of the shuffled rows (every cell in scope: min_rows 0,
    no min_stat) and, for the observed pairs, their own cells of the shuffled rows."""

    def __init__(self, rows, samples, seed):
        self.eng, self.L, self.samples = engine(), len(rows[0]), samples
        self.shuffled = [on_device(shuffled(rows, k, seed)) for k in range(samples)]
        self.scans = {}

    def values(self, statistic, correction, minspan):
        """Per sample the float64 tensor of the in-scope cells' C."""
        key = (statistic, correction, minspan)
        if key not in self.scans:
            cap = max(scope_cells(self.L, minspan), 1)
            self.scans[key] = [self.eng.covariation_stat_scan(d, statistic, correction, minspan=minspan, min_rows=0, min_stat=None, cap=cap)[3]
                               for d in self.shuffled]
            assert all(v.numel() == scope_cells(self.L, minspan) for v in self.scans[key])
        return self.scans[key]

    def null(self, statistic, correction, minspan, pairs, value):
        """(null_ge int64[P], own_ge int32[P], null_max float64[K]) for observed device tensors pairs int32[P, 2], value."""
        import torch
        P = int(value.numel())
        null_ge, own_ge = torch.zeros(P, dtype=torch.int64, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
        null_max = torch.full((self.samples,), float("-inf"), dtype=torch.float64, device="cuda")
        for k, cells in enumerate(self.values(statistic, correction, minspan)):
            null_ge += (cells.numel() - torch.searchsorted(torch.sort(cells)[0], value)) if P else 0      # the cells >= value[p]
            if cells.numel():
                null_max[k] = cells.max()
            if P:
                own = self.eng.covariation_stat_pairs(self.shuffled[k], pairs, statistic, correction)[2]
                own_ge += (own >= value).to(torch.int32)
        return null_ge, own_ge, null_max


def observed_scan(eng, d_rows, statistic, correction, minspan, min_rows=1):
    """(pairs int32[P, 2], value) of the scan of the observed rows, sorted by (v, w)."""
    import torch
    L = int(d_rows.shape[1])
    flat, _, _, value, _ = eng.covariation_stat_scan(d_rows, statistic, correction, minspan=minspan, min_rows=min_rows, min_stat=None,
                                                     cap=max(scope_cells(L, minspan), 1))
    flat, order = torch.sort(flat)
    return torch.stack((flat // L, flat % L), 1).to(torch.int32).contiguous(), value[order].contiguous()


def observed_pairs(eng, d_rows, statistic, correction, pairs):
    import torch
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)
    return d_pairs, eng.covariation_stat_pairs(d_rows, d_pairs, statistic, correction)[2]


def same(got, exp, what):
    import torch
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.float64] and all(t.is_cuda for t in got), what
    for name, g, e in zip(("null_ge", "own_ge", "null_max"), got, exp):
        assert g.shape == e.shape and torch.equal(g, e), (what, name, g.tolist()[:8], e.tolist()[:8])


@pytest.mark.parametrize("R", [1, 63, 64, 65, "chunk+1"])
def test_null_equals_the_composed_entries_whatever_the_batch(R):
    tile, chunk = consts()[:2]
    R = 64 * chunk + 1 if R == "chunk+1" else R
    eng, K, minspan = engine(), 3, 4
    for L in (1, 2, tile - 1, tile, tile + 1, 3 * tile + 1):
        rows = random_rows(1000 * R + L, R, L, "ACGU-" if L % 2 else "ACGUacgutT-.~N&")
        d_rows = on_device(rows)
        for at, seed in enumerate(SEEDS):
            composed = Composed(rows, K, seed)
            for statistic, correction in COMBOS[at::len(SEEDS)]:               # every statistic with every correction over the seeds
                what = (R, L, statistic, correction, seed)
                pairs, value = observed_scan(eng, d_rows, statistic, correction, minspan)
                exp = composed.null(statistic, correction, minspan, pairs, value)
                for batch in (1, 2, 3):
                    same(eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, minspan, K, seed, batch=batch), exp, what + (batch,))
                assert (exp[1] <= K).all() and (L < 6 or (exp[0].max() > 0 and exp[2].max() > float("-inf")))
                pairs, value = observed_pairs(eng, d_rows, statistic, correction, some_pairs(R + L, L))
                exp = composed.null(statistic, correction, minspan, pairs, value)
                same(eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, minspan, K, seed), exp, what + ("pairs",))
                same(eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, minspan, K, seed, batch=2), exp, what + ("pairs", 2))


@pytest.mark.parametrize("statistic,correction", COMBOS)
def test_every_statistic_and_correction_at_every_seed(statistic, correction):
    """The rotation of the test above, closed: each statistic with each correction at each seed, at one multi-tile shape."""
    tile = consts()[0]
    eng, K, R, L = engine(), 3, 65, 2 * tile + 5
    rows = random_rows(77, R, L, "ACGU-")
    d_rows = on_device(rows)
    pairs, value = observed_scan(eng, d_rows, statistic, correction, 4)
    for seed in SEEDS:
        exp = Composed(rows, K, seed).null(statistic, correction, 4, pairs, value)
        same(eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, 4, K, seed, batch=2), exp, (statistic, correction, seed))


def test_more_tiles_than_blocks():
    """R = 3, L = 64 tiles + 1: 2145 tiles for at most 2048 blocks of the one sample, so the first blocks take a second tile."""
    tile, _, max_blocks = consts()[:3]
    L = tile * 64 + 1
    assert (L + tile - 1) // tile * ((L + tile - 1) // tile + 1) // 2 > max_blocks
    rows = random_rows(64, 3, L, "ACGU-", helices=0)
    eng, d_rows, composed = engine(), on_device(rows), Composed(rows, 1, 8)
    given = [(0, L - 1), (5, 9), (L - 5, L - 1), (tile, 40 * tile), (3, 5)] + some_pairs(3, L, 65)
    for pairs, value in (observed_pairs(eng, d_rows, "gt", "apc", given), observed_scan(eng, d_rows, "gt", "apc", 4)):
        exp = composed.null("gt", "apc", 4, pairs, value)
        assert exp[0].max() > 0 and exp[0].min() < scope_cells(L, 4)
        same(eng.covariation_stat_null(d_rows, pairs, value, "gt", "apc", 4, 1, 8), exp, int(value.numel()))


def test_more_observed_values_than_bins_in_lds():
    """The scan keeps the lowest COVAR_STAT_NULL_LDS_BINS thresholds and bins in LDS: with more distinct observed values the
    null cells must fall on both sides of that boundary, and the counts stay exact."""
    import torch
    tile, lds_bins = consts()[0], consts()[4]
    R, L, K, seed = 65, 3 * tile + 1, 2, 5
    rows = random_rows(12, R, L, "ACGU-")
    eng, d_rows, composed = engine(), on_device(rows), Composed(rows, K, seed)
    pairs, value = observed_scan(eng, d_rows, "gt", "apc", 4)
    thresholds = torch.unique(value)
    assert thresholds.numel() > lds_bins + 100
    cells = torch.cat(composed.values("gt", "apc", 4))
    bins = torch.searchsorted(thresholds, cells, right=True)                 # the thresholds <= C
    assert (bins < lds_bins).sum() > 100 and (bins >= lds_bins).sum() > 100
    exp = composed.null("gt", "apc", 4, pairs, value)
    for batch in (1, 2):
        same(eng.covariation_stat_null(d_rows, pairs, value, "gt", "apc", 4, K, seed, batch=batch), exp, batch)


@pytest.mark.parametrize("R", [65, 130])
def test_null_under_the_bracket_of_the_plain_python_reference(R):
    """Condition (on the reference alone, before the device result is looked at): the uncertain share of the pooled counts is
    at most 1 % and at least 90 % of the pairs have lo == hi.  With the numpy fallback and a wider band the uncertain share
    was 106 of 7.7e7 at R = 65 without a correction and 0 everywhere else; at R = 9 equal tables tie massively without a
    correction, which is why small R is covered by the exact tests above and not here."""
    tile = consts()[0]
    L, K, seed, minspan = 3 * tile + 1, 4, 9, 4
    rows = random_rows(500 + R, R, L, "ACGU-", helices=4)
    eng, d_rows = engine(), on_device(rows)
    for statistic, correction in COMBOS:
        bracket = Bracket(rows, statistic, correction, minspan, K, seed)
        pairs, value = observed_scan(eng, d_rows, statistic, correction, minspan)
        host_pairs = [tuple(p) for p in pairs.tolist()]
        pooled = bracket.table(host_pairs)[0]
        print(R, statistic, correction, "pairs", len(pooled), "uncertain", sum(hi - lo for lo, hi in pooled), "of", sum(hi for lo, hi in pooled),
              "exact pairs", sum(lo == hi for lo, hi in pooled))
        assert len(pooled) > 4000 and sharp_enough(pooled), (statistic, correction)
        got = eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, minspan, K, seed)
        check_bracket(bracket, host_pairs, got[0].tolist(), got[1].tolist(), got[2].tolist(), (R, statistic, correction))


def direct(rows, pairs, value, statistic, correction, minspan, K, seed, batch):
    """sq_covariation_stat_null itself: (return code, hist, own_ge, null_max, out) with the outputs pre-filled with -7."""
    import torch
    from squarna_amd import _lib
    lib = _lib.load()
    d_rows = on_device(rows)
    R, L, P = len(rows), len(rows[0]), len(pairs)
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)
    d_value = torch.tensor(value, dtype=torch.float64, device="cuda")
    thr = torch.unique(d_value)
    U = int(thr.numel())
    nbytes = lib.sq_covariation_stat_null_scratch(R, L, batch)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    hist, own, out = (torch.full((n,), -7, dtype=dt, device="cuda") for n, dt in ((U + 1, torch.int64), (P, torch.int32), (2, torch.int64)))
    null_max = torch.full((K,), -7.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)
    rc = lib.sq_covariation_stat_null(ptr(d_rows), R, L, STATISTICS.index(statistic), CORRECTIONS.index(correction), minspan, ptr(d_pairs),
                                      ptr(d_value), P, ptr(thr), U, K, seed, batch, ptr(scratch), nbytes, ptr(hist), ptr(own), ptr(null_max),
                                      ptr(out), None)
    torch.cuda.synchronize()
    return rc, hist, own, null_max, out


def test_histogram_total_monotony_repeatability_and_a_bad_pair():
    import torch
    tile = consts()[0]
    R, L, K, seed = 70, 2 * tile + 3, 5, SEEDS[2]
    rows = random_rows(9, R, L, "ACGU-")
    eng, d_rows = engine(), on_device(rows)
    for statistic, correction, minspan in (("gt", "apc", 4), ("mi", None, 1), ("chi", "asc", L)):
        pairs, value = observed_scan(eng, d_rows, statistic, correction, 1)
        a = eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, minspan, K, seed, batch=2)
        b = eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, minspan, K, seed, batch=2)
        for x, y in zip(a, b):                                                  # two calls give the same bits
            assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
        null_ge, own_ge, null_max = a
        order = torch.sort(value)[1]
        assert (null_ge[order][1:] <= null_ge[order][:-1]).all() and (own_ge <= K).all() and (own_ge >= 0).all()
        assert (null_ge <= K * scope_cells(L, minspan)).all() and not torch.isnan(null_max).any()
        rc, hist, own, most, out = direct(rows, pairs.tolist(), value.tolist(), statistic, correction, minspan, K, seed, 3)
        assert rc == 0 and out.tolist() == [0, 0] and int(hist.sum()) == K * scope_cells(L, minspan) and (hist >= 0).all()
        assert torch.equal(own, own_ge) and torch.equal(most, null_max)
        if minspan >= L:                                                        # no cell in scope
            assert most.tolist() == [float("-inf")] * K and int(null_ge.sum()) == 0
    # a pair that is no pair: status 2, it counts nothing, every other pair is right
    good = some_pairs(4, L, 40)
    value = observed_pairs(eng, d_rows, "gt", "apc", good)[1].tolist()
    rc, hist, own, most, out = direct(rows, good, value, "gt", "apc", 4, K, seed, 2)
    assert rc == 0 and out.tolist() == [0, 0]
    for bad in ((5, 5), (7, 3), (-1, 4), (3, L)):
        pairs = good[:11] + [bad] + good[11:]
        rc, hist2, own2, most2, out2 = direct(rows, pairs, value[:11] + [-1e300] + value[11:], "gt", "apc", 4, K, seed, 2)
        assert rc == 0 and out2.tolist() == [0, 2] and int(own2[11]) == 0, bad
        assert own2.tolist()[:11] + own2.tolist()[12:] == own.tolist() and torch.equal(most2, most) and int(hist2.sum()) == int(hist.sum())
        with pytest.raises(RuntimeError, match="sq_covariation_stat_null: a pair is not 0 <= v < w < %d columns" % L):
            eng.covariation_stat_null(d_rows, torch.tensor(pairs, dtype=torch.int32, device="cuda"),
                                      torch.tensor(value[:11] + [0.0] + value[11:], dtype=torch.float64, device="cuda"), "gt", "apc", 4, K, seed)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib, CovariationStatisticsSignificance
    lib = _lib.load()
    cap = consts()[3]
    R, L, P, U, K, batch = 9, 20, 3, 2, 4, 2
    scratch_of = lib.sq_covariation_stat_null_scratch
    assert scratch_of(0, 5, 1) == 0 and scratch_of(5, 0, 1) == 0 and scratch_of(5, 5, 0) == 0
    nbytes = scratch_of(R, L, batch)
    assert nbytes == batch * (5 * 1 * 64 + 1 * 64 + 21) * 8 + 184             # per sample planes, partials, means; 9 * 20 class bytes to 8
    fill = lambda dt, n: torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda")
    bufs = [fill(dt, n) for dt, n in ((torch.uint8, R * L), (torch.int32, 2 * P), (torch.float64, P), (torch.float64, U),
                                      (torch.int64, scratch_of(cap + 1, L, batch) // 8), (torch.int64, U + 1), (torch.int32, P),
                                      (torch.float64, K), (torch.int64, 2))]
    rows, pairs, value, thr, scratch, hist, own, null_max, out = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    good = dict(rows=rows, R=R, L=L, stat=1, corr=1, minspan=4, pairs=pairs, value=value, P=P, thr=thr, U=U, K=K, seed=5, batch=batch,
                scratch=scratch, nbytes=nbytes, hist=hist, own=own, null_max=null_max, out=out)
    order = ("rows", "R", "L", "stat", "corr", "minspan", "pairs", "value", "P", "thr", "U", "K", "seed", "batch", "scratch", "nbytes", "hist",
             "own", "null_max", "out")
    for key, bad in (("rows", None), ("pairs", None), ("value", None), ("thr", None), ("scratch", None), ("hist", None), ("own", None),
                     ("null_max", None), ("out", None), ("R", 0), ("L", 0), ("K", 0), ("K", -1), ("batch", 0), ("batch", 65536), ("minspan", -1),
                     ("P", -1), ("U", -1), ("stat", -1), ("stat", 3), ("corr", -1), ("corr", 3), ("nbytes", nbytes - 8), ("R", cap + 1)):
        args = dict(good, **{key: bad})
        if key == "R" and bad > cap:
            args["nbytes"] = scratch_of(bad, L, batch)                       # (large enough: the row cap is what refuses)
        assert lib.sq_covariation_stat_null(*(args[k] for k in order), None) == -1, key
        msg = lib.sq_last_error()
        assert msg.startswith(b"sq_covariation_stat_null: "), msg
        assert (b"scratch" in msg) == (key == "nbytes") and ((b"%d rows" % cap) in msg) == (key == "R" and bad > cap), (key, msg)
    torch.cuda.synchronize()
    for t in bufs:                                                           # nothing was launched, cleared or written
        assert (t == (249 if t.dtype == torch.uint8 else -7)).all()
    with pytest.raises(ValueError, match="COVAR_NULL_MAX_ROWS = %d" % cap):
        CovariationStatisticsSignificance(sequences=["ACGU"] * (cap + 1), samples=1)


def test_the_device_result_against_the_cpu_built_result_under_the_bracket():
    import torch
    from squarna_amd import CovariationStatistics, CovariationStatisticsSignificance, engine as E
    from tests.oracle_engine import OracleEngine
    rows, planted = planted_rows()
    K, seed = 6, PLANTED["seed"]
    res = CovariationStatisticsSignificance(sequences=rows, samples=K, seed=seed)
    with E.use_engine(OracleEngine()):
        host = CovariationStatisticsSignificance(sequences=rows, samples=K, seed=seed)
    assert res.source == "device" and res.device.type == "cuda" and res.observed.source == "device" and host.source == "host"
    assert (res.samples, res.seed, res.null_cells, len(res)) == (host.samples, host.seed, host.null_cells, len(host)) and len(res) > 1000
    observed = CovariationStatistics(sequences=rows)
    for key in ("pair_cols", "joint", "raw", "value", "col_mean", "mean_all"):  # .observed is CovariationStatistics' result, unchanged
        assert torch.equal(getattr(res.observed, key), getattr(observed, key)), key
    pairs = [tuple(p) for p in res.observed.pair_cols.tolist()]
    assert pairs == [tuple(p) for p in host.observed.pair_cols.tolist()]
    bracket = Bracket(rows, "gt", "apc", 4, K, seed)
    pooled, own = bracket.table(pairs)
    assert sharp_enough(pooled)
    for r in (res, host):
        assert [t.dtype for t in (r.null_ge, r.own_ge, r.null_max)] == [torch.int64, torch.int32, torch.float64]
        check_bracket(bracket, pairs, r.null_ge.tolist(), r.own_ge.tolist(), r.null_max.tolist(), r.source)
    sure = [k for k, (lo, hi) in enumerate(pooled) if lo == hi]
    assert res.null_ge[sure].tolist() == host.null_ge[sure].tolist()
    at = [pairs.index(p) for p in planted]
    assert res.evalue()[at].tolist() == [0.0] * len(at) and res.significant()[at].all() and res.significant().is_cuda
    null_ge, own_ge, null_max, value = (t.cpu().numpy() for t in (res.null_ge, res.own_ge, res.null_max, res.observed.value))
    max_ge = (null_max[None, :] >= value[:, None]).sum(1)
    for got, exp in ((res.evalue(), null_ge.astype(np.float64) / np.float64(K)), (res.pvalue(), (1 + own_ge).astype(np.float64) / np.float64(K + 1)),
                     (res.pvalue_max(), (1 + max_ge).astype(np.float64) / np.float64(K + 1))):
        assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), exp)
    assert res.to_matrix().is_cuda and torch.equal(res.to_matrix("value"), res.observed.to_matrix("value"))
    v, w = pairs[at[0]]
    assert res.of(v, w)["null_ge"] == 0 and res.of(v, w)["value"] == float(res.observed.value[at[0]])
    assert res.cpu().null_ge.tolist() == res.null_ge.tolist() and res.cpu().observed.device.type == "cpu"
