"""GPU tests of CovariationStatisticsSignificance(weights=) and its device entry (sq_covariation_wstat_null).

Exactly, against the existing device entries composed by the test: sample k of the null is formed as strings by shuffled() of
tests/covariation_null_checks.py and fed, with the same weights, to HipEngine.covariation_wstat_scan / covariation_wstat_pairs,
and the counts and the maxima are taken with torch -- the entry states that it forms the bits those entries form for the
shuffled rows.  Exactly against the unweighted entry for weights of 1.  Under the bracket of
tests/covariation_wstat_null_checks.py against the plain-Python reference, and against the result built under the
OracleEngine."""
import ctypes

import pytest

from squarna_amd.covariation_significance import scope_cells
from tests.covariation_checks import random_rows
from tests.covariation_null_checks import PLANTED, SEEDS, planted_rows, shuffled
from tests.covariation_stat_checks import CORRECTIONS, STATISTICS
from tests.covariation_wstat_checks import WEIGHTS, random_weights
from tests.covariation_wstat_null_checks import WeightedBracket, check_bracket, sharp_enough
from tests.test_hip_covariation_stat_null import COMBOS, engine, on_device, same, some_pairs

pytestmark = pytest.mark.gpu

ALI = "examples/ali_input.afa"


def consts():
    from squarna_amd import device_calls as dc
    assert {0.0, 2.0 ** -20, 1 / 3, 2048.0} <= set(WEIGHTS)                   # the pool random_weights draws from
    return dc.COVAR_STAT_TILE, dc.COVAR_STAT_WORD_CHUNK, dc.COVAR_STAT_MAX_BLOCKS, dc.COVAR_NULL_MAX_ROWS, dc.COVAR_WSTAT_NULL_LDS_BINS


def device_weights(weights):
    import torch
    return torch.tensor([float(w) for w in weights], dtype=torch.float64).cuda()


class Composed:
    """The weighted null of `rows` from the existing entries: per sample the weighted scan of the shuffled rows (every cell in
    scope: min_rows 0, no min_stat, room for all cells) and, for the observed pairs, their own cells of the shuffled rows."""

    def __init__(self, rows, weights, samples, seed):
        self.eng, self.L, self.samples, self.weights = engine(), len(rows[0]), samples, device_weights(weights)
        self.shuffled = [on_device(shuffled(rows, k, seed)) for k in range(samples)]
        self.scans = {}

    def values(self, statistic, correction, minspan):
        """Per sample the float64 tensor of the in-scope cells' C."""
        key = (statistic, correction, minspan)
        if key not in self.scans:
            cap = max(scope_cells(self.L, minspan), 1)
            self.scans[key] = [self.eng.covariation_wstat_scan(d, self.weights, statistic, correction, minspan=minspan, min_rows=0.0,
                                                               min_stat=None, cap=cap)[3] for d in self.shuffled]
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
                own = self.eng.covariation_wstat_pairs(self.shuffled[k], self.weights, pairs, statistic, correction)[2]
                own_ge += (own >= value).to(torch.int32)
        return null_ge, own_ge, null_max


def observed_scan(eng, d_rows, d_weights, statistic, correction, minspan, min_rows=2.0 ** -20):
    """(pairs int32[P, 2], value) of the weighted scan of the observed rows, sorted by (v, w)."""
    import torch
    L = int(d_rows.shape[1])
    flat, _, _, value, _ = eng.covariation_wstat_scan(d_rows, d_weights, statistic, correction, minspan=minspan, min_rows=min_rows,
                                                      min_stat=None, cap=max(scope_cells(L, minspan), 1))
    flat, order = torch.sort(flat)
    return torch.stack((flat // L, flat % L), 1).to(torch.int32).contiguous(), value[order].contiguous()


def observed_pairs(eng, d_rows, d_weights, statistic, correction, pairs):
    import torch
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)
    return d_pairs, eng.covariation_wstat_pairs(d_rows, d_weights, d_pairs, statistic, correction)[2]


@pytest.mark.parametrize("R", [1, 63, 64, 65, "chunk+1"])
def test_null_equals_the_composed_entries_whatever_the_batch(R):
    tile, chunk = consts()[:2]
    R = 64 * chunk + 1 if R == "chunk+1" else R
    eng, K, minspan = engine(), 3, 4
    for L in (1, 2, tile - 1, tile, tile + 1, 3 * tile + 1):
        rows = random_rows(1000 * R + L, R, L, "ACGU-" if L % 2 else "ACGUacgutT-.~N&")
        weights = random_weights(1000 * R + L, R)
        d_rows, d_weights = on_device(rows), device_weights(weights)
        for at, seed in enumerate(SEEDS):
            composed = Composed(rows, weights, K, seed)
            for statistic, correction in COMBOS[at::len(SEEDS)]:               # every statistic with every correction over the seeds
                what = (R, L, statistic, correction, seed)
                pairs, value = observed_scan(eng, d_rows, d_weights, statistic, correction, minspan)
                exp = composed.null(statistic, correction, minspan, pairs, value)
                for batch in (1, 2, 3):
                    same(eng.covariation_wstat_null(d_rows, d_weights, pairs, value, statistic, correction, minspan, K, seed, batch=batch), exp,
                         what + (batch,))
                assert (exp[1] <= K).all() and (L < 6 or R < 63 or (exp[0].max() > 0 and exp[2].max() > float("-inf")))
                pairs, value = observed_pairs(eng, d_rows, d_weights, statistic, correction, some_pairs(R + L, L))
                exp = composed.null(statistic, correction, minspan, pairs, value)
                same(eng.covariation_wstat_null(d_rows, d_weights, pairs, value, statistic, correction, minspan, K, seed), exp, what + ("pairs",))
                same(eng.covariation_wstat_null(d_rows, d_weights, pairs, value, statistic, correction, minspan, K, seed, batch=2), exp,
                     what + ("pairs", 2))


@pytest.mark.parametrize("statistic,correction", COMBOS)
def test_every_statistic_and_correction_at_every_seed(statistic, correction):
    """The rotation of the test above, closed: each statistic with each correction at each seed, at one multi-tile shape."""
    tile = consts()[0]
    eng, K, R, L = engine(), 3, 65, 2 * tile + 5
    rows, weights = random_rows(77, R, L, "ACGU-"), random_weights(77, R)
    d_rows, d_weights = on_device(rows), device_weights(weights)
    pairs, value = observed_scan(eng, d_rows, d_weights, statistic, correction, 4)
    for seed in SEEDS:
        exp = Composed(rows, weights, K, seed).null(statistic, correction, 4, pairs, value)
        same(eng.covariation_wstat_null(d_rows, d_weights, pairs, value, statistic, correction, 4, K, seed, batch=2), exp,
             (statistic, correction, seed))


def test_weights_of_one_give_the_unweighted_entry_bit_for_bit():
    import torch
    tile, chunk = consts()[:2]
    eng, K = engine(), 3
    for R, L in ((65, 2 * tile + 5), (64 * chunk + 1, tile + 1), (9, 20)):
        rows = random_rows(R + L, R, L, "ACGU-")
        d_rows, ones = on_device(rows), torch.ones(R, dtype=torch.float64, device="cuda")
        for at, (statistic, correction) in enumerate(COMBOS):
            seed, minspan = SEEDS[at % len(SEEDS)], (4, 1)[at % 2]
            pairs, value = observed_scan(eng, d_rows, ones, statistic, correction, minspan)
            plain = eng.covariation_stat_null(d_rows, pairs, value, statistic, correction, minspan, K, seed)
            same(eng.covariation_wstat_null(d_rows, ones, pairs, value, statistic, correction, minspan, K, seed), plain, (R, L, statistic, correction))
            assert int(plain[0].max()) > 0


def test_more_tiles_than_blocks():
    """R = 3, L = 64 tiles + 1: 2145 tiles for at most 2048 blocks of the one sample, so the first blocks take a second tile."""
    tile, _, max_blocks = consts()[:3]
    L = tile * 64 + 1
    assert (L + tile - 1) // tile * ((L + tile - 1) // tile + 1) // 2 > max_blocks
    rows, weights = random_rows(64, 3, L, "ACGU-", helices=0), [1 / 3, 1.0, 0.25]
    eng, d_rows, d_weights, composed = engine(), on_device(rows), device_weights(weights), Composed(rows, weights, 1, 8)
    given = [(0, L - 1), (5, 9), (L - 5, L - 1), (tile, 40 * tile), (3, 5)] + some_pairs(3, L, 65)
    for pairs, value in (observed_pairs(eng, d_rows, d_weights, "gt", "apc", given), observed_scan(eng, d_rows, d_weights, "gt", "apc", 4)):
        exp = composed.null("gt", "apc", 4, pairs, value)
        assert exp[0].max() > 0 and exp[0].min() < scope_cells(L, 4)
        same(eng.covariation_wstat_null(d_rows, d_weights, pairs, value, "gt", "apc", 4, 1, 8), exp, int(value.numel()))


def test_more_observed_values_than_bins_in_lds_and_none():
    """The scan keeps the lowest COVAR_WSTAT_NULL_LDS_BINS thresholds and bins in LDS: with more distinct observed values the
    null cells must fall on both sides of that boundary, and the counts stay exact.  Without an observed pair (P = U = 0) the
    entry still gives the samples' maxima."""
    import torch
    tile, lds_bins = consts()[0], consts()[4]
    R, L, K, seed = 65, 3 * tile + 1, 2, 5
    rows, weights = random_rows(12, R, L, "ACGU-"), random_weights(12, R)
    eng, d_rows, d_weights, composed = engine(), on_device(rows), device_weights(weights), Composed(rows, weights, K, seed)
    pairs, value = observed_scan(eng, d_rows, d_weights, "gt", "apc", 4)
    thresholds = torch.unique(value)
    assert thresholds.numel() > lds_bins + 100
    cells = torch.cat(composed.values("gt", "apc", 4))
    bins = torch.searchsorted(thresholds, cells, right=True)                 # the thresholds <= C
    assert (bins < lds_bins).sum() > 100 and (bins >= lds_bins).sum() > 100
    exp = composed.null("gt", "apc", 4, pairs, value)
    for batch in (1, 2):
        same(eng.covariation_wstat_null(d_rows, d_weights, pairs, value, "gt", "apc", 4, K, seed, batch=batch), exp, batch)
    nothing = (torch.empty((0, 2), dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.float64, device="cuda"))
    got = eng.covariation_wstat_null(d_rows, d_weights, *nothing, "gt", "apc", 4, K, seed)
    same(got, composed.null("gt", "apc", 4, *nothing), "P = 0")
    assert got[0].numel() == 0 and torch.equal(got[2], exp[2])


def direct(rows, weights, pairs, value, statistic, correction, minspan, K, seed, batch):
    """sq_covariation_wstat_null itself: (return code, hist, own_ge, null_max, out) with the outputs pre-filled with -7."""
    import torch
    from squarna_amd import _lib
    lib = _lib.load()
    d_rows, d_weights = on_device(rows), device_weights(weights)
    R, L, P = len(rows), len(rows[0]), len(pairs)
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)
    d_value = torch.tensor(value, dtype=torch.float64, device="cuda")
    thr = torch.unique(d_value)
    U = int(thr.numel())
    nbytes = lib.sq_covariation_wstat_null_scratch(R, L, batch)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    hist, own, out = (torch.full((n,), -7, dtype=dt, device="cuda") for n, dt in ((U + 1, torch.int64), (P, torch.int32), (2, torch.int64)))
    null_max = torch.full((K,), -7.0, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else None)
    rc = lib.sq_covariation_wstat_null(ptr(d_rows), R, L, STATISTICS.index(statistic), CORRECTIONS.index(correction), minspan, ptr(d_pairs),
                                       ptr(d_value), P, ptr(thr), U, K, seed, batch, ptr(scratch), nbytes, ptr(hist), ptr(own), ptr(null_max),
                                       ptr(out), None, ptr(d_weights))
    torch.cuda.synchronize()
    return rc, hist, own, null_max, out


def test_histogram_total_repeatability_a_bad_pair_and_a_bad_weight():
    import torch
    tile = consts()[0]
    R, L, K, seed = 70, 2 * tile + 3, 5, SEEDS[2]
    rows, weights = random_rows(9, R, L, "ACGU-"), random_weights(9, R)
    eng, d_rows, d_weights = engine(), on_device(rows), device_weights(weights)
    for statistic, correction, minspan in (("gt", "apc", 4), ("mi", None, 1), ("chi", "asc", L)):
        pairs, value = observed_scan(eng, d_rows, d_weights, statistic, correction, 1)
        a = eng.covariation_wstat_null(d_rows, d_weights, pairs, value, statistic, correction, minspan, K, seed, batch=2)
        b = eng.covariation_wstat_null(d_rows, d_weights, pairs, value, statistic, correction, minspan, K, seed, batch=2)
        for x, y in zip(a, b):                                                  # two calls give the same bits
            assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
        null_ge, own_ge, null_max = a
        order = torch.sort(value)[1]
        assert (null_ge[order][1:] <= null_ge[order][:-1]).all() and (own_ge <= K).all() and (own_ge >= 0).all()
        assert (null_ge <= K * scope_cells(L, minspan)).all() and not torch.isnan(null_max).any()
        rc, hist, own, most, out = direct(rows, weights, pairs.tolist(), value.tolist(), statistic, correction, minspan, K, seed, 3)
        assert rc == 0 and out.tolist() == [0, 0] and int(hist.sum()) == K * scope_cells(L, minspan) and (hist >= 0).all()
        assert torch.equal(own, own_ge) and torch.equal(most, null_max)
        if minspan >= L:                                                        # no cell in scope
            assert most.tolist() == [float("-inf")] * K and int(null_ge.sum()) == 0
    # a pair that is no pair: status 2, it counts nothing, every other pair is right
    good = some_pairs(4, L, 40)
    value = observed_pairs(eng, d_rows, d_weights, "gt", "apc", good)[1].tolist()
    rc, hist, own, most, out = direct(rows, weights, good, value, "gt", "apc", 4, K, seed, 2)
    assert rc == 0 and out.tolist() == [0, 0]
    for bad in ((5, 5), (7, 3), (-1, 4), (3, L)):
        pairs = good[:11] + [bad] + good[11:]
        rc, hist2, own2, most2, out2 = direct(rows, weights, pairs, value[:11] + [-1e300] + value[11:], "gt", "apc", 4, K, seed, 2)
        assert rc == 0 and out2.tolist() == [0, 2] and int(own2[11]) == 0, bad
        assert own2.tolist()[:11] + own2.tolist()[12:] == own.tolist() and torch.equal(most2, most) and int(hist2.sum()) == int(hist.sum())
        with pytest.raises(RuntimeError, match="sq_covariation_wstat_null: a pair is not 0 <= v < w < %d columns" % L):
            eng.covariation_wstat_null(d_rows, d_weights, torch.tensor(pairs, dtype=torch.int32, device="cuda"),
                                       torch.tensor(value[:11] + [0.0] + value[11:], dtype=torch.float64, device="cuda"), "gt", "apc", 4, K, seed)
    # a weight that is no weight: status 3 (above a bad pair's 2), it counts as 0
    for bad in (float("nan"), float("inf"), -1.0, 2048.5):
        spoiled = weights[:4] + [bad] + weights[5:]
        rc, _, own3, most3, out3 = direct(rows, spoiled, good[:11] + [(5, 5)], value[:11] + [0.0], "gt", "apc", 4, K, seed, 2)
        zeroed = direct(rows, weights[:4] + [0.0] + weights[5:], good[:11], value[:11], "gt", "apc", 4, K, seed, 2)
        assert rc == 0 and out3.tolist() == [0, 3] and own3.tolist()[:11] == zeroed[2].tolist() and torch.equal(most3, zeroed[3]), bad
        with pytest.raises(RuntimeError, match="sq_covariation_wstat_null: a weight is not a finite number"):
            eng.covariation_wstat_null(d_rows, device_weights(spoiled), torch.tensor(good, dtype=torch.int32, device="cuda"),
                                       torch.tensor(value, dtype=torch.float64, device="cuda"), "gt", "apc", 4, K, seed)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib, CovariationStatisticsSignificance
    lib = _lib.load()
    cap, chunk = consts()[3], consts()[1]
    R, L, P, U, K, batch = 9, 20, 3, 2, 4, 2
    scratch_of = lib.sq_covariation_wstat_null_scratch
    assert scratch_of(0, 5, 1) == 0 and scratch_of(5, 0, 1) == 0 and scratch_of(5, 5, 0) == 0
    nbytes = scratch_of(R, L, batch)
    assert nbytes == lib.sq_covariation_stat_null_scratch(R, L, batch) + 64 * chunk * 4        # and one chunk of rows of q
    fill = lambda dt, n: torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda")
    bufs = [fill(dt, n) for dt, n in ((torch.uint8, R * L), (torch.int32, 2 * P), (torch.float64, P), (torch.float64, U),
                                      (torch.int64, scratch_of(cap + 1, L, batch) // 8), (torch.int64, U + 1), (torch.int32, P),
                                      (torch.float64, K), (torch.int64, 2), (torch.float64, cap + 1))]
    rows, pairs, value, thr, scratch, hist, own, null_max, out, weights = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    good = dict(rows=rows, R=R, L=L, stat=1, corr=1, minspan=4, pairs=pairs, value=value, P=P, thr=thr, U=U, K=K, seed=5, batch=batch,
                scratch=scratch, nbytes=nbytes, hist=hist, own=own, null_max=null_max, out=out, stream=None, weights=weights)
    order = ("rows", "R", "L", "stat", "corr", "minspan", "pairs", "value", "P", "thr", "U", "K", "seed", "batch", "scratch", "nbytes", "hist",
             "own", "null_max", "out", "stream", "weights")
    for key, bad in (("rows", None), ("weights", None), ("pairs", None), ("value", None), ("thr", None), ("scratch", None), ("hist", None),
                     ("own", None), ("null_max", None), ("out", None), ("R", 0), ("L", 0), ("K", 0), ("K", -1), ("batch", 0), ("batch", 65536),
                     ("minspan", -1), ("P", -1), ("U", -1), ("stat", -1), ("stat", 3), ("corr", -1), ("corr", 3), ("nbytes", nbytes - 8),
                     ("R", cap + 1)):
        args = dict(good, **{key: bad})
        if key == "R" and bad > cap:
            args["nbytes"] = scratch_of(bad, L, batch)                       # (large enough: the row cap is what refuses)
        assert lib.sq_covariation_wstat_null(*(args[k] for k in order)) == -1, key
        msg = lib.sq_last_error()
        assert msg.startswith(b"sq_covariation_wstat_null: "), msg
        assert (b"scratch" in msg) == (key == "nbytes") and ((b"%d rows" % cap) in msg) == (key == "R" and bad > cap), (key, msg)
    torch.cuda.synchronize()
    for t in bufs:                                                           # nothing was launched, cleared or written
        assert (t == (249 if t.dtype == torch.uint8 else -7)).all()
    with pytest.raises(ValueError, match="COVAR_NULL_MAX_ROWS = %d" % cap):
        CovariationStatisticsSignificance(sequences=["ACGU"] * (cap + 1), weights=[1.0] * (cap + 1), samples=1)


def test_null_under_the_bracket_of_the_plain_python_reference():
    """The planted-helix alignment with random_weights(1, R): rows of weight 0, 2^-20, 1 / 3 and 2048 among them.  Condition (on
    the reference alone, before the device result is looked at): the uncertain share of the pooled counts is at most 1 % and at
    least 90 % of the pairs have lo == hi.  On the reference alone the uncertain share was 0 of about 5e6 for every statistic and
    correction, and every pair had lo == hi."""
    rows, _ = planted_rows()
    weights = random_weights(1, len(rows))
    assert {0.0, 2.0 ** -20, 1 / 3, 2048.0} <= set(weights)
    K, seed, minspan = 4, PLANTED["seed"], 4
    eng, d_rows, d_weights = engine(), on_device(rows), device_weights(weights)
    for statistic, correction in COMBOS:
        bracket = WeightedBracket(rows, weights, statistic, correction, minspan, K, seed)
        pairs, value = observed_scan(eng, d_rows, d_weights, statistic, correction, minspan)
        host_pairs = [tuple(p) for p in pairs.tolist()]
        pooled = bracket.table(host_pairs)[0]
        print(statistic, correction, "pairs", len(pooled), "uncertain", sum(hi - lo for lo, hi in pooled), "of", sum(hi for lo, hi in pooled),
              "exact pairs", sum(lo == hi for lo, hi in pooled))
        assert len(pooled) > 1000 and sharp_enough(pooled), (statistic, correction)
        got = eng.covariation_wstat_null(d_rows, d_weights, pairs, value, statistic, correction, minspan, K, seed)
        check_bracket(bracket, host_pairs, got[0].tolist(), got[1].tolist(), got[2].tolist(), (statistic, correction))


def test_the_public_call_with_row_identity_weights_against_the_cpu_built_result():
    """CovariationStatisticsSignificance(weights=RowIdentity(...).weights()) on the example alignment: formed on the device from
    the device's weights, and equal to the result built under the OracleEngine from the same weights within the bracket."""
    import torch
    from squarna_amd import CovariationStatistics, CovariationStatisticsSignificance, RowIdentity, engine as E
    from tests.oracle_engine import OracleEngine
    weights = RowIdentity(inputfile=ALI).weights()
    assert weights.is_cuda and weights.dtype == torch.float64 and float(weights.min()) < 1.0
    K, seed = 4, 11
    res = CovariationStatisticsSignificance(inputfile=ALI, weights=weights, samples=K, seed=seed)
    with E.use_engine(OracleEngine()):
        host = CovariationStatisticsSignificance(inputfile=ALI, weights=weights.cpu(), samples=K, seed=seed)
    assert res.source == "device" and res.device.type == "cuda" and res.observed.source == "device" and host.source == "host"
    assert all(t.is_cuda for t in (res.null_ge, res.own_ge, res.null_max, res.weights)) and res.weights.data_ptr() == weights.data_ptr()
    assert [t.dtype for t in (res.null_ge, res.own_ge, res.null_max)] == [torch.int64, torch.int32, torch.float64]
    assert (res.samples, res.seed, res.null_cells, len(res)) == (host.samples, host.seed, host.null_cells, len(host)) and len(res) > 100
    observed = CovariationStatistics(inputfile=ALI, weights=weights)
    for key in ("pair_cols", "joint", "raw", "value", "col_mean", "mean_all", "weights"):     # .observed is the weighted statistics' result
        assert torch.equal(getattr(res.observed, key), getattr(observed, key)), key
    pairs = [tuple(p) for p in res.observed.pair_cols.tolist()]
    assert pairs == [tuple(p) for p in host.observed.pair_cols.tolist()]
    bracket = WeightedBracket(res.observed.sequences, weights.tolist(), "gt", "apc", 4, K, seed)
    pooled = bracket.table(pairs)[0]
    for r in (res, host):
        check_bracket(bracket, pairs, r.null_ge.tolist(), r.own_ge.tolist(), r.null_max.tolist(), r.source)
    sure = [k for k, (lo, hi) in enumerate(pooled) if lo == hi]
    assert len(sure) * 2 > len(pairs) and res.null_ge[sure].tolist() == host.null_ge[sure].tolist()
    assert res.evalue().is_cuda and res.significant().is_cuda and res.to_matrix().is_cuda
    assert res.cpu().null_ge.tolist() == res.null_ge.tolist() and res.cpu().weights.device.type == "cpu"
