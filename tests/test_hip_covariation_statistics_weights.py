"""GPU tests of CovariationStatistics(weights=) and its two device entries (sq_covariation_wstat_scan,
sq_covariation_wstat_pairs) against the plain-Python reference of tests/covariation_wstat_checks.py, the device's own unweighted
entries (weights of 1 and integer weights: the same bits) and the result built under the OracleEngine.  Q and record sets are
compared exactly, raw, value and the means under the float bound derived in covariation_wstat_checks.py; records are compared
after sorting by flat index."""
import ctypes
import math
import random
from fractions import Fraction

import numpy as np
import pytest

from tests.covariation_checks import random_rows
from tests.covariation_stat_checks import BOUND, CORRECTIONS, DEFAULTS, EVERY_CELL, STATISTICS, check_means, check_records, columns
from tests.covariation_wstat_checks import ONE, joint_w, quantise, random_weights, raw_terms_w, reference
from tests.test_hip_covariation_statistics import device_rows, raw_pairs, raw_scan

pytestmark = pytest.mark.gpu

ALI = "examples/ali_input.afa"


def consts():
    from squarna_amd import device_calls as dc
    assert dc.COVAR_WSTAT_ONE == ONE
    return dc.COVAR_STAT_TILE, dc.COVAR_STAT_WORD_CHUNK, dc.COVAR_STAT_MAX_BLOCKS


def device_weights(weights):
    import torch
    return torch.tensor([float(w) for w in weights], dtype=torch.float64).cuda()


def wraw_scan(rows, weights, statistic="gt", correction="apc", cap=None, **thr):
    """HipEngine.covariation_wstat_scan as device tensors sorted by flat index: (flat, Q, raw, value, mean)."""
    import torch
    from squarna_amd.engine import HipEngine
    L = len(rows[0])
    flat, Q, raw, value, mean = HipEngine().covariation_wstat_scan(device_rows(rows), device_weights(weights), statistic, correction, cap=cap, **thr)
    assert all(t.is_cuda for t in (flat, Q, raw, value))
    assert (flat.dtype, Q.dtype, raw.dtype, value.dtype) == (torch.int64, torch.int64, torch.float64, torch.float64)
    assert tuple(Q.shape) == (int(flat.numel()), 16) and raw.shape == flat.shape == value.shape
    assert (mean is None) == (correction is None) and (mean is None or (mean.is_cuda and mean.dtype == torch.float64 and tuple(mean.shape) == (L + 1,)))
    order = torch.argsort(flat)
    flat = flat[order]
    assert int(flat.unique().numel()) == int(flat.numel())                   # no cell twice
    return flat, Q[order], raw[order], value[order], mean


def check_wscan(ref, rows, weights, statistic, correction, cap=None, **thr):
    L = len(rows[0])
    flat, Q, raw, value, mean = wraw_scan(rows, weights, statistic, correction, cap=cap, **thr)
    what = (len(rows), L, statistic, correction, thr)
    check_records(ref, statistic, correction, [(f // L, f % L) for f in flat.tolist()], Q.tolist(), raw.tolist(), value.tolist(),
                  ref.select(statistic, correction, **thr), what)
    if correction is not None:
        check_means(ref, statistic, mean[:L].tolist(), float(mean[L]), what)
    return flat, Q, raw, value, mean


def wraw_pairs(rows, weights, pairs, statistic="gt", correction="apc"):
    import torch
    from squarna_amd.engine import HipEngine
    Q, raw, value, mean = HipEngine().covariation_wstat_pairs(device_rows(rows), device_weights(weights),
                                                              torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).cuda(), statistic, correction)
    assert Q.is_cuda and raw.is_cuda and value.is_cuda and (Q.dtype, raw.dtype, value.dtype) == (torch.int64, torch.float64, torch.float64)
    assert tuple(Q.shape) == (len(pairs), 16) and tuple(raw.shape) == tuple(value.shape) == (len(pairs),)
    return Q, raw, value, mean


def with_both_ends(weights):
    """The drawn weights with a 0 and a 2048 among them where there is room."""
    weights = list(weights)
    if len(weights) > 2:
        weights[1], weights[-1] = 0.0, 2048.0
    return weights


@pytest.mark.parametrize("R", [1, 63, 64, 65, "chunk+1"])
def test_scan_and_pairs_against_the_reference(R):
    """Every cell (nothing thresholded) for every statistic and correction, the defaults for the default statistic, and 70
    given pairs: Q exactly, raw, value and the means under the bound."""
    tile, chunk, _ = consts()
    R = 64 * chunk + 1 if R == "chunk+1" else R
    rng = random.Random(R)
    for L in (1, 2, tile - 1, tile, tile + 1, 3 * tile + 1):
        rows, weights = random_rows(1000 * R + L, R, L), with_both_ends(random_weights(1000 * R + L, R))
        ref = reference(rows, weights)
        for s in STATISTICS:
            for c in CORRECTIONS:
                check_wscan(ref, rows, weights, s, c, **EVERY_CELL)
        check_wscan(ref, rows, weights, "gt", "apc", **DEFAULTS)
        pairs = [rng.choice(sorted(ref.n)) for _ in range(70)] if ref.n else []              # any order, repeats, any span
        for s, c in (("gt", "apc"), ("mi", "asc"), ("chi", None)):
            Q, raw, value, mean = wraw_pairs(rows, weights, pairs, s, c)
            check_records(ref, s, c, pairs, Q.tolist(), raw.tolist(), value.tolist(), [ref.record(s, c, v, w) for v, w in pairs], (R, L, s, c))
            if c is not None:
                check_means(ref, s, mean[:L].tolist(), float(mean[L]), (R, L, s, c, "pairs"))


def test_weights_of_one_and_integer_weights_give_the_bits_of_the_unweighted_entries():
    """R = 65, L = 3 tiles + 1.  All weights 1.0 against the device's unweighted entries on the same rows, and integer weights
    k[r] in 0..3 against them on the alignment with row r repeated k[r] times: Q = n * 2^20 and every float bit for bit."""
    import torch
    tile = consts()[0]
    L = 3 * tile + 1
    rows = random_rows(65097, 65, L, "ACGU-", helices=4)
    rng = random.Random(65)
    k = [rng.randrange(4) for _ in rows]
    repeated = [r for r, times in zip(rows, k) for _ in range(times)]
    for weights, plain_rows in (([1.0] * 65, rows), (k, repeated)):
        for s in STATISTICS:
            for c in CORRECTIONS:
                for thr in (EVERY_CELL, DEFAULTS):
                    flat, Q, raw, value, mean = wraw_scan(rows, weights, s, c, **thr)
                    p_flat, n, p_raw, p_value, p_mean = raw_scan(plain_rows, s, c, **thr)
                    assert torch.equal(flat, p_flat) and torch.equal(Q, n.long() * ONE) and int(flat.numel()) > 0, (s, c)
                    assert torch.equal(raw, p_raw) and torch.equal(value, p_value), (s, c)
                    assert mean is p_mean is None or torch.equal(mean, p_mean), (s, c)
                pairs = [(0, 1), (5, 20), (5, 20), (3, L - 1), (tile - 1, 2 * tile)]
                Q, raw, value, mean = wraw_pairs(rows, weights, pairs, s, c)
                n, p_raw, p_value, p_mean = raw_pairs(plain_rows, pairs, s, c)
                assert torch.equal(Q, n.long() * ONE) and torch.equal(raw, p_raw) and torch.equal(value, p_value), (s, c)
                assert mean is p_mean is None or torch.equal(mean, p_mean), (s, c)


def test_the_stage_flushes_inside_a_tile_and_the_call_is_repeated_once():
    """R = 5, L = 4 tiles, the columns alternate G / C, every weight is 0.5 and nothing is thresholded: every cell of every tile
    off the diagonal is a hit, so the stage flushes inside the tile.  With cap 100 the first call stores 100 records and counts
    them all; the second has room."""
    import torch
    tile = consts()[0]
    L = 4 * tile
    rows, weights = ["GC" * (L // 2)] * 5, [0.5] * 5
    ref = reference(rows, weights)
    exp = ref.select("gt", "apc", **EVERY_CELL)
    assert len(exp) == L * (L - 1) // 2 and exp[0][2][2 * 4 + 1] == 5 * ONE // 2 and sum(exp[0][2]) == 5 * ONE // 2 and exp[0][3:] == (0.0, 0.0)
    full = check_wscan(ref, rows, weights, "gt", "apc", **EVERY_CELL)
    assert int(full[0].numel()) == len(exp) and not full[2].any() and not full[3].any() and not full[4].any()       # conserved: exactly 0
    again = wraw_scan(rows, weights, "gt", "apc", cap=100, **EVERY_CELL)
    assert all(torch.equal(a, b) for a, b in zip(full, again))


def test_more_tiles_than_blocks():
    """R = 3, L = 64 tiles + 1, weights (1 / 3, 1, 0.25): 2145 tiles for at most 2048 blocks, so the first blocks take a second
    tile, and a column has 65 partial sums.  The reference is the plain-Python table and terms per distinct pair of column
    strings (R = 3: few), gathered with numpy; a column sum is math.fsum over the distinct strings of (their number) * S.  The
    bound is BOUND, as everywhere."""
    tile, _, max_blocks = consts()
    L = tile * 64 + 1
    assert (L + tile - 1) // tile * ((L + tile - 1) // tile + 1) // 2 > max_blocks
    rows, weights = random_rows(64, 3, L, "ACGU-", helices=0), [1 / 3, 1.0, 0.25]
    q = quantise(weights)
    cols = columns(rows)
    kinds = sorted(set(cols))
    K, kind = len(kinds), np.array([kinds.index(c) for c in cols])
    tables = [[joint_w(a, b, q) for b in kinds] for a in kinds]
    terms = [[raw_terms_w(tables[a][b], "gt") for b in range(K)] for a in range(K)]
    n = np.array(tables, dtype=np.int64)                                                         # [K, K, 16]
    S = np.array([[math.fsum(t) for t in row] for row in terms])
    scale = np.array([[math.fsum(abs(x) for x in t) for t in row] for row in terms])
    assert np.abs(S - S.T).max() <= BOUND * scale.max()                                          # (v, w) or (w, v): the same S
    mult = np.bincount(kind, minlength=K)
    mean_of_kind = [(math.fsum(int(mult[b]) * S[a, b] for b in range(K)) - S[a, a]) / (L - 1) for a in range(K)]
    mean = np.array(mean_of_kind)[kind]
    mean_all = math.fsum(int(mult[a]) * mean_of_kind[a] for a in range(K)) / L
    min_rows = 1.3                                                                               # 1 / 3 + 1 and more; no sum of q near it
    assert all(abs(Fraction(sum(q[r] for r in some), ONE) - Fraction(min_rows)) > Fraction(1, ONE) for some in
               ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)))
    flat, Q, raw, value, d_mean = wraw_scan(rows, weights, "gt", "apc", minspan=4, min_rows=min_rows, min_stat=None)
    bound = BOUND
    got_mean = d_mean.cpu().numpy()
    assert (np.abs(got_mean[:L] - mean) <= bound * mean).all() and abs(got_mean[L] - mean_all) <= bound * mean_all and mean_all > 0
    v, w = np.triu_indices(L, 4)
    keep = n[kind[v], kind[w]].sum(-1) >= min_rows * ONE
    v, w = v[keep], w[keep]
    assert len(v) > 100000 and (w == L - 1).any() and not keep.all()
    assert np.array_equal(flat.cpu().numpy(), v * L + w)
    assert np.array_equal(Q.cpu().numpy(), n[kind[v], kind[w]])
    assert (np.abs(raw.cpu().numpy() - S[kind[v], kind[w]]) <= bound * scale[kind[v], kind[w]]).all()
    term = mean[v] * mean[w] / mean_all
    assert (np.abs(value.cpu().numpy() - (S[kind[v], kind[w]] - term)) <= bound * (np.abs(S[kind[v], kind[w]]) + np.abs(term))).all()


def test_two_calls_give_the_same_bits_and_scan_and_pairs_the_same_records():
    import torch
    tile = consts()[0]
    L = 3 * tile + 1
    rows, weights = random_rows(5, 130, L, "ACGU-", helices=4), random_weights(5, 130)
    for s in STATISTICS:
        for c in CORRECTIONS:
            one, two = wraw_scan(rows, weights, s, c, **EVERY_CELL), wraw_scan(rows, weights, s, c, **EVERY_CELL)
            assert all(a is b is None or torch.equal(a, b) for a, b in zip(one, two)), (s, c)
            flat, Q, raw, value, mean = one
            pairs = torch.stack((flat // L, flat % L), 1).tolist()
            p_Q, p_raw, p_value, p_mean = wraw_pairs(rows, weights, pairs, s, c)
            assert torch.equal(p_Q, Q) and torch.equal(p_raw, raw) and torch.equal(p_value, value), (s, c)             # bit for bit
            assert mean is p_mean is None or torch.equal(mean, p_mean)
            if c is not None:                                                # the means: of every pair of columns, whatever the thresholds
                assert torch.equal(wraw_scan(rows, weights, s, c, minspan=tile + 3, min_rows=100.5, min_stat=1.0)[4], mean), (s, c)


def _raw(dtype_sizes):
    """Device buffers filled with a sentinel (249 in bytes, -7 otherwise) for direct calls of the entries."""
    import torch
    return [torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda") for dt, n in dtype_sizes]


def test_pairs_status_leaves_the_other_records_right_and_a_bad_weight_raises():
    import torch
    from squarna_amd import _lib, CovariationStatistics
    from squarna_amd.engine import HipEngine
    lib = _lib.load()
    rows, weights = random_rows(12, 9, 20), with_both_ends(random_weights(12, 9))
    ref = reference(rows, weights)
    pairs = [(2, 11), (3, 20), (0, 19)]                                      # the middle one: w = L
    d_rows, d_weights, d_pairs = device_rows(rows), device_weights(weights), torch.tensor(pairs, dtype=torch.int32).cuda()
    nbytes = lib.sq_covariation_wstat_scratch(9, 20)
    scratch, mean, joint, raw, value, out = _raw([(torch.int64, nbytes // 8), (torch.float64, 21), (torch.int64, 48), (torch.float64, 3),
                                                  (torch.float64, 3), (torch.int64, 2)])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.sq_covariation_wstat_pairs(p(d_rows), 9, 20, p(d_weights), 1, 1, p(d_pairs), 3, p(scratch), nbytes, p(mean), p(joint), p(raw),
                                          p(value), p(out), None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 2]
    assert joint.view(3, 16)[1].tolist() == [0] * 16 and raw[1] == 0 and value[1] == 0
    keep = [0, 2]
    check_records(ref, "gt", "apc", [pairs[k] for k in keep], joint.view(3, 16)[keep].tolist(), raw[keep].tolist(), value[keep].tolist(),
                  [ref.record("gt", "apc", *pairs[k]) for k in keep])
    check_means(ref, "gt", mean[:20].tolist(), float(mean[20]))
    with pytest.raises(RuntimeError, match="a pair is not"):
        CovariationStatistics(sequences=rows, weights=weights, pairs=pairs)
    for bad in ([(4, 4)], [(-1, 3)], [(9, 2)]):
        with pytest.raises(RuntimeError, match="a pair is not"):
            wraw_pairs(rows, weights, bad)
    for bad in (float("nan"), float("inf"), -1.0, 2048.5):                   # handed to the engine directly: status 3
        spoiled = weights[:4] + [bad] + weights[5:]
        with pytest.raises(RuntimeError, match="a weight is not"):
            HipEngine().covariation_wstat_scan(d_rows, device_weights(spoiled))
        with pytest.raises(RuntimeError, match="a weight is not"):
            wraw_pairs(rows, spoiled, [(2, 11)])


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib, device_calls as dc
    lib = _lib.load()
    R, L, cap = 9, 20, 8
    assert lib.sq_covariation_wstat_scratch(0, 5) == 0 and lib.sq_covariation_wstat_scratch(5, 0) == 0
    nbytes = lib.sq_covariation_wstat_scratch(R, L)
    assert nbytes == lib.sq_covariation_stat_scratch(R, L) + 64 * consts()[1] * 4                 # and one chunk of rows of q
    sizes = [(torch.uint8, R * L), (torch.float64, R), (torch.int64, nbytes // 8), (torch.float64, L + 1), (torch.int64, cap),
             (torch.int64, cap * 16), (torch.float64, cap), (torch.float64, cap), (torch.int64, 2), (torch.int32, 6)]
    bufs = _raw(sizes)
    rows, weights, scratch, mean, flat, joint, raw, value, out, pairs = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    scan, lookup = lib.sq_covariation_wstat_scan, lib.sq_covariation_wstat_pairs
    good = dict(rows=rows, R=R, L=L, weights=weights, stat=1, corr=1, minspan=4, min_rows=1.0, min_stat=0.5, scratch=scratch, nbytes=nbytes,
                mean=mean, flat=flat, joint=joint, raw=raw, value=value, cap=cap, out=out)
    order = ("rows", "R", "L", "weights", "stat", "corr", "minspan", "min_rows", "min_stat", "scratch", "nbytes", "mean", "flat", "joint", "raw",
             "value", "cap", "out")
    too_many = dc.COVAR_WSTAT_MAX_ROWS + 1
    for key, bad in (("rows", None), ("weights", None), ("scratch", None), ("mean", None), ("flat", None), ("joint", None), ("raw", None),
                     ("value", None), ("out", None), ("R", 0), ("L", 0), ("nbytes", nbytes - 8), ("stat", -1), ("stat", 3), ("corr", -1),
                     ("corr", 3), ("minspan", -1), ("min_rows", -0.5), ("min_rows", float("nan")), ("min_stat", float("nan")), ("cap", -1),
                     ("R", too_many)):
        args = dict(good, **{key: bad})
        if key == "R" and bad == too_many:                                   # (with room enough for that many rows, were they taken)
            args["nbytes"] = lib.sq_covariation_wstat_scratch(too_many, L)
        assert scan(*(args[k] for k in order), None) == -1, key
        assert (b"scratch" in lib.sq_last_error()) == (key == "nbytes"), key
        assert (b"2^22 rows" in lib.sq_last_error()) == (bad == too_many), key
    good = dict(rows=rows, R=R, L=L, weights=weights, stat=1, corr=1, pairs=pairs, P=3, scratch=scratch, nbytes=nbytes, mean=mean, joint=joint,
                raw=raw, value=value, out=out)
    order = ("rows", "R", "L", "weights", "stat", "corr", "pairs", "P", "scratch", "nbytes", "mean", "joint", "raw", "value", "out")
    for key, bad in (("rows", None), ("weights", None), ("pairs", None), ("scratch", None), ("mean", None), ("joint", None), ("raw", None),
                     ("value", None), ("out", None), ("R", 0), ("L", -3), ("nbytes", 0), ("stat", 7), ("corr", 5), ("P", -1), ("R", too_many)):
        args = dict(good, **{key: bad})
        if key == "R" and bad == too_many:
            args["nbytes"] = lib.sq_covariation_wstat_scratch(too_many, L)
        assert lookup(*(args[k] for k in order), None) == -1, key
        assert (b"2^22 rows" in lib.sq_last_error()) == (bad == too_many), key
    torch.cuda.synchronize()
    for t in bufs:                                                           # nothing was launched, cleared or written
        assert (t == (249 if t.dtype == torch.uint8 else -7)).all()


def test_row_identity_weights_go_in_as_they_are_and_equal_the_cpu_built_result():
    """CovariationStatistics(weights=RowIdentity(...).weights()) on the example alignment: formed on the device from the
    device's weights, and equal to the result built under the OracleEngine from the same weights: pairs and the table
    exactly, floats under the bound with the reference's scales."""
    import torch
    from squarna_amd import CovariationStatistics, RowIdentity, engine as E
    from tests.oracle_engine import OracleEngine
    weights = RowIdentity(inputfile=ALI).weights()
    assert weights.is_cuda and weights.dtype == torch.float64 and float(weights.min()) < 1.0
    for kw in (dict(), dict(statistic="mi", correction="asc", min_rows=0.75), dict(pairs=[(0, 9), (3, 30), (0, 9)], statistic="chi", correction=None)):
        res = CovariationStatistics(inputfile=ALI, weights=weights, **kw)
        with E.use_engine(OracleEngine()):
            host = CovariationStatistics(inputfile=ALI, weights=weights.cpu(), **kw)
        ref = reference(res.sequences, weights.tolist())
        s, c = res.statistic, res.correction
        assert res.source == "device" and res.device.type == "cuda" and host.source == "host" and res.mode == host.mode and len(res) == len(host) > 0
        for key in ("pair_cols", "joint", "rows", "weights"):
            assert getattr(res, key).is_cuda and getattr(res, key).dtype == getattr(host, key).dtype and torch.equal(getattr(res, key).cpu(), getattr(host, key)), key
        assert res.raw.is_cuda and res.value.is_cuda and res.weights.data_ptr() == weights.data_ptr()       # not copied, not downloaded
        assert torch.equal(res.canonical().cpu(), host.canonical()) and all(torch.equal(a.cpu(), b) for a, b in zip(res.marginals(), host.marginals()))
        cols = [tuple(p) for p in res.pair_cols.tolist()]
        scale_raw = torch.tensor([ref.scale[s][p] for p in cols], dtype=torch.float64)
        scale_value = torch.tensor([abs(ref.S[s][p]) + abs(ref.term(s, c, *p)) for p in cols], dtype=torch.float64)
        assert ((res.raw.cpu() - host.raw).abs() <= BOUND * scale_raw).all() and ((res.value.cpu() - host.value).abs() <= BOUND * scale_value).all()
        if c is not None:
            assert res.col_mean.is_cuda and ((res.col_mean.cpu() - host.col_mean).abs() <= BOUND * host.col_mean).all()
            assert abs(float(res.mean_all) - float(host.mean_all)) <= BOUND * float(host.mean_all)
        check_records(ref, s, c, cols, (res.joint * ONE).long().tolist(), res.raw.tolist(), res.value.tolist(), [ref.record(s, c, *p) for p in cols])
        assert res.to_matrix().is_cuda and res.to_matrix("GC").is_cuda and torch.equal(res.to_matrix("rows").cpu(), host.to_matrix("rows"))
        assert res.cpu().value.tolist() == res.value.tolist() and len(res.top(3)) == min(3, len(res)) and res.top(3).value.is_cuda
