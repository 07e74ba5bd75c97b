"""GPU tests of CovariationSignificance() and its device entries (sq_covariation_null, sq_covariation_null_planes) against the
numpy path of squarna_amd/covariation_significance.py -- which tests/test_covariation_significance_api.py pins to the
plain-Python restatement -- and against the result built under the OracleEngine.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest

from squarna_amd.covariation_significance import _host_null, _shuffled_classes
from tests.covariation_checks import ALPHABET, random_rows
from tests.covariation_null_checks import MASK, PLANTED, planted_rows, planted_stats

pytestmark = pytest.mark.gpu

ALI = "examples/ali_input.afa"


def consts():
    from squarna_amd import device_calls as dc
    return dc.COVAR_TILE, dc.COVAR_WORD_CHUNK, dc.COVAR_MAX_BLOCKS, dc.COVAR_NULL_MAX_ROWS, dc.COVAR_NULL_LDS_BINS


def byte_rows(rows):
    return np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), len(rows[0])).copy()


def numpy_planes(rows, k, seed):
    """uint64[5, W, Lpad]: the planes of sample k from the numpy shuffle, bit by bit."""
    from squarna_amd.covariation import _classes
    cls = _shuffled_classes(_classes(byte_rows(rows)), k, seed)
    R, L = cls.shape
    W, Lpad = (R + 63) // 64, (L + 63) // 64 * 64
    out = np.zeros((5, W, Lpad), np.uint64)
    for p in range(5):
        bits = np.zeros((W * 64, L), np.uint64)
        bits[:R] = cls == p
        out[p, :, :L] = (bits.reshape(W, 64, L) << np.arange(64, dtype=np.uint64)[None, :, None]).sum(1, dtype=np.uint64)
    return out


def gpu_planes(rows, k, seed):
    import torch
    from squarna_amd.engine import HipEngine
    got = HipEngine().covariation_null_planes(torch.from_numpy(byte_rows(rows)).cuda(), k, seed)
    assert got.is_cuda and got.dtype == torch.int64
    return got.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 130, "cap"])
def test_planes_against_numpy(R):
    R = consts()[3] if R == "cap" else R
    for L in (1, 31, 64, 65):
        rows = random_rows(7 * R + L, R, L)
        for k, seed in ((0, 0), (5, MASK)):
            got, exp = gpu_planes(rows, k, seed), numpy_planes(rows, k, seed)
            assert got.shape == exp.shape and np.array_equal(got, exp), (R, L, k, seed)
            assert not got[:, :, L:].any() and (R % 64 == 0 or not (got[:, -1, :] >> np.uint64(R % 64)).any())
            assert sum(int(np.unpackbits(got[p].view(np.uint8)).sum()) for p in range(5)) == sum(ch in "ACGUacgutT-.~" for r in rows for ch in r)


def test_planes_of_gaps_and_of_lowercase_and_t():
    gaps = ["-.~" * 11] * 70
    got = gpu_planes(gaps, 2, 9)
    assert np.array_equal(got, numpy_planes(gaps, 2, 9)) and not got[:4].any()
    assert [int(w) for w in got[4, :, 0]] == [MASK, (1 << 6) - 1] and not got[4, :, 33:].any()
    mixed = random_rows(4, 67, 40, "acgutTACGU")
    got = gpu_planes(mixed, 1, 3)
    assert np.array_equal(got, numpy_planes(mixed, 1, 3)) and not got[4].any()
    assert np.array_equal(got, numpy_planes([r.upper().replace("T", "U") for r in mixed], 1, 3))


def test_planes_of_several_samples_from_one_launch():
    import torch
    from squarna_amd.engine import HipEngine
    rows = random_rows(21, 67, 70)
    got = HipEngine().covariation_null_planes(torch.from_numpy(byte_rows(rows)).cuda(), 4, 9, count=3)
    assert tuple(got.shape) == (3, 5, 2, 128)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), np.stack([numpy_planes(rows, 4 + s, 9) for s in range(3)]))


def gpu_null(rows, pairs, cov, minspan, samples, seed, batch=None):
    import torch
    from squarna_amd.engine import HipEngine
    d_pairs = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).cuda()
    got = HipEngine().covariation_null(torch.from_numpy(byte_rows(rows)).cuda(), d_pairs, torch.tensor(cov, dtype=torch.int64).cuda(),
                                       minspan, samples, seed, batch=batch)
    assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int64, torch.int32, torch.int64]
    assert [tuple(t.shape) for t in got] == [(len(pairs),), (len(pairs),), (samples,)]
    return [t.tolist() for t in got]


def numpy_null(rows, pairs, cov, minspan, samples, seed):
    got = _host_null(byte_rows(rows), np.array(pairs, np.int64).reshape(-1, 2), np.array(cov, np.int64), minspan, samples, seed)
    return [a.tolist() for a in got]


def observed(rows, **thr):
    """(pairs, cov) of the numpy scan of the rows."""
    from squarna_amd.covariation import _host_scan
    cols, _, cov = _host_scan(byte_rows(rows), thr["minspan"], thr["min_rows"], thr["min_cov"])
    return [tuple(p) for p in cols.tolist()], cov.tolist()


@pytest.mark.parametrize("R", [1, 65, "chunk+1"])
def test_null_against_the_numpy_path_whatever_the_batch(R):
    tile, chunk = consts()[:2]
    R = 64 * chunk + 1 if R == "chunk+1" else R
    for L in (2, tile - 1, tile + 1, 3 * tile + 1):
        rows = random_rows(1000 * R + L, R, L, ALPHABET if L % 2 else "ACGU-")
        pairs, cov = observed(rows, minspan=1, min_rows=1, min_cov=1)
        for samples in (1, 3, 7):
            exp = numpy_null(rows, pairs, cov, 4, samples, R + samples)
            assert len(exp[2]) == samples and (R == 1 or L < 6 or (any(exp[0]) and max(exp[2]) > 0))
            for batch in sorted({1, 2, samples}):
                assert gpu_null(rows, pairs, cov, 4, samples, R + samples, batch) == exp, (R, L, samples, batch)
            assert gpu_null(rows, pairs, cov, 4, samples, R + samples) == exp, (R, L, samples)


def test_null_thresholds_at_their_edges():
    """No pair; one threshold (every cov equal); every cell a distinct pair with thresholds from 0 on; a threshold above every
    null value; no cell in scope; more thresholds than the scan keeps in LDS."""
    from tests.covariation_checks import EVERY_CELL
    tile, chunk, _, _, lds_bins = consts()
    L = tile + 9
    rows = ["G" + r[1:5] + "C" + r[6:] for r in random_rows(11, 65, L, "ACGU-")]      # (0, 5): G-C in every row, cov 0 in every sample
    assert gpu_null(rows, [], [], 4, 3, 1) == numpy_null(rows, [], [], 4, 3, 1)
    pairs, cov = observed(rows, **EVERY_CELL)
    assert len(pairs) == L * (L - 1) // 2 and min(cov) == 0
    exp = numpy_null(rows, pairs, cov, 1, 3, 1)
    assert gpu_null(rows, pairs, cov, 1, 3, 1, 2) == exp and exp[0][cov.index(0)] == 3 * len(pairs)       # cov 0: every null cell
    middle = sorted(cov)[len(cov) // 2]
    same = [middle] * 40
    exp = numpy_null(rows, pairs[:40], same, 4, 3, 1)
    assert gpu_null(rows, pairs[:40], same, 4, 3, 1) == exp and len(set(exp[0])) == 1 and 0 < exp[0][0] < 3 * len(pairs)
    high = [65 * 65 + 1, middle, 2 ** 40]
    exp = numpy_null(rows, pairs[:3], high, 4, 2, 1)
    assert gpu_null(rows, pairs[:3], high, 4, 2, 1) == exp and exp[0][0] == exp[0][2] == 0 == exp[1][0] and exp[0][1] > 0
    for minspan in (L, L + 7):
        got = gpu_null(rows, pairs[:5], cov[:5], minspan, 3, 1)
        assert got == numpy_null(rows, pairs[:5], cov[:5], minspan, 3, 1) and got[0] == [0] * 5 and got[2] == [0] * 3
    wide = random_rows(12, 64 * chunk + 1, 40, "ACGU")
    cells = [(v, w) for v in range(40) for w in range(v + 1, 40)]
    many = [cells[k % len(cells)] for k in range(2 * lds_bins)]
    values = list(range(2 * lds_bins))
    exp = numpy_null(wide, many, values, 4, 2, 5)
    assert min(exp[2]) > lds_bins                                            # cells beyond the bins kept in LDS
    assert gpu_null(wide, many, values, 4, 2, 5) == exp


def test_more_tiles_than_blocks():
    """R = 3, L = 64 tiles + 1: 2145 tiles for at most 2048 blocks of the one sample of a batch, so the first blocks take a
    second tile; with two samples a batch every block takes several."""
    tile, _, max_blocks = consts()[:3]
    L = tile * 64 + 1
    assert (L + tile - 1) // tile * ((L + tile - 1) // tile + 1) // 2 > max_blocks
    rows = random_rows(64, 3, L, "ACGU-", helices=0)
    pairs = [(0, L - 1), (5, 9), (L - 5, L - 1), (tile, 40 * tile), (3, 5)]
    cov = [1, 2, 3, 4, 1]
    exp = numpy_null(rows, pairs, cov, 4, 2, 8)
    assert all(exp[0]) and min(exp[2]) >= 4
    assert gpu_null(rows, pairs, cov, 4, 2, 8, 1) == exp and gpu_null(rows, pairs, cov, 4, 2, 8, 2) == exp


def _raw(dtype_sizes):
    """Device buffers filled with a sentinel (249 in bytes, -7 otherwise) for direct calls of the entries."""
    import torch
    return [torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda") for dt, n in dtype_sizes]


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib, CovariationSignificance
    lib = _lib.load()
    cap = consts()[3]
    R, L, P, U, K, batch = 9, 20, 3, 2, 4, 2
    scratch_of = lib.sq_covariation_null_scratch
    assert scratch_of(0, 5, 1) == 0 and scratch_of(5, 0, 1) == 0 and scratch_of(5, 5, 0) == 0
    nbytes = scratch_of(R, L, batch)
    assert nbytes == batch * 5 * 1 * 64 * 8 + 184                            # the planes of two samples, 9 * 20 class bytes rounded up to 8
    sizes = [(torch.uint8, R * L), (torch.int32, 2 * P), (torch.int64, P), (torch.int64, U), (torch.int64, scratch_of(cap + 1, L, batch) // 8),
             (torch.int64, U + 1), (torch.int32, P), (torch.int64, K), (torch.int64, 2)]
    bufs = _raw(sizes)
    rows, pairs, cov, thr, scratch, hist, own, null_max, out = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    good = dict(rows=rows, R=R, L=L, minspan=4, pairs=pairs, cov=cov, P=P, thr=thr, U=U, K=K, seed=5, batch=batch, scratch=scratch,
                nbytes=nbytes, hist=hist, own=own, null_max=null_max, out=out)
    order = ("rows", "R", "L", "minspan", "pairs", "cov", "P", "thr", "U", "K", "seed", "batch", "scratch", "nbytes", "hist", "own", "null_max", "out")
    for key, bad in (("rows", None), ("pairs", None), ("cov", None), ("thr", None), ("scratch", None), ("hist", None), ("own", None),
                     ("null_max", None), ("out", None), ("R", 0), ("L", 0), ("K", 0), ("K", -1), ("batch", 0), ("batch", 65536), ("minspan", -1),
                     ("P", -1), ("U", -1), ("nbytes", nbytes - 8), ("R", cap + 1)):
        args = dict(good, **{key: bad})
        if key == "R" and bad > cap:
            args["nbytes"] = scratch_of(bad, L, batch)                       # (large enough: the row cap is what refuses)
        assert lib.sq_covariation_null(*(args[k] for k in order), None) == -1, key
        msg = lib.sq_last_error()
        assert (b"scratch" in msg) == (key == "nbytes") and ((b"%d rows" % cap) in msg) == (key == "R" and bad > cap), (key, msg)
    one = scratch_of(R, L, 1)
    for args in ((None, R, L, 0, 1, 5, scratch, one), (rows, R, L, 0, 1, 5, None, one), (rows, R, L, -1, 1, 5, scratch, one),
                 (rows, R, L, 0, 1, 5, scratch, one - 8), (rows, R, L, 0, 2, 5, scratch, one), (rows, R, L, 0, 0, 5, scratch, one),
                 (rows, cap + 1, L, 0, 1, 5, scratch, scratch_of(cap + 1, L, 1)), (rows, 0, L, 0, 1, 5, scratch, one)):
        assert lib.sq_covariation_null_planes(*args, None) == -1, args[1:6]
    torch.cuda.synchronize()
    for t in bufs:                                                           # nothing was launched, cleared or written
        assert (t == (249 if t.dtype == torch.uint8 else -7)).all()
    with pytest.raises(ValueError, match="COVAR_NULL_MAX_ROWS = %d" % cap):
        CovariationSignificance(sequences=["ACGU"] * (cap + 1), samples=1)


def same_result(res, host):
    import torch
    assert res.source == "device" and res.device.type == "cuda" and host.source == "host" and res.observed.source == "device"
    assert (res.samples, res.seed, res.null_cells, len(res)) == (host.samples, host.seed, host.null_cells, len(host)) and len(res)
    for key in ("pair_cols", "counts", "cov"):
        assert getattr(res.observed, key).tolist() == getattr(host.observed, key).tolist(), key
    for key in ("null_ge", "own_ge", "null_max"):
        got = getattr(res, key)
        assert got.is_cuda and got.dtype == getattr(host, key).dtype and got.tolist() == getattr(host, key).tolist(), key
    K = res.samples
    cov, null_ge, own_ge, null_max = (t.cpu().numpy() for t in (res.observed.cov, res.null_ge, res.own_ge, res.null_max))
    max_ge = (null_max[None, :] >= cov[:, None]).sum(1)
    for got, exp in ((res.evalue(), null_ge.astype(np.float64) / np.float64(K)), (res.pvalue(), (1 + own_ge).astype(np.float64) / np.float64(K + 1)),
                     (res.pvalue_max(), (1 + max_ge).astype(np.float64) / np.float64(K + 1))):
        assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), exp)
    assert res.significant().is_cuda and res.significant().tolist() == host.significant().tolist()
    assert res.to_matrix().is_cuda and torch.equal(res.to_matrix("pvalue").cpu(), host.to_matrix("pvalue"))
    v, w = res.observed.pair_cols[0].tolist()
    assert res.of(v, w) == host.of(v, w) and res.cpu().null_ge.tolist() == host.null_ge.tolist() and res.cpu().observed.device.type == "cpu"


def test_significance_of_the_example_alignment_equals_the_cpu_built_result():
    from squarna_amd import CovariationSignificance, FoldAlignment, engine as E
    from tests.oracle_engine import OracleEngine
    res = CovariationSignificance(inputfile=ALI, samples=20, seed=4)
    steps = CovariationSignificance(alignment=FoldAlignment(inputfile=ALI), pairs="steps", samples=20, seed=4)
    with E.use_engine(OracleEngine()):
        host = CovariationSignificance(inputfile=ALI, samples=20, seed=4)
        host_steps = CovariationSignificance(alignment=FoldAlignment(inputfile=ALI), pairs="steps", samples=20, seed=4)
    assert res.observed.mode == host.observed.mode == "scan" and steps.observed.mode == host_steps.observed.mode == "pairs"
    same_result(res, host)
    same_result(steps, host_steps)
    assert res.null_max.tolist() == steps.null_max.tolist()                  # the null is the alignment's, whatever the pairs


def test_significance_of_the_planted_helices_equals_the_restatement():
    from squarna_amd import CovariationSignificance, engine as E
    from tests.oracle_engine import OracleEngine
    rows, planted = planted_rows()
    res = CovariationSignificance(sequences=rows, samples=PLANTED["samples"], seed=PLANTED["seed"])
    with E.use_engine(OracleEngine()):
        host = CovariationSignificance(sequences=rows, samples=PLANTED["samples"], seed=PLANTED["seed"])
    same_result(res, host)
    pairs, covs, null_ge, own_ge, null_max, null_cells = planted_stats()
    assert [tuple(p) for p in res.observed.pair_cols.tolist()] == pairs and res.observed.cov.tolist() == covs
    assert (res.null_ge.tolist(), res.own_ge.tolist(), res.null_max.tolist(), res.null_cells) == (null_ge, own_ge, null_max, null_cells)
    at = [pairs.index(p) for p in planted]
    evalue = res.evalue().tolist()
    assert all(res.own_ge[k] == 0 for k in at) and all(evalue[k] == min(evalue) for k in at)
