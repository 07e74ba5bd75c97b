"""GPU tests of Covariation() and its two device entries (sq_covariation_scan, sq_covariation_pairs) against the count
reference of tests/covariation_checks.py (plain Python counts and the distance table), the numpy fallback and the result built
under the OracleEngine.  All comparisons are exact; records are compared after sorting by flat index."""
import ctypes
import random

import numpy as np
import pytest

from tests.covariation_checks import DEFAULTS, EVERY_CELL, check_records, count_cells, count_select, random_rows, select

pytestmark = pytest.mark.gpu

ALI = "examples/ali_input.afa"


def consts():
    from squarna_amd import device_calls as dc
    return dc.COVAR_TILE, dc.COVAR_WORD_CHUNK, dc.COVAR_MAX_BLOCKS


def device_rows(rows):
    import torch
    return torch.from_numpy(np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), len(rows[0])).copy()).cuda()


def gpu_scan(rows, cap=None, **thr):
    """HipEngine.covariation_scan as [(v, w, counts, cov)] sorted by flat index."""
    import torch
    from squarna_amd.engine import HipEngine
    L = len(rows[0])
    flat, counts, cov = HipEngine().covariation_scan(device_rows(rows), cap=cap, **thr)
    assert flat.is_cuda and counts.is_cuda and cov.is_cuda and (flat.dtype, counts.dtype, cov.dtype) == (torch.int64, torch.int32, torch.int64)
    assert tuple(counts.shape) == (int(flat.numel()), 7) and cov.shape == flat.shape
    order = torch.argsort(flat)
    flat, counts, cov = flat[order].tolist(), counts[order].tolist(), cov[order].tolist()
    assert len(set(flat)) == len(flat)                                       # no cell twice
    return [(f // L, f % L, c, x) for f, c, x in zip(flat, counts, cov)]


def gpu_pairs(rows, pairs):
    import torch
    from squarna_amd.engine import HipEngine
    counts, cov = HipEngine().covariation_pairs(device_rows(rows), torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).cuda())
    assert counts.is_cuda and cov.is_cuda and counts.dtype == torch.int32 and cov.dtype == torch.int64
    assert tuple(counts.shape) == (len(pairs), 7) and tuple(cov.shape) == (len(pairs),)
    return [(v, w, c, x) for (v, w), c, x in zip(pairs, counts.tolist(), cov.tolist())]


@pytest.mark.parametrize("R", [1, 63, 64, 65, "chunk+1"])
def test_scan_and_pairs_against_the_count_reference(R):
    tile, chunk, _ = consts()
    R = 64 * chunk + 1 if R == "chunk+1" else R
    rng = random.Random(R)
    for L in (1, 2, tile - 1, tile, tile + 1, 3 * tile + 1):
        rows = random_rows(1000 * R + L, R, L)
        cells = count_cells(rows)
        for thr in (DEFAULTS, EVERY_CELL):
            assert gpu_scan(rows, **thr) == select(cells, **thr), (R, L, thr)
        pairs = [rng.choice(sorted(cells)) for _ in range(70)] if cells else []          # any order, repeats, any span
        assert gpu_pairs(rows, pairs) == [(v, w) + cells[(v, w)] for v, w in pairs], (R, L)


def test_the_stage_flushes_inside_a_tile_and_the_call_is_repeated_once():
    """R = 5, L = 4 tiles, the columns alternate G / C and nothing is thresholded: every cell of every tile off the diagonal is
    a hit, 1024 a tile, so the stage flushes inside the tile.  With cap 100 the first call stores 100 records and counts them
    all; the second has room."""
    tile = consts()[0]
    L = 4 * tile
    rows = ["GC" * (L // 2)] * 5
    exp = count_select(rows, **EVERY_CELL)
    assert len(exp) == L * (L - 1) // 2 and exp[0][2:] == ([0, 0, 5, 0, 0, 0, 0], 0) and exp[1][2:] == ([0] * 7, 0)
    full = gpu_scan(rows, **EVERY_CELL)
    assert full == exp
    assert gpu_scan(rows, cap=100, **EVERY_CELL) == full


def test_more_tiles_than_blocks():
    """R = 3, L = 64 tiles + 1: 2145 tiles for at most 2048 blocks, so the first blocks take a second tile."""
    tile, _, max_blocks = consts()
    L = tile * 64 + 1
    assert (L + tile - 1) // tile * ((L + tile - 1) // tile + 1) // 2 > max_blocks
    rows = random_rows(64, 3, L, "ACGU-", helices=0)
    exp = count_select(rows, minspan=4, min_rows=3, min_cov=1)
    assert len(exp) > 1000 and any(w == L - 1 for _, w, _, _ in exp)
    assert gpu_scan(rows, minspan=4, min_rows=3, min_cov=1) == exp


def _raw(dtype_sizes):
    """Device buffers filled with a sentinel (249 in bytes, -7 otherwise) for direct calls of the entries."""
    import torch
    return [torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda") for dt, n in dtype_sizes]


def test_pairs_status_leaves_the_other_records_right():
    import torch
    from squarna_amd import _lib, Covariation
    lib = _lib.load()
    rows = random_rows(12, 9, 20)
    cells = count_cells(rows)
    pairs = [(2, 11), (3, 20), (0, 19)]                                      # the middle one: w = L
    d_rows, d_pairs = device_rows(rows), torch.tensor(pairs, dtype=torch.int32).cuda()
    nbytes = lib.sq_covariation_scratch(9, 20)
    scratch, counts, cov, out = _raw([(torch.int64, nbytes // 8), (torch.int32, 21), (torch.int64, 3), (torch.int64, 2)])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.sq_covariation_pairs(p(d_rows), 9, 20, p(d_pairs), 3, p(scratch), nbytes, p(counts), p(cov), p(out), None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 2]
    got = list(zip(counts.view(3, 7).tolist(), cov.tolist()))
    assert got[1] == ([0] * 7, 0) and got[0] == cells[(2, 11)] and got[2] == cells[(0, 19)]
    with pytest.raises(RuntimeError):
        Covariation(sequences=rows, pairs=pairs)
    for bad in ([(4, 4)], [(-1, 3)], [(9, 2)]):
        with pytest.raises(RuntimeError):
            gpu_pairs(rows, bad)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib
    lib = _lib.load()
    R, L, cap = 9, 20, 8
    assert lib.sq_covariation_scratch(0, 5) == 0 and lib.sq_covariation_scratch(5, 0) == 0
    nbytes = lib.sq_covariation_scratch(R, L)
    assert nbytes == 5 * 1 * 64 * 8                                          # five planes, one word of rows, 64 padded columns
    sizes = [(torch.uint8, R * L), (torch.int64, nbytes // 8), (torch.int64, cap), (torch.int32, cap * 7), (torch.int64, cap), (torch.int64, 2),
             (torch.int32, 6)]
    bufs = _raw(sizes)
    rows, scratch, flat, counts, cov, out, pairs = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    scan, lookup = lib.sq_covariation_scan, lib.sq_covariation_pairs
    good = dict(rows=rows, R=R, L=L, minspan=4, min_rows=1, min_cov=1, scratch=scratch, nbytes=nbytes, flat=flat, counts=counts, cov=cov,
                cap=cap, out=out)
    order = ("rows", "R", "L", "minspan", "min_rows", "min_cov", "scratch", "nbytes", "flat", "counts", "cov", "cap", "out")
    for key, bad in (("rows", None), ("scratch", None), ("flat", None), ("counts", None), ("cov", None), ("out", None), ("R", 0), ("L", 0),
                     ("nbytes", nbytes - 8), ("minspan", -1), ("min_rows", -1), ("min_cov", -1), ("cap", -1)):
        args = dict(good, **{key: bad})
        assert scan(*(args[k] for k in order), None) == -1, key
        assert (b"scratch" in lib.sq_last_error()) == (key == "nbytes"), key
    good = dict(rows=rows, R=R, L=L, pairs=pairs, P=3, scratch=scratch, nbytes=nbytes, counts=counts, cov=cov, out=out)
    order = ("rows", "R", "L", "pairs", "P", "scratch", "nbytes", "counts", "cov", "out")
    for key, bad in (("rows", None), ("pairs", None), ("scratch", None), ("counts", None), ("cov", None), ("out", None), ("R", 0), ("L", -3),
                     ("nbytes", 0), ("P", -1)):
        args = dict(good, **{key: bad})
        assert lookup(*(args[k] for k in order), None) == -1, key
    torch.cuda.synchronize()
    for t in bufs:                                                           # nothing was launched, cleared or written
        assert (t == (249 if t.dtype == torch.uint8 else -7)).all()


def test_covariation_of_a_folded_alignment_equals_the_cpu_built_result():
    import torch
    from squarna_amd import Covariation, FoldAlignment, engine as E
    from tests.oracle_engine import OracleEngine
    res = Covariation(alignment=FoldAlignment(inputfile=ALI))
    with E.use_engine(OracleEngine()):
        host = Covariation(alignment=FoldAlignment(inputfile=ALI))
    assert res.source == "device" and res.device.type == "cuda" and host.source == "host" and res.mode == host.mode == "pairs" and len(res)
    assert (res.pair_cols.dtype, res.counts.dtype, res.cov.dtype) == (torch.int32, torch.int32, torch.int64)
    assert (res.names, res.sequences, res.R, res.L) == (host.names, host.sequences, host.R, host.L)
    for key in ("pair_cols", "counts", "cov", "bp_rows", "both_gap", "incompatible", "types"):
        got = getattr(res, key)
        assert got.is_cuda and got.dtype == getattr(host, key).dtype and got.tolist() == getattr(host, key).tolist(), key
    assert res.covarying().tolist() == host.covarying().tolist() and (res.score(0.5).cpu() - host.score(0.5)).abs().max() <= 1e-12
    assert torch.equal(res.to_matrix().cpu(), host.to_matrix()) and res.to_matrix("types").is_cuda
    v, w = res.pair_cols[0].tolist()
    assert res.of(v, w) == host.of(v, w) and res.cpu().cov.tolist() == host.cov.tolist()
    table = Covariation(alignment=FoldAlignment(inputfile=ALI), pairs="table")
    assert table.source == "device" and len(table)
    check_records(table.pair_cols.tolist(), table.counts.tolist(), table.cov.tolist(),
                  [(v, w) + count_cells(table.sequences)[(v, w)] for v, w in table.pair_cols.tolist()])


def test_scan_of_a_random_alignment_equals_the_numpy_fallback():
    from squarna_amd import Covariation, engine as E
    from tests.oracle_engine import OracleEngine
    rows = random_rows(130200, 130, 200, "ACGU-", helices=4)
    res = Covariation(sequences=rows)
    with E.use_engine(OracleEngine()):
        host = Covariation(sequences=rows)
    assert res.source == "device" and res.mode == host.mode == "scan" and host.source == "host" and len(res) == len(host) > 1000
    for key in ("pair_cols", "counts", "cov"):
        assert getattr(res, key).is_cuda and getattr(res, key).tolist() == getattr(host, key).tolist(), key
    flat = res.pair_cols[:, 0].long() * 200 + res.pair_cols[:, 1].long()
    assert (flat[1:] > flat[:-1]).all()                                      # sorted by (v, w)
    assert (res.score().cpu() - host.score()).abs().max() <= 1e-12
