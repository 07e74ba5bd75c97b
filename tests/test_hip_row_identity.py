"""GPU tests of RowIdentity() and its device entry (sq_row_identity) against the naive reference of tests/identity_checks.py
(zipped strings, a loop over a list of kept rows) and the numpy fallback built under the OracleEngine.  All comparisons are
exact.  The shapes are the smallest at which each part can go wrong: R around the 64-row tile (which is also the word of the
kept mask), L around the 64-column word and the chunk of words a block stages, more tiles than blocks, and the row counts at
which a lane of the filter kernel holds one more power of two of words of a row (4096 rows per word and lane)."""
import ctypes
import random

import numpy as np
import pytest

from tests.identity_checks import DENOMINATORS, as_lists, chain_rows, check_result, family_rows, mixed_rows, naive

pytestmark = pytest.mark.gpu


def consts():
    from squarna_amd import device_calls as dc
    return dc.IDENTITY_TILE, dc.IDENTITY_WORD_CHUNK, dc.IDENTITY_MAX_BLOCKS


def device_rows(rows):
    import torch
    return torch.from_numpy(np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), len(rows[0])).copy()).cuda()


def gpu(rows, denominator="shorter", T=8000, matrix=True):
    """HipEngine.row_identity as a dict of host lists."""
    import torch
    from squarna_amd.engine import HipEngine
    R = len(rows)
    res = HipEngine().row_identity(device_rows(rows), DENOMINATORS.index(denominator), T, matrix)
    for key in ("len", "bases", "neighbours"):
        assert res[key].is_cuda and res[key].dtype == torch.int32 and tuple(res[key].shape) == (R,), key
    assert res["keep"].is_cuda and res["keep"].dtype == torch.bool and tuple(res["keep"].shape) == (R,)
    if matrix:
        assert all(res[k].is_cuda and res[k].dtype == torch.int32 and tuple(res[k].shape) == (R, R) for k in ("same", "both"))
    else:
        assert res["same"] is None and res["both"] is None
    return as_lists(res)


def host(rows, **kw):
    from squarna_amd import RowIdentity, engine as E
    from tests.oracle_engine import OracleEngine
    with E.use_engine(OracleEngine()):
        return RowIdentity(sequences=rows, **kw)


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 129, 193])
def test_shapes_against_the_naive_reference(R):
    chunk = consts()[1]
    for L in (1, 63, 64, 65, 64 * chunk + 1):
        rows = mixed_rows(1000 * R + L, R, L) if L < 100 else family_rows(1000 * R + L, R, L, families=5, alphabet="ACGU-N")
        for denominator in DENOMINATORS:
            for T in (0, 8000, 10000):
                check_result(gpu(rows, denominator, T), naive(rows, denominator, T), (R, L, denominator, T))


def test_the_exact_threshold():
    """same = 4 of den = 5: neighbours at 8000 basis points, not at 8001, whatever the denominator is made of.  The padded
    rows give the three denominators three values: 5 residues in the shorter row, 5 aligned columns ... and L."""
    for rows, dens in ((["ACGUA", "ACGUC"], (5, 5, 5)),
                       (["ACGUA--NN-----", "ACGUC----NN---"], (7, 5, 14)), (["ACGUAACGUAAN--", "ACGUCUGCAU--NN"], (12, 10, 14))):
        for denominator, den in zip(DENOMINATORS, dens):
            same = naive(rows, denominator, 0)["same"][0][1]
            T = same * 10000 // den                                          # the largest T at which the two are neighbours
            assert same * 10000 >= T * den > same * 10000 - den
            at, above = gpu(rows, denominator, T), gpu(rows, denominator, T + 1)
            check_result(at, naive(rows, denominator, T), (rows, denominator, T))
            check_result(above, naive(rows, denominator, T + 1), (rows, denominator, T + 1))
            assert at["neighbours"] == [2, 2] and at["keep"] == [True, False] and above["neighbours"] == [1, 1] and above["keep"] == [True, True]
    assert gpu(["ACGUA", "ACGUC"], "shorter", 8000)["neighbours"] == [2, 2] and gpu(["ACGUA", "ACGUC"], "shorter", 8001)["neighbours"] == [1, 1]


def test_special_rows():
    """Identical rows; an all-gap row (len 0, den 0 under "shorter" and "aligned": a neighbour of nobody even at T = 0, and
    kept; under "columns" den is L > 0 and at T = 0 the definition makes every pair of rows neighbours); a row of N only."""
    same = ["ACGUacgu-.~tT"] * 70
    got = gpu(same, "shorter", 10000)
    check_result(got, naive(same, "shorter", 10000))
    assert got["neighbours"] == [70] * 70 and got["keep"] == [True] + [False] * 69 and got["len"] == [10] * 70
    rows = ["ACGUACGUAC", "----------", "NNNNNNNNNN", "ACGUACGUAC", ".~-.~-.~-."]
    for denominator in DENOMINATORS:
        for T in (0, 1, 10000):
            got = gpu(rows, denominator, T)
            check_result(got, naive(rows, denominator, T), (denominator, T))
            assert got["len"] == [10, 0, 10, 10, 0] and got["bases"] == [10, 0, 0, 10, 0]
            assert got["same"][1] == [0] * 5 and got["both"][1] == [0] * 5 and got["same"][2] == [0] * 5 and got["both"][2] == [10, 0, 10, 10, 0]
            if denominator != "columns" or T:
                assert got["neighbours"][1] == got["neighbours"][4] == 1 and got["keep"][1] and got["keep"][4]
    assert gpu(rows, "columns", 0)["neighbours"] == [5] * 5


def test_the_filter_is_sequential():
    """a ~ b, b ~ c, a !~ c at rows 63, 64, 65 (two words of the kept mask): b is dropped and protects nobody, so c is kept.
    Then a chain of 130 rows in which row k is a neighbour of k - 1 and k + 1 only: exactly the even rows stay."""
    a, b, c = "AAAAAAAACCCC", "AAAAAAAAAAAA", "CCCCAAAAAAAA"                     # a-b 8 / 12, b-c 8 / 12, a-c 4 / 12
    rows = ["-" * 12] * 63 + [a, b, c]
    got = gpu(rows, "shorter", 6000)
    check_result(got, naive(rows, "shorter", 6000))
    assert got["keep"] == [True] * 64 + [False, True] and got["neighbours"][63:] == [2, 3, 2]
    chain = chain_rows(130)
    for denominator in ("shorter", "aligned"):
        got = gpu(chain, denominator, 5000, matrix=False)
        assert got["keep"] == [k % 2 == 0 for k in range(130)] and got["neighbours"] == [2] + [3] * 128 + [2]
        assert got["len"] == got["bases"] == [4] * 130
        check_result(got, as_lists(host(chain, threshold=0.5, denominator=denominator, matrix=False)), denominator)


def test_matrix_or_not():
    rows = mixed_rows(5, 131, 90)
    for denominator in DENOMINATORS:
        full, bare = gpu(rows, denominator, 7500), gpu(rows, denominator, 7500, matrix=False)
        assert all(bare[k] == full[k] for k in ("len", "bases", "neighbours", "keep")) and bare["same"] is None
        check_result(full, naive(rows, denominator, 7500), denominator)


def test_more_tiles_than_blocks_and_the_api_against_the_numpy_path():
    """R = 63 tiles + 1: 2080 tiles for at most 2048 blocks, so the first blocks take a second tile.  The naive reference
    would zip eight million pairs of rows: the numpy path (pinned to it at the small shapes) stands in."""
    import torch
    from squarna_amd import RowIdentity
    tile, _, max_blocks = consts()
    R = tile * 63 + 1
    assert (R + tile - 1) // tile * ((R + tile - 1) // tile + 1) // 2 > max_blocks
    rows = family_rows(63, R, 9, families=40, rate=0.1)
    res, ref = RowIdentity(sequences=rows, threshold=0.85), host(rows, threshold=0.85)
    assert res.source == "device" and ref.source == "host" and res.device.type == "cuda" and res.same is not None
    for key in ("len", "bases", "neighbours", "keep", "same", "both"):
        got = getattr(res, key)
        assert got.is_cuda and got.dtype == getattr(ref, key).dtype and torch.equal(got.cpu(), getattr(ref, key)), key
    assert 1 < int(res.keep.sum()) < R and int(res.neighbours.max()) > 1
    assert res.neighbours_at(0.85).tolist() == res.neighbours.tolist() and res.filtered() == ref.filtered()
    assert torch.equal(res.identity().cpu(), ref.identity()) and res.weights().is_cuda and torch.equal(res.weights().cpu(), ref.weights())
    best, where = res.nearest()
    assert torch.equal(best.cpu(), ref.nearest()[0]) and torch.equal(where.cpu(), ref.nearest()[1])
    # (two float64 sums of n = 8.1e6 numbers in [0, 1] in different orders: each is within n * 2^-53 of the exact sum relative
    # to it, so the two means, themselves <= 1, differ by at most 2 * 8.1e6 * 1.2e-16 < 2e-9)
    assert abs(res.mean_identity().item() - ref.mean_identity().item()) <= 2e-9
    assert res.identity_of(3, 4000) == ref.identity_of(3, 4000)
    back = res.cpu()
    assert back.device.type == "cpu" and torch.equal(back.same, ref.same) and back.keep.tolist() == ref.keep.tolist()


def test_more_rows_than_one_word_per_lane_holds():
    """4200 rows: the kept mask has 66 words, so a lane of the filter kernel holds two words of a row.  The first 4100 rows are
    all different (all kept at T = 10000); the last 100 repeat the rows 4096 .. 4099, whose kept bits lie in word 64, and are
    dropped by nothing else.  Then T = 8000 against the numpy path: neighbours in every word, verdicts that depend on verdicts."""
    rng = random.Random(4200)
    seen = set()
    while len(seen) < 4100:
        seen.add("".join(rng.choice("ACGU") for _ in range(10)))
    first = sorted(seen)
    rng.shuffle(first)
    rows = first + [first[4096 + k % 4] for k in range(100)]
    got = gpu(rows, "shorter", 10000, matrix=False)
    assert got["keep"] == [True] * 4100 + [False] * 100 and got["neighbours"][4096:4100] == [26] * 4 and got["neighbours"][4100:] == [26] * 100
    assert got["neighbours"][:4096] == [1] * 4096
    ref = as_lists(host(rows, threshold=1.0, matrix=False))
    check_result(got, ref)
    near = gpu(rows, "shorter", 8000, matrix=False)                           # (many neighbours in every word)
    check_result(near, as_lists(host(rows, threshold=0.8, matrix=False)))
    assert near["keep"] != got["keep"]


@pytest.mark.parametrize("n", [64 * 64 + 1, 64 * 128 + 1, 64 * 256 + 1, 64 * 512 + 1])
def test_every_form_of_the_filter_kernel_on_planted_duplicates(n):
    """A lane of the filter kernel holds 1, 2, 4, 8 or 16 words of a row of the bit matrix; with n rows and more it holds 2, 4,
    8 and 16 (the tests above run the one-word form).  Gap-free rows of ten bases at T = 10000: two rows are neighbours iff
    they are the same string, so a plain dict gives the expectation.  The first n rows are all different; then come 100
    copies of rows of the first word of the kept mask, 100 of the last full word among the n and 100 copies of the last four
    of the n, whose kept bits lie in word n / 64 -- the first that the next smaller form could not hold.  A copy is dropped by
    the one kept bit of its original, and a dropped copy protects nobody."""
    rng = random.Random(n)
    seen = set()
    while len(seen) < n:
        seen.add("".join(rng.choice("ACGU") for _ in range(10)))
    first = sorted(seen)
    rng.shuffle(first)
    R = n + 300
    rows = first + [first[rng.randrange(64)] for _ in range(100)] + [first[n // 64 * 64 - 1 - rng.randrange(64)] for _ in range(100)] + \
        [first[n - 1 - k % 4] for k in range(100)]
    count, original = {}, {}
    for k, row in enumerate(rows):
        count[row] = count.get(row, 0) + 1
        original.setdefault(row, k)
    got = gpu(rows, "shorter", 10000, matrix=False)
    assert got["keep"] == [original[row] == k for k, row in enumerate(rows)] and got["keep"] == [True] * n + [False] * 300
    assert got["neighbours"] == [count[row] for row in rows] and min(got["neighbours"][n - 4:n]) >= 26
    assert got["len"] == got["bases"] == [10] * R


def _raw(dtype_sizes):
    """Device buffers filled with a sentinel (249 in bytes, -7 otherwise) for direct calls of the entry."""
    import torch
    return [torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda") for dt, n in dtype_sizes]


def _untouched(t):
    return bool((t == (249 if t.element_size() == 1 else -7)).all())


def test_direct_calls_write_nothing_beyond_their_rows():
    import torch
    from squarna_amd import _lib
    lib = _lib.load()
    R, L, pad = 70, 67, 16
    rows = mixed_rows(70, R, L)
    exp = naive(rows, "aligned", 7000)
    d_rows = device_rows(rows)
    nbytes = lib.sq_row_identity_scratch(R, L)
    assert nbytes == (4 * 2 * 128 + 70 * 2) * 8                              # four planes, two words of columns, 128 padded rows; 70 x 2 words
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for matrix in (True, False):
        scratch, length, bases, same, both, nb, keep, out = _raw([(torch.int64, nbytes // 8 + pad), (torch.int32, R + pad), (torch.int32, R + pad),
                                                                  (torch.int32, R * R + pad), (torch.int32, R * R + pad), (torch.int32, R + pad),
                                                                  (torch.uint8, R + pad), (torch.int64, 2 + pad)])
        assert lib.sq_row_identity(p(d_rows), R, L, 1, 7000, p(scratch), nbytes, p(length), p(bases), p(same if matrix else None),
                                   p(both if matrix else None), p(nb), p(keep), p(out), None) == 0
        torch.cuda.synchronize()
        assert out[:2].tolist() == [0, 0]
        assert (length[:R].tolist(), bases[:R].tolist(), nb[:R].tolist()) == (exp["len"], exp["bases"], exp["neighbours"])
        assert [bool(x) for x in keep[:R].tolist()] == exp["keep"] and set(keep[:R].tolist()) <= {0, 1}
        for t, n in ((scratch, nbytes // 8), (length, R), (bases, R), (nb, R), (keep, R), (out, 2), (same, R * R if matrix else 0),
                     (both, R * R if matrix else 0)):
            assert _untouched(t[n:]), n
        if matrix:
            assert same[:R * R].view(R, R).tolist() == exp["same"] and both[:R * R].view(R, R).tolist() == exp["both"]
        # the measuring entry: one kernel at a time on what the earlier ones left gives the same numbers again
        tail = (p(d_rows), R, L, 1, 7000, p(scratch), nbytes, p(length), p(bases), p(same if matrix else None), p(both if matrix else None),
                p(nb), p(keep), p(out), None)
        assert lib.sq_row_identity_phases(0, *tail) == -1 and lib.sq_row_identity_phases(8, *tail) == -1
        for phase in (1, 2, 4):
            assert lib.sq_row_identity_phases(phase, *tail) == 0
            torch.cuda.synchronize()
            assert (length[:R].tolist(), bases[:R].tolist(), nb[:R].tolist()) == (exp["len"], exp["bases"], exp["neighbours"])
            assert [bool(x) for x in keep[:R].tolist()] == exp["keep"] and _untouched(keep[R:]) and _untouched(nb[R:]) and _untouched(scratch[nbytes // 8:])


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib, device_calls as dc
    lib = _lib.load()
    R, L = 9, 20
    assert lib.sq_row_identity_scratch(0, 5) == 0 and lib.sq_row_identity_scratch(5, 0) == 0
    assert lib.sq_row_identity_scratch(dc.IDENTITY_MAX_ROWS + 1, 5) == 0 and lib.sq_row_identity_scratch(5, dc.IDENTITY_MAX_COLS + 1) == 0
    assert lib.sq_row_identity_scratch(dc.IDENTITY_MAX_ROWS, 64) == (4 * 65536 + 65535 * 1024) * 8
    nbytes = lib.sq_row_identity_scratch(R, L)
    assert nbytes == (4 * 1 * 64 + 9) * 8
    bufs = _raw([(torch.uint8, R * L), (torch.int64, nbytes // 8), (torch.int32, R), (torch.int32, R), (torch.int32, R * R), (torch.int32, R * R),
                 (torch.int32, R), (torch.uint8, R), (torch.int64, 2)])
    rows, scratch, length, bases, same, both, nb, keep, out = (ctypes.c_void_p(t.data_ptr()) for t in bufs)
    good = dict(rows=rows, R=R, L=L, den=0, T=8000, scratch=scratch, nbytes=nbytes, len=length, bases=bases, same=same, both=both, nb=nb,
                keep=keep, out=out)
    order = ("rows", "R", "L", "den", "T", "scratch", "nbytes", "len", "bases", "same", "both", "nb", "keep", "out")
    for key, bad in (("rows", None), ("scratch", None), ("len", None), ("bases", None), ("nb", None), ("keep", None), ("out", None), ("R", 0),
                     ("R", -1), ("L", 0), ("R", dc.IDENTITY_MAX_ROWS + 1), ("L", dc.IDENTITY_MAX_COLS + 1), ("den", -1), ("den", 3), ("T", -1),
                     ("T", 10001), ("same", None), ("both", None), ("nbytes", nbytes - 8), ("nbytes", 0)):
        args = dict(good, **{key: bad})
        assert lib.sq_row_identity(*(args[k] for k in order), None) == -1, (key, bad)
        assert (b"scratch" in lib.sq_last_error()) == (key == "nbytes"), key
    torch.cuda.synchronize()
    for t in bufs:                                                           # nothing was launched, cleared or written
        assert _untouched(t)
    with pytest.raises(ValueError, match="RowIdentity"):
        from squarna_amd import RowIdentity
        RowIdentity(sequences=["A"] * (dc.IDENTITY_MAX_ROWS + 1))


def test_row_identity_of_a_folded_alignment_equals_the_cpu_built_result():
    import torch
    from squarna_amd import Covariation, FoldAlignment, RowIdentity
    ali = FoldAlignment(inputfile="examples/ali_input.afa")
    res = RowIdentity(alignment=ali, threshold=0.9)
    ref = host(list(ali.sequences), names=list(ali.names), threshold=0.9)
    assert res.source == "device" and res.device == ali.device and (res.names, res.sequences) == (ref.names, ref.sequences)
    assert as_lists(res) == as_lists(ref)
    check_result(as_lists(res), naive(res.sequences, "shorter", 9000))
    names, seqs = res.filtered()
    cov = Covariation(sequences=seqs, names=names)
    assert cov.source == "device" and cov.R == int(res.keep.sum()) and cov.names == names
