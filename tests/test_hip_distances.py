"""GPU tests of Distances() and its device entry (sq_structure_distances) against the naive reference of
tests/distances_checks.py (sets of pairs, a loop over a list of kept rows), closed forms and the numpy fallback built under
the OracleEngine.  All comparisons are exact.  The shapes are the smallest at which each part can go wrong: S around the
64-row tile (which is also the word of the kept mask), widths around the 64-column word and the chunk of words a block
stages, the widths at which one more span plane appears, groups that begin and end inside a tile, more planned tiles than
blocks, and the row counts at which a lane of the filter kernel holds one more power of two of words of a row."""
import ctypes
import os

import numpy as np
import pytest

from tests.distances_checks import as_lists, chain_rows, check_result, family_rows, naive, partners_of

pytestmark = pytest.mark.gpu
GROUP_SIZES = [0, 1, 3, 64, 65, 2, 0, 130]


def consts():
    from squarna_amd import device_calls as dc
    return dc.DISTANCES_TILE, dc.DISTANCES_WORD_CHUNK, dc.DISTANCES_MAX_BLOCKS


def gpu(structures, **kw):
    from squarna_amd import Distances
    res = Distances(structures, **kw)
    assert res.source == "device" and all(getattr(res, k).is_cuda for k in ("status", "npairs", "neighbours", "leader", "keep", "row_off", "mat_off"))
    return res


def host(structures, **kw):
    from squarna_amd import Distances, engine as E
    from tests.oracle_engine import OracleEngine
    with E.use_engine(OracleEngine()):
        return Distances(structures, **kw)


def split(rows, sizes):
    cut = np.concatenate(([0], np.cumsum(sizes))).tolist()
    return [rows[a:b] for a, b in zip(cut, cut[1:])]


def threshold_of(kw):
    return ("relative", int(round(kw["relative"] * 10000))) if "relative" in kw else ("radius", kw.get("radius", 0))


def check(groups, **kw):
    res = gpu(groups, **kw)
    check_result(as_lists(res), naive(groups, *threshold_of(kw)), ([len(g) for g in groups], kw))
    return res


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 193])
def test_shapes_against_the_naive_reference(S):
    chunk = consts()[1]
    for j, W in enumerate((1, 2, 63, 64, 65, 64 * chunk + 1)):
        rows = family_rows(1000 * S + W, S, W, families=max(S // 16, 2), knots=j % 2 == 1)
        for kw in (dict(radius=0), dict(radius=2), dict(relative=0.25)):
            check([rows], **kw)


@pytest.mark.parametrize("k", [1, 5, 8, 14])
def test_span_planes(k):
    """Widths 2^k and 2^k + 1 (one more plane), and at width 2^k + 2 two rows whose only pairs are (0, 1) and (0, 2^k + 1):
    their spans differ in the top bit alone, so they share nothing."""
    for W in (2 ** k, 2 ** k + 1, 2 ** k + 2):
        near_row, far_row = "()" + "." * (W - 2), "(" + "." * (W - 2) + ")"
        rows = [near_row, far_row, far_row] + family_rows(W, 5, W, families=2)
        res = check([rows], radius=0)
        if W > 2:
            assert res.common_of(0)[:3, :3].tolist() == [[1, 0, 0], [0, 1, 1], [0, 1, 1]] and res.leader[:3].tolist() == [0, 1, 1]


def test_groups_that_share_tiles():
    """Groups that begin and end inside a tile, empty groups, and the same structures planted in different groups that share
    a tile: they are neighbours within their group only."""
    sizes = GROUP_SIZES
    rows = family_rows(5, sum(sizes), 40, families=4, knots=True)
    plant = "((..((...))..))" + "." * 25
    for at in (1, 3, 4, 67, 68, 133, 134, 135, 264):                       # in every non-empty group, next to the borders
        rows[at] = plant
    groups = split(rows, sizes)
    for kw in (dict(radius=0), dict(radius=3), dict(relative=0.2)):
        check(groups, **kw)
    res = gpu(groups, radius=0)
    assert res.leader[[1, 3, 4, 67, 68, 133, 134, 135, 264]].tolist() == [1, 1, 4, 4, 68, 133, 133, 135, 135]
    assert res.neighbours[[1, 3, 4, 67, 68, 133, 134, 135, 264]].tolist() == [2, 2, 2, 2, 1, 2, 2, 2, 2] and res.mat_off.tolist()[-1] == sum(n * n for n in sizes)
    check([rows], radius=0)                                                 # the same rows as one group: now they all are
    everything = gpu(groups, groups="all", radius=0)
    assert everything.leader[[1, 3, 4, 67, 68, 133, 134, 135, 264]].tolist() == [1] * 9
    mixed = [family_rows(7 + k, n, 20 + 50 * k, families=2) for k, n in enumerate([5, 0, 70, 3])]   # widths differ between groups
    check(mixed, radius=1)
    check_result(as_lists(gpu(mixed, groups="all", relative=0.3)), naive([[r for g in mixed for r in g]], "relative", 3000))


def test_the_exact_thresholds():
    rows = ["(((())))", "(((..)))", "(......)", "........", "........"]          # npairs 4 3 1 0 0
    for a, b, d in ((0, 1, 1), (0, 2, 3), (1, 2, 2), (0, 3, 4)):
        for radius, near in ((d, True), (d - 1, False)):
            res = check([[rows[a], rows[b]]], radius=radius)
            assert res.neighbours.tolist() == [1 + near] * 2 and res.keep.tolist() == [True, not near]
    # relative: d * 10000 <= T * (na + nb); rows 0 and 1: d = 1 of 7 pairs: the smallest T that admits them is 1429
    for T, near in ((1429, True), (1428, False)):
        assert check([[rows[0], rows[1]]], relative=T / 10000).neighbours.tolist() == [1 + near] * 2
    assert check([[rows[3], rows[4]]], relative=0.0).neighbours.tolist() == [2, 2]           # two empty structures
    assert check([[rows[2], rows[3]]], relative=0.9999).neighbours.tolist() == [1, 1]        # d = 1 of 1: only T = 10000 admits
    assert check([[rows[2], rows[3]]], relative=1.0).neighbours.tolist() == [2, 2]


def test_the_filter_order():
    """a ~ b, b ~ c, a !~ c at rows 63, 64, 65: b is dropped and protects nobody, so c is kept; and a 130-row chain in which
    exactly the even rows are kept and every odd row's leader is the row below it."""
    three = ["()()....", "()()()..", "..()()()"]                                 # distances a-b 1, b-c 2, a-c 3
    res = check([["." * 8] * 63, three], radius=2)
    assert res.keep[63:].tolist() == [True, False, True] and res.leader[63:].tolist() == [63, 63, 65] and res.neighbours[63:].tolist() == [2, 3, 2]
    arr = np.full((1, 66, 8), -1, np.int32)
    arr[0, :63, 0] = 0                                                           # 63 invalid rows of the same group before them
    arr[0, 63:] = [partners_of(r) for r in three]
    one = gpu(arr, radius=2, strict=False)
    check_result(as_lists(one), naive([[None] * 63 + three], "radius", 2))
    assert one.keep[63:].tolist() == [True, False, True] and one.leader.tolist() == [-1] * 63 + [63, 63, 65]
    for kw in (dict(radius=2), dict(relative=0.5)):
        chain = check([chain_rows(130)], **kw)
        assert chain.keep.tolist() == [k % 2 == 0 for k in range(130)] and chain.leader.tolist() == [k - k % 2 for k in range(130)]
        assert chain.neighbours.tolist() == [2] + [3] * 128 + [2]


def test_the_numpy_path_is_the_naive_reference_at_the_small_shapes():
    rows = family_rows(3, 150, 9, families=6, edits=2)
    for groups in ([rows], split(rows, [70, 0, 80])):
        for kw in (dict(radius=1), dict(relative=0.34)):
            check_result(as_lists(host(groups, **kw)), naive(groups, *threshold_of(kw)))


def test_more_planned_tiles_than_blocks():
    """One group of 64 * 63 + 1 rows: 64 * 65 / 2 = 2080 planned tiles for at most 2048 blocks, against the numpy path."""
    tile, _, blocks = consts()
    S = tile * 63 + 1
    from squarna_amd.distances import plan_tiles
    assert len(plan_tiles([0, S])) == 2080 > blocks
    rows = family_rows(11, S, 9, families=40, edits=2)
    import torch
    for kw in (dict(radius=1), dict(relative=0.34)):
        got, ref = gpu([rows], **kw), host([rows], **kw)
        for key in ("status", "npairs", "neighbours", "leader", "keep", "common"):   # (16 million cells: compared as tensors)
            assert torch.equal(getattr(got, key).cpu(), getattr(ref, key)), (kw, key)


@pytest.mark.parametrize("S", [4097, 8193, 16385, 32769, 65535])
def test_the_filter_kernels_words_per_lane(S):
    """The row counts at which a lane of the filter kernel holds 2, 4, 8 and 16 words of a row, and the most rows, against a
    closed form: the first H = ceil(S / 2) rows are all different (row r holds the pair (2 i, 2 i + 1) for every set bit i of
    r) and row r >= H repeats row r - H, so under radius 0 exactly the first H rows are kept and row r is led by r mod H,
    far below it in the bit matrix."""
    import torch
    H = (S + 1) // 2
    code = np.arange(S, dtype=np.int64) % H
    bits = (code[:, None] >> np.arange(16)) & 1                                  # [S, 16]
    arr = np.full((S, 32), -1, np.int32)
    arr[:, 0::2] = np.where(bits == 1, np.arange(1, 32, 2), -1)
    arr[:, 1::2] = np.where(bits == 1, np.arange(0, 32, 2), -1)
    res = gpu(torch.from_numpy(arr.reshape(1, S, 32)).cuda(), radius=0, matrix=False)
    rows = np.arange(S)
    assert res.common is None and not res.status.any()
    assert res.npairs.cpu().numpy().tolist() == bits.sum(1).tolist()
    assert res.keep.cpu().numpy().tolist() == (rows < H).tolist() and res.leader.cpu().numpy().tolist() == code.tolist()
    assert res.neighbours.cpu().numpy().tolist() == (1 + (rows + H < S) + (rows >= H)).tolist()
    far = gpu(torch.from_numpy(arr.reshape(1, S, 32)).cuda(), radius=1, matrix=False)   # rows 0 and 1 (codes 0 and 1) are one pair apart
    assert far.keep[:4].tolist() == [True, False, False, True] and far.leader[:4].tolist() == [0, 0, 0, 3]


def _raw(dtype_sizes):
    """Device buffers filled with a sentinel (249 in bytes, -7 otherwise) for direct calls of the entry."""
    import torch
    return [torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda") for dt, n in dtype_sizes]


def _untouched(t):
    return bool((t == (249 if t.element_size() == 1 else -7)).all())


def _tables(groups, pad_rows=0):
    """The device tables of a direct call for groups of dot-bracket rows (None: an invalid row), and the plan."""
    import torch
    from squarna_amd.distances import plan_tiles
    rows = [r for g in groups for r in g]
    W = max(len(r) for r in rows if r is not None)
    flat = np.full((len(rows), W), -1, np.int32)
    for q, r in enumerate(rows):
        flat[q, :W if r is None else len(r)] = 0 if r is None else partners_of(r)   # (an invalid row: column 0 is its own partner)
    sizes = [len(g) for g in groups]
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(partner=up(flat.reshape(-1)), start=up(np.arange(len(rows), dtype=np.int64) * W),
                width=up(np.array([W if r is None else len(r) for r in rows], np.int32)), group=up(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)),
                goff=up(off), moff=up(np.concatenate(([0], np.cumsum(np.diff(off.astype(np.int64)) ** 2)))), tiles=up(plan_tiles(off)),
                S=len(rows), W=W, G=len(sizes), nmax=max(sizes), cells=int(sum(n * n for n in sizes)))


def test_direct_calls_write_nothing_beyond_their_rows():
    import torch
    from squarna_amd import _lib
    lib = _lib.load()
    pad = 16
    rows = family_rows(70, 133, 67, families=5, knots=True)
    rows[5] = rows[40] = rows[69] = None
    groups = split(rows, [3, 0, 67, 63])                                          # group 2 crosses the tile border, group 3 ends the rows
    exp = naive(groups, "radius", 3)
    t = _tables(groups)
    S, W, T = t["S"], t["W"], int(t["tiles"].shape[0])
    nbytes = lib.sq_structure_distances_scratch(S, W, T)
    assert T == 5 and nbytes == (8 * 2 * 192 + 133 * 3) * 8                       # open + 7 span planes, two words of columns, 192 padded rows; 133 x 3 words
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    for matrix in (True, False):
        scratch, status, npairs, common, nb, leader, keep, out = _raw([(torch.int64, nbytes // 8 + pad), (torch.int32, S + pad), (torch.int32, S + pad),
                                                                       (torch.int32, t["cells"] + pad), (torch.int32, S + pad), (torch.int32, S + pad),
                                                                       (torch.uint8, S + pad), (torch.int64, 2 + pad)])
        tail = (p(t["partner"]), int(t["partner"].numel()), p(t["start"]), p(t["width"]), p(t["group"]), S, W, p(t["goff"]), p(t["moff"]), t["G"],
                t["nmax"], p(t["tiles"]), T, 0, 3, p(scratch), nbytes, p(status), p(npairs), p(common if matrix else None),
                t["cells"] if matrix else 0, p(nb), p(leader), p(keep), p(out), None)

        def same():
            torch.cuda.synchronize()
            got = dict(status=status[:S].tolist(), npairs=npairs[:S].tolist(), neighbours=nb[:S].tolist(), leader=leader[:S].tolist(),
                       keep=[bool(x) for x in keep[:S].tolist()], common=common[:t["cells"]].tolist() if matrix else exp["common"])
            check_result(got, exp, matrix)
            assert set(keep[:S].tolist()) <= {0, 1} and out[:2].tolist() == [0, 0]
            for buf, n in ((scratch, nbytes // 8), (status, S), (npairs, S), (nb, S), (leader, S), (keep, S), (out, 2),
                           (common, t["cells"] if matrix else 0)):
                assert _untouched(buf[n:]), n

        assert lib.sq_structure_distances(*tail) == 0
        same()
        # the measuring entry: one kernel at a time on what the earlier ones left gives the same numbers again
        assert lib.sq_structure_distances_phases(0, *tail) == -1 and lib.sq_structure_distances_phases(8, *tail) == -1
        for phase in (1, 2, 4):
            assert lib.sq_structure_distances_phases(phase, *tail) == 0
            same()
    # an entry of the plan outside the tile range is skipped and reported; the other tiles are done
    bad = t["tiles"].clone()
    bad[1] = torch.tensor([2, 1], dtype=torch.int32)                                # (tile (0, 1): groups 2's rows 3 .. 63 against 64 .. 69)
    tail = tail[:11] + (p(bad),) + tail[12:]
    assert lib.sq_structure_distances(*tail) == 0
    torch.cuda.synchronize()
    assert out[:2].tolist() == [0, 1] and status[:S].tolist() == exp["status"] and nb[:3].tolist() == exp["neighbours"][:3]
    assert _untouched(scratch[nbytes // 8:]) and _untouched(nb[S:]) and _untouched(leader[S:]) and _untouched(keep[S:])


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib, device_calls as dc
    lib = _lib.load()
    groups = [family_rows(1, 9, 20)]
    t = _tables(groups)
    S, W, T = 9, 20, 1
    scr = lib.sq_structure_distances_scratch
    assert scr(0, 5, 1) == 0 and scr(5, 0, 1) == 0 and scr(5, 5, -1) == 0 and scr(5, 5, 2) == 0 and scr(65, 5, 4) == 0 and scr(65, 5, 3) > 0
    assert scr(dc.DISTANCES_MAX_ROWS + 1, 5, 1) == 0 and scr(5, dc.DISTANCES_MAX_COLS + 1, 1) == 0
    assert scr(dc.DISTANCES_MAX_ROWS, dc.DISTANCES_MAX_COLS, 1) == (16 * 512 * 65536 + 65535 * 1024) * 8
    nbytes = scr(S, W, T)
    assert nbytes == (6 * 1 * 64 + 9) * 8                                          # open + the 5 bits of 19
    bufs = _raw([(torch.int64, nbytes // 8), (torch.int32, S), (torch.int32, S), (torch.int32, S * S), (torch.int32, S), (torch.int32, S),
                 (torch.uint8, S), (torch.int64, 2)])
    scratch, status, npairs, common, nb, leader, keep, out = (ctypes.c_void_p(b.data_ptr()) for b in bufs)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    good = dict(partner=ptr(t["partner"]), plen=S * W, start=ptr(t["start"]), width=ptr(t["width"]), group=ptr(t["group"]), S=S, W=W,
                goff=ptr(t["goff"]), moff=ptr(t["moff"]), G=1, nmax=S, tiles=ptr(t["tiles"]), T=T, mode=0, thr=0, scratch=scratch, nbytes=nbytes,
                status=status, npairs=npairs, common=common, cells=S * S, nb=nb, leader=leader, keep=keep, out=out)
    order = tuple(good)
    for key, bad in (("partner", None), ("start", None), ("width", None), ("group", None), ("goff", None), ("moff", None), ("tiles", None),
                     ("scratch", None), ("status", None), ("npairs", None), ("nb", None), ("leader", None), ("keep", None), ("out", None),
                     ("plen", 0), ("S", 0), ("S", -1), ("S", dc.DISTANCES_MAX_ROWS + 1), ("W", 0), ("W", dc.DISTANCES_MAX_COLS + 1), ("G", 0),
                     ("nmax", 0), ("nmax", S + 1), ("T", 0), ("T", 2), ("mode", -1), ("mode", 2), ("thr", -1), ("common", None), ("cells", 0),
                     ("cells", -1), ("nbytes", nbytes - 8), ("nbytes", 0)):
        args = dict(good, **{key: bad})
        assert lib.sq_structure_distances(*(args[k] for k in order), None) == -1, (key, bad)
        assert (b"scratch" in lib.sq_last_error()) == (key == "nbytes"), key
    assert lib.sq_structure_distances(*(dict(good, mode=1, thr=10001)[k] for k in order), None) == -1
    torch.cuda.synchronize()
    for b in bufs:                                                                # nothing was launched, cleared or written
        assert _untouched(b)
    from squarna_amd import Distances
    with pytest.raises(ValueError, match="Distances"):
        Distances([["()"] * (dc.DISTANCES_MAX_ROWS + 1)], matrix=False)
    with pytest.raises(ValueError, match="Distances"):
        Distances([["." * (dc.DISTANCES_MAX_COLS + 1)]])


def test_a_cuda_tensor_is_used_where_it_is_and_other_integer_types_are_accepted():
    import torch
    from squarna_amd import engine as E
    groups = split(family_rows(21, 40, 30, families=3, knots=True), [13, 0, 20, 7])
    ref = as_lists(host(groups, radius=2))
    K = max(len(g) for g in groups)
    arr = np.full((len(groups), K, 30), -1, np.int32)
    for r, g in enumerate(groups):
        for k, dbn in enumerate(g):
            arr[r, k] = partners_of(dbn)
    nstruct = [len(g) for g in groups]
    dev = torch.from_numpy(arr).cuda()
    seen = []
    eng = E.get_engine()
    real = eng.structure_distances
    try:
        eng.structure_distances = lambda partner, *a, **kw: (seen.append(partner.data_ptr()), real(partner, *a, **kw))[1]
        res = gpu(dev, nstruct=nstruct, radius=2)
    finally:
        del eng.structure_distances
    assert seen == [dev.data_ptr()] and as_lists(res) == ref
    for form in (arr, arr.astype(np.int16), arr.astype(np.int64), dev.long(), dev.short(), torch.tensor(nstruct)):
        kw = dict(nstruct=form) if form.ndim == 1 else dict(nstruct=nstruct)
        assert as_lists(gpu(dev if form.ndim == 1 else form, radius=2, **kw)) == ref
    assert as_lists(gpu(groups, radius=2)) == ref
    empty = gpu(dev, nstruct=[0, 0, 0, 0])
    assert empty.S == 0 and empty.status.is_cuda and empty.kept().tolist() == []
    strict = arr.copy()
    strict[2, 4, 3] = 3
    with pytest.raises(ValueError, match=r"Distances: record 2 \(>record3\), row 4"):
        gpu(torch.from_numpy(strict).cuda(), nstruct=nstruct)


def test_distances_of_a_fold_equal_the_host_built_result():
    from squarna_amd import Fold
    from squarna_amd.inputs import ParseDefaultInput
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recs = list(ParseDefaultInput(os.path.join(root, "squarna_amd", "data", "datasets", "SRtest150.fas"), "qf"))[:6]
    fold = Fold(records=[(r[0], r[1], None, None, None) for r in recs], configfile="nobpp")
    for kw in (dict(radius=4), dict(relative=0.2, groups="all")):
        res = gpu(fold, **kw)
        ref = host(fold.cpu(), **kw)
        assert res.device == fold.device and res.names == ref.names == list(fold.names) and res.S == len(fold) + int(fold.nstruct.sum())
        assert as_lists(res) == as_lists(ref) and res.row_off.tolist() == ref.row_off.tolist()
        assert res.medoid().tolist() == ref.medoid().tolist() and res.mean_distance().tolist() == ref.mean_distance().tolist()
        assert res.neighbours_at(**{k: v for k, v in kw.items() if k != "groups"}).tolist() == res.neighbours.tolist()
        assert [t.tolist() for t in res.clusters()] == [t.tolist() for t in ref.clusters()] and res.nearest(0)[1].tolist() == ref.nearest(0)[1].tolist()
