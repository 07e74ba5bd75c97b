"""GPU tests of Project() / Lift() and their device entries (sq_project_rows, sq_lift_rows) against the naive reference of
tests/project_checks.py (plain loops over characters) and the numpy path built under the OracleEngine.  All comparisons are
exact.  The shapes are the smallest at which each part can go wrong: L around the 64-column chunk, around the two chunks and
around the four chunks a block's waves walk at a time, rows that are all gaps, have no gap or have gaps only in the first or
last chunk, one row of more than 64 chunks (a lane of the base scan then sums two chunks), and one more row than blocks."""
import ctypes

import numpy as np
import pytest

from squarna_amd.device_calls import PROJECT_MAX_BLOCKS
from tests.project_checks import (GAP_CHARS, WIDTHS, aligned_rows, check_equal, class_line, lift_lists, naive, naive_lift, project_lists,
                                  short_lines, special_rows, structure_line)

pytestmark = pytest.mark.gpu
ALI = "examples/ali_input.afa"
PROJECT_KEYS = ("length", "col_of", "pos_of", "partner", "cls", "counts", "status")
LIFT_KEYS = ("length", "col_of", "pos_of", "partner", "status", "nstruct")


def gpu_project(**kw):
    from squarna_amd import Project
    res = Project(**kw)
    assert res.source == "device" and all(getattr(res, k).is_cuda for k in PROJECT_KEYS)
    return res


def gpu_lift(**kw):
    from squarna_amd import Lift
    res = Lift(**kw)
    assert res.source == "device" and all(getattr(res, k).is_cuda for k in LIFT_KEYS)
    return res


def host(entry, **kw):
    import squarna_amd
    from squarna_amd import engine as E
    from tests.oracle_engine import OracleEngine
    with E.use_engine(OracleEngine()):
        res = getattr(squarna_amd, entry)(**kw)
    assert res.source == "host"
    return res


def same_tensors(got, ref, keys):
    for key in keys:
        a, b = getattr(got, key), getattr(ref, key)
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and a.cpu().tolist() == b.tolist(), key


def padded(short, width=None):
    K = max(max(len(mine) for mine in short), 1)
    width = max(max((len(p) for mine in short for p in mine), default=0), 1) if width is None else width
    out = np.full((len(short), K, width), -1, np.int32)
    for r, mine in enumerate(short):
        for k, p in enumerate(mine):
            out[r, k, :len(p)] = p
    return out


@pytest.mark.parametrize("L", WIDTHS)
def test_shapes_against_the_naive_reference_and_the_numpy_path(L):
    rows = aligned_rows(L, 6, L) + special_rows(L)
    for K in (1, 3):
        shared = [structure_line(10 * L + k, L, knots=k == 1) for k in range(K)]
        per_row = [[class_line(row)] + [structure_line(100 * L + 10 * r + k, L) for k in range(K - 1)] for r, row in enumerate(rows)]
        for lines in (shared, per_row):
            for canonical_only, min_loop in ((False, 0), (True, 3), (False, L)):
                kw = dict(sequences=rows, structures=np.array(lines), canonical_only=canonical_only, min_loop=min_loop)
                res = gpu_project(**kw)
                check_equal(project_lists(res), naive(rows, lines, canonical_only, min_loop), (L, K, canonical_only, min_loop))
                same_tensors(res, host("Project", **kw), PROJECT_KEYS)
        short = short_lines(L + K, rows, K, knots=True)
        res = gpu_lift(sequences=rows, structures=padded(short))
        check_equal(lift_lists(res, [K] * len(rows)), naive_lift(rows, short), (L, K, "lift"))
        same_tensors(res, host("Lift", sequences=rows, structures=padded(short)), LIFT_KEYS)
        back = gpu_project(sequences=rows, structures=res.partner)              # the round trip, on the device throughout
        assert back.partner.cpu().tolist() == padded(short, int(back.partner.shape[2])).tolist()


def test_a_row_of_more_than_sixty_four_chunks():
    L = 4097
    rows = aligned_rows(9, 2, L) + [("GA-CU." * 700)[:L]]
    inner = structure_line(1, L - 2, knots=True)
    lines = [[L - 1] + [p + 1 if p >= 0 else -1 for p in inner] + [0], class_line(rows[0])]   # a pair across the whole row
    for kw in (dict(), dict(canonical_only=True, min_loop=5)):
        res = gpu_project(sequences=rows, structures=np.array(lines), **kw)
        check_equal(project_lists(res), naive(rows, lines, kw.get("canonical_only", False), kw.get("min_loop", 0)), kw)
    short = short_lines(4, rows, 2, knots=True)
    res = gpu_lift(sequences=rows, structures=padded(short))
    check_equal(lift_lists(res, [2] * 3), naive_lift(rows, short))


def test_more_rows_than_blocks():
    R, L = PROJECT_MAX_BLOCKS + 1, 70
    rows = aligned_rows(70, R, L)
    lines = [structure_line(5, L, knots=True)]
    res = gpu_project(sequences=rows, structures=np.array(lines), min_loop=1)
    check_equal(project_lists(res), naive(rows, lines, False, 1))
    short = short_lines(6, rows, 1)
    lifted = gpu_lift(sequences=rows, structures=padded(short))
    check_equal(lift_lists(lifted, [1] * R), naive_lift(rows, short))


def test_an_alignment_on_the_device_is_read_where_it_is():
    from squarna_amd import Covariation, FoldAlignment, engine as E
    a = FoldAlignment(inputfile=ALI)
    assert a.steps.is_cuda
    seen = []
    eng = E.get_engine()
    real = eng.project_rows
    try:
        eng.project_rows = lambda rows, structs, *args, **kw: (seen.append(structs.data_ptr()), real(rows, structs, *args, **kw))[1]
        res = gpu_project(alignment=a)
        one = gpu_project(alignment=a, step=2)
    finally:
        del eng.project_rows
    assert seen == [a.steps.data_ptr(), a.steps[1].data_ptr()] and res.device == a.steps.device
    ref = host("Project", alignment=a.cpu())
    assert (res.K, res.shared, res.names) == (3, True, ref.names)
    same_tensors(res, ref, PROJECT_KEYS)
    same_tensors(one, host("Project", alignment=a.cpu(), step=2), PROJECT_KEYS)
    check_equal(project_lists(res), naive(a.sequences, a.steps.cpu().tolist()))
    assert res.kept_fraction().cpu().tolist() == ref.kept_fraction().tolist() and res.worst_rows(1).cpu().tolist() == ref.worst_rows(1).tolist()
    for step in (1, 2, 3):
        pairs = a.pairs(step)
        cov = Covariation(alignment=a, pairs=pairs)
        v = [p[0] for p in pairs]
        assert res.support(step - 1)[v].tolist() == cov.bp_rows.tolist() and res.contradicting(step - 1)[v].tolist() == cov.incompatible.tolist()
    assert res.dbn(0, 2) == ref.dbn(0, 2)


def test_lift_of_a_fold_equals_the_host_built_result():
    from squarna_amd import Distances, Fold, Score
    from squarna_amd.covariation import _read_alignment
    names, seqs = _read_alignment(ALI, "unknown", "qtrf", False)
    ungapped = ["".join(ch for ch in s if ch not in GAP_CHARS) for s in seqs]
    fold = Fold(records=ungapped, configfile="nobpp")
    assert fold.partner.is_cuda
    res = gpu_lift(inputfile=ALI, structures=fold)
    ref = host("Lift", inputfile=ALI, structures=fold.cpu())
    same_tensors(res, ref, LIFT_KEYS)
    assert res.nstruct.cpu().tolist() == (1 + fold.nstruct).cpu().tolist() and res.names == names
    assert res.pair_frequency(1).cpu().tolist() == ref.pair_frequency(1).tolist() and res.dbn(3, 1) == ref.dbn(3, 1)
    back = gpu_project(inputfile=ALI, structures=res.partner)
    top = fold.to_padded()                                                      # the structures, without the consensus
    assert back.partner[:, 1:, :].cpu().tolist() == top[:, :, :].cpu().tolist()
    scored = Score(records=ungapped, structures=back.to_padded(), nstruct=res.nstruct)
    assert not scored.status.any()
    dist = Distances(res.to_padded(), nstruct=res.nstruct, groups="all")
    assert dist.S == int(res.nstruct.sum()) and not dist.status.any()


def _raw(dtype_sizes):
    """Device buffers filled with a sentinel (249 in bytes, -7 otherwise) for direct calls of the entries."""
    import torch
    return [torch.full((n,), 249 if dt == torch.uint8 else -7, dtype=dt, device="cuda") for dt, n in dtype_sizes]


def _untouched(t):
    return bool((t == (249 if t.element_size() == 1 else -7)).all())


def _bytes(rows):
    import torch
    return torch.from_numpy(np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), len(rows[0])).copy()).cuda()


def test_direct_calls_write_nothing_beyond_their_rows():
    import torch
    from squarna_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    R, L, K, pad = 7, 131, 2, 37
    rows = aligned_rows(3, R - 1, L) + ["-" * L]
    exp_len = [sum(ch not in GAP_CHARS for ch in row) for row in rows]
    Lmax = max(exp_len)
    d_rows = _bytes(rows)
    lines = [structure_line(2, L, knots=True), class_line(rows[1])]
    bad = list(lines[1])
    bad[5] = 5
    per_row = [[lines[0], bad if r == 2 else lines[1]] for r in range(R)]
    for structs, stride in ((lines, 0), (per_row, K * L)):
        d_structs = torch.tensor(structs, dtype=torch.int32).cuda().contiguous()
        sizes = [(torch.int32, R), (torch.int32, R * Lmax), (torch.int32, R * L), (torch.int32, R * K * Lmax), (torch.uint8, R * K * L),
                 (torch.int32, R * K * 12), (torch.int32, R * K)]
        bufs = _raw([(dt, n + pad) for dt, n in sizes])
        assert lib.sq_project_rows(p(d_rows), R, L, p(d_structs), stride, K, Lmax, 0, 2, *(p(b) for b in bufs), None) == 0
        torch.cuda.synchronize()
        for b, (_, n) in zip(bufs, sizes):
            assert _untouched(b[n:]) and not bool((b[:n] == (249 if b.element_size() == 1 else -7)).any())
        exp = naive(rows, structs, False, 2)
        length, col_of, pos_of, partner, cls, counts, status = (b[:n].cpu() for b, (_, n) in zip(bufs, sizes))
        assert length.tolist() == exp["length"] and pos_of.view(R, L).tolist() == exp["pos_of"] and status.view(R, K).tolist() == exp["status"]
        assert cls.view(R, K, L).tolist() == exp["cls"] and counts.view(R, K, 12).tolist() == exp["counts"]
        assert [row[:n] for row, n in zip(partner.view(R, K, Lmax)[:, 0].tolist(), exp_len)] == [q[0] for q in exp["partner"]]
        assert status.view(R, K)[2].tolist() == ([0, 0] if stride == 0 else [0, 1])
    # a caller whose Lmax is too small: the rows that do not fit get status 2 and no structure, and nothing is written
    # beyond the buffers
    small = sorted(exp_len)[3]
    sizes = [(torch.int32, R), (torch.int32, R * small), (torch.int32, R * L), (torch.int32, R * K * small), (torch.uint8, R * K * L),
             (torch.int32, R * K * 12), (torch.int32, R * K)]
    bufs = _raw([(dt, n + pad) for dt, n in sizes])
    d_structs = torch.tensor(lines, dtype=torch.int32).cuda()
    assert lib.sq_project_rows(p(d_rows), R, L, p(d_structs), 0, K, small, 0, 0, *(p(b) for b in bufs), None) == 0
    torch.cuda.synchronize()
    for b, (_, n) in zip(bufs, sizes):
        assert _untouched(b[n:])
    assert bufs[0][:R].tolist() == exp_len and bufs[6][:R * K].view(R, K)[:, 0].tolist() == [2 if n > small else 0 for n in exp_len]
    fit = naive(rows, lines)
    for r in range(R):
        got = bufs[3][:R * K * small].view(R, K, small)[r, 0].tolist()
        assert got == ([-1] * small if exp_len[r] > small else fit["partner"][r][0] + [-1] * (small - exp_len[r]))
    # the lift: lines of a stride wider than the rows, fewer lines than K, one row whose lines lie outside the buffer
    short = short_lines(8, rows, K, knots=True)
    width = Lmax + 3
    flat = torch.from_numpy(padded(short, width)).cuda().contiguous().view(-1)
    start = torch.arange(R, dtype=torch.int64) * K * width
    start[4] = flat.numel() - width                                             # room for one line, two are asked for
    nstruct = torch.tensor([2, 1, 0, 2, 2, 2, 2], dtype=torch.int32)
    stride = torch.full((R,), width, dtype=torch.int32)
    sizes = [(torch.int32, R), (torch.int32, R * Lmax), (torch.int32, R * L), (torch.int32, R * K * L), (torch.int32, R * K)]
    bufs = _raw([(dt, n + pad) for dt, n in sizes])
    assert lib.sq_lift_rows(p(d_rows), R, L, p(flat), flat.numel(), p(start.cuda()), p(stride.cuda()), p(nstruct.cuda()), K, Lmax,
                            *(p(b) for b in bufs), None) == 0
    torch.cuda.synchronize()
    for b, (_, n) in zip(bufs, sizes):
        assert _untouched(b[n:]) and not bool((b[:n] == -7).any())
    exp = naive_lift(rows, short)
    partner, status = bufs[3][:R * K * L].view(R, K, L).cpu().tolist(), bufs[4][:R * K].view(R, K).cpu().tolist()
    assert status == [[0, 0], [0, 0], [0, 0], [0, 0], [2, 2], [0, 0], [0, 0]]
    for r, n in enumerate(nstruct.tolist()):
        for k in range(K):
            assert partner[r][k] == (exp["partner"][r][k] if k < n and r != 4 else [-1] * L), (r, k)
    assert bufs[1][:R * Lmax].view(R, Lmax).cpu().tolist() == [c + [-1] * (Lmax - len(c)) for c in exp["col_of"]]


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import Lift, Project, _lib, device_calls as dc
    lib = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    R, L, K, Lmax = 3, 20, 2, 20
    d_rows = _bytes(aligned_rows(1, R, L))
    d_structs = torch.full((K, L), -1, dtype=torch.int32, device="cuda")
    bufs = _raw([(torch.int32, R), (torch.int32, R * Lmax), (torch.int32, R * L), (torch.int32, R * K * Lmax), (torch.uint8, R * K * L),
                 (torch.int32, R * K * 12), (torch.int32, R * K)])
    good = dict(rows=ptr(d_rows), R=R, L=L, structs=ptr(d_structs), stride=0, K=K, Lmax=Lmax, canonical=0, min_loop=0, length=ptr(bufs[0]),
                col_of=ptr(bufs[1]), pos_of=ptr(bufs[2]), partner=ptr(bufs[3]), cls=ptr(bufs[4]), counts=ptr(bufs[5]), status=ptr(bufs[6]))
    order = tuple(good)
    assert lib.sq_project_rows(*(good[k] for k in order), None) == 0
    torch.cuda.synchronize()
    assert not any(_untouched(b) for b in bufs)
    bufs2 = _raw([(torch.int32, R), (torch.int32, R * Lmax), (torch.int32, R * L), (torch.int32, R * K * Lmax), (torch.uint8, R * K * L),
                  (torch.int32, R * K * 12), (torch.int32, R * K)])
    good.update(length=ptr(bufs2[0]), col_of=ptr(bufs2[1]), pos_of=ptr(bufs2[2]), partner=ptr(bufs2[3]), cls=ptr(bufs2[4]),
                counts=ptr(bufs2[5]), status=ptr(bufs2[6]))
    for key, bad in (("rows", None), ("structs", None), ("length", None), ("col_of", None), ("pos_of", None), ("partner", None), ("cls", None),
                     ("counts", None), ("status", None), ("R", 0), ("R", -1), ("R", dc.PROJECT_MAX_ROWS + 1), ("L", 0),
                     ("L", dc.PROJECT_MAX_COLS + 1), ("K", 0), ("K", -1), ("Lmax", 0), ("Lmax", dc.PROJECT_MAX_COLS + 1), ("stride", L),
                     ("stride", -1), ("canonical", 2), ("min_loop", -1)):
        args = dict(good, **{key: bad})
        assert lib.sq_project_rows(*(args[k] for k in order), None) == -1, (key, bad)
        assert b"sq_project_rows" in lib.sq_last_error()
    short = torch.full((R * K * Lmax,), -1, dtype=torch.int32, device="cuda")
    start = (torch.arange(R, dtype=torch.int64) * K * Lmax).cuda()
    stride, nstruct = torch.full((R,), Lmax, dtype=torch.int32, device="cuda"), torch.full((R,), K, dtype=torch.int32, device="cuda")
    lift = dict(rows=ptr(d_rows), R=R, L=L, short=ptr(short), short_len=short.numel(), start=ptr(start), stride=ptr(stride),
                nstruct=ptr(nstruct), K=K, Lmax=Lmax, length=ptr(bufs2[0]), col_of=ptr(bufs2[1]), pos_of=ptr(bufs2[2]),
                partner=ptr(bufs2[3]), status=ptr(bufs2[6]))
    order = tuple(lift)
    for key, bad in (("rows", None), ("short", None), ("start", None), ("stride", None), ("nstruct", None), ("length", None), ("col_of", None),
                     ("pos_of", None), ("partner", None), ("status", None), ("short_len", 0), ("R", 0), ("R", dc.PROJECT_MAX_ROWS + 1), ("L", 0),
                     ("L", dc.PROJECT_MAX_COLS + 1), ("K", 0), ("Lmax", 0), ("Lmax", dc.PROJECT_MAX_COLS + 1)):
        args = dict(lift, **{key: bad})
        assert lib.sq_lift_rows(*(args[k] for k in order), None) == -1, (key, bad)
        assert b"sq_lift_rows" in lib.sq_last_error()
    torch.cuda.synchronize()
    for b in bufs2:                                                             # nothing was launched, cleared or written
        assert _untouched(b)
    with pytest.raises(ValueError, match="Project"):
        Project(sequences=["A" * (dc.PROJECT_MAX_COLS + 1)], structures=np.full(dc.PROJECT_MAX_COLS + 1, -1))
    with pytest.raises(ValueError, match="Lift"):
        Lift(sequences=["A" * (dc.PROJECT_MAX_COLS + 1)], structures=np.full((1, 1, dc.PROJECT_MAX_COLS + 1), -1))


def test_cuda_tensors_and_other_integer_types():
    import torch
    from squarna_amd import engine as E
    L = 90
    rows = aligned_rows(12, 9, L)
    lines = [structure_line(1, L), structure_line(2, L, knots=True)]
    ref = project_lists(host("Project", sequences=rows, structures=np.array(lines)))
    dev = torch.tensor(lines, dtype=torch.int32).cuda()
    seen = []
    eng = E.get_engine()
    real = eng.project_rows
    try:
        eng.project_rows = lambda r, structs, *args, **kw: (seen.append(structs.data_ptr()), real(r, structs, *args, **kw))[1]
        res = gpu_project(sequences=rows, structures=dev)
    finally:
        del eng.project_rows
    assert seen == [dev.data_ptr()] and project_lists(res) == ref
    for form in (dev.short(), dev.long(), np.array(lines, np.int16), np.array(lines, np.int64), dev[None].expand(9, 2, L).contiguous().long()):
        assert project_lists(gpu_project(sequences=rows, structures=form)) == ref
    short = padded(short_lines(2, rows, 2))
    ref = host("Lift", sequences=rows, structures=short, nstruct=[2, 1, 0, 2, 2, 2, 1, 2, 2])
    d_short = torch.from_numpy(short).cuda()
    for form in (d_short, d_short.short(), d_short.long(), short.astype(np.int64)):
        same_tensors(gpu_lift(sequences=rows, structures=form, nstruct=[2, 1, 0, 2, 2, 2, 1, 2, 2]), ref, LIFT_KEYS)
    strict = np.array(lines)
    strict[1, 7] = 7
    with pytest.raises(ValueError, match=r"Project: row 0 \(>record1\), line 1"):
        gpu_project(sequences=rows, structures=torch.from_numpy(strict).cuda())
    res = gpu_project(sequences=rows, structures=torch.from_numpy(strict).cuda(), strict=False)
    assert res.status.cpu().tolist() == [[0, 1]] * 9 and bool((res.partner[:, 1] == -1).all()) and not bool(res.counts[:, 1].any())
