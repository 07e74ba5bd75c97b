"""GPU tests of FoldWindows() and its device entry sq_window_pair_count: the windowed mode whose pair table, rank order and
consensus are formed on the device, against the CPU-built result under the OracleEngine and the plain-Python restatement
of tests/fold_windows_checks.py (a dict count, the coverage by enumeration, a sorted() key, a sequential first fit).
All comparisons are exact."""
import ctypes
import random

import pytest

from tests.fold_windows_checks import (LIMITS, REAL, check_equal, check_result, check_views, cover_enum, cover_sorted, expected_global,
                                       first_fit, pack_tables, random_seq, synthetic_windows)

pytestmark = pytest.mark.gpu


def _three_records():
    rng = random.Random(9)
    reacts = [round(rng.random(), 3) for _ in range(400)]
    ref = "((((((......))))))" + "." * 32
    recs = [("long", random_seq(1, 400), reacts, None, None), ("short", random_seq(4, 50), None, "." * 50, ref),
            ("edge", random_seq(5, 61), None, None, None)]
    return dict(records=recs, window=60, step=7, configfile="greedynobpp", freqlimit=0.2), [None, ref, None]


def _inputs(tag):
    if tag == "three_records":
        return _three_records()
    seq, window, step, conf = REAL[tag]
    return dict(inputseq=seq, window=window, step=step, configfile=conf), None


@pytest.mark.parametrize("tag", sorted(REAL) + ["three_records"])
def test_result_stays_on_the_device_and_equals_the_cpu_built_one(tag):
    from squarna_amd import FoldWindows, engine as E
    from tests.oracle_engine import OracleEngine
    kw, refs = _inputs(tag)
    res = FoldWindows(**kw)
    assert res.source == "device" and res.device.type == "cuda" and res.windows.partner.is_cuda and res.windows.source == "device"
    assert all(getattr(res, key).is_cuda for key in res._TENSORS)
    Ltot = int(res.pos_off[-1])
    assert len(res.first_fit_rounds) == 1 and 1 <= res.first_fit_rounds[0] <= Ltot // 2 + 1
    tables = check_result(res, refs)
    assert sum(len(t) for t in tables) > 200
    check_views(res, tables)
    with E.use_engine(OracleEngine()):
        exp = FoldWindows(**kw)
    assert exp.source == "host"
    check_equal(res, exp)


def _device_tables(Ns, window, step, seed, nested=False, rec0=0):
    import torch
    rng = random.Random(seed)
    gstart, lens, rows, per_rec = synthetic_windows(rng, Ns, window, step, nested=nested)
    partner, cell_off = pack_tables(rows, rng, rec0)
    t = dict(partner=torch.tensor(partner, dtype=torch.int32).cuda(), cell_off=torch.tensor(cell_off, dtype=torch.int64).cuda(),
             starts=torch.tensor(gstart, dtype=torch.int64).cuda(), lens=torch.tensor(lens, dtype=torch.int32).cuda())
    return t, per_rec


def _as_dict(out, Ltot):
    flat, count, cover, first = (x.tolist() for x in out)
    table = {divmod(f, Ltot): (c, cov, k) for f, c, cov, k in zip(flat, count, cover, first)}
    assert len(table) == len(flat), "a pair was given twice"
    return table


SHAPES = {"30_8_3": ([30], 8, 3), "257_64_1": ([257], 64, 1), "600_65_7": ([600], 65, 7), "mixed_64_5": ([1, 2, 63, 64, 65, 300], 64, 5),
          "three_40_40": ([90, 20, 75], 40, 40), "700_300_11": ([700], 300, 11)}                # (windows of more than one 256-thread pass)


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_count_against_the_dict(tag):
    import torch
    from squarna_amd.engine import HipEngine
    Ns, window, step = SHAPES[tag]
    for rec0 in (0, 2):
        t, per_rec = _device_tables(Ns, window, step, 11 + rec0, rec0=rec0)
        out = HipEngine().window_pair_count(t["partner"], t["cell_off"], rec0, t["starts"], t["lens"], sum(Ns))
        assert [x.dtype for x in out] == [torch.int64, torch.int32, torch.int32, torch.int32] and all(x.is_cuda for x in out)
        exp = expected_global(per_rec, Ns)
        assert _as_dict(out, sum(Ns)) == exp and (len(exp) > 0) == (max(Ns) > 1)


@pytest.mark.parametrize("N,window,step", [(5000, 150, 5), (12000, 150, 1)])
def test_nested_windows_many_records_per_block(N, window, step):
    """Every window holds the same nested pairs, so nearly every entry is a pair of its own: 971 windows give tens of thousands
    of records (a block stages its two windows' and flushes once); 11,851 windows over the kernel's 512 blocks give ~1,700
    records per block -- the 1,024-record stage is flushed twice on the way and once at the end."""
    from squarna_amd.engine import HipEngine
    t, per_rec = _device_tables([N], window, step, 3, nested=True)
    assert int(t["starts"].numel()) == len(per_rec[0][0]) == {5: 971, 1: 11851}[step]
    out = HipEngine().window_pair_count(t["partner"], t["cell_off"], 0, t["starts"], t["lens"], N)
    exp = expected_global(per_rec, [N], cover=cover_sorted)
    assert len(exp) == {5: 72825, 1: 888825}[step]
    assert _as_dict(out, N) == exp
    s, wlen, _ = per_rec[0]
    assert all(cover_enum(i, j, s, wlen) == cov for (i, j), (_, cov, _) in list(exp.items())[::997])


def test_all_unpaired_and_no_window():
    import torch
    from squarna_amd.engine import HipEngine
    eng = HipEngine()
    starts = torch.arange(0, 300, 10, dtype=torch.int64).cuda()
    lens = torch.full((30,), 50, dtype=torch.int32).cuda()
    partner = torch.full((30 * 50,), -1, dtype=torch.int32).cuda()
    cell_off = torch.arange(0, 31 * 50, 50, dtype=torch.int64).cuda()
    out = eng.window_pair_count(partner, cell_off, 0, starts, lens, 340)
    assert [int(x.numel()) for x in out] == [0, 0, 0, 0]
    out = eng.window_pair_count(partner, cell_off, 0, starts[:0], lens[:0], 340)
    assert [int(x.numel()) for x in out] == [0, 0, 0, 0]


def test_cap_below_the_count():
    """The entry reports the true number and writes nothing beyond cap; the method's repeat then returns all."""
    import torch
    from squarna_amd import _lib
    from squarna_amd.engine import HipEngine
    Ns = [600]
    t, per_rec = _device_tables(Ns, 65, 7, 21)
    exp = expected_global(per_rec, Ns)
    cap = 40
    assert len(exp) > 3 * cap
    L = _lib.load()
    flat = torch.full((cap + 64,), -7, dtype=torch.int64).cuda()
    small = [torch.full((cap + 64,), -7, dtype=torch.int32).cuda() for _ in range(3)]
    out = torch.full((2,), -7, dtype=torch.int64).cuda()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = L.sq_window_pair_count(p(t["partner"]), p(t["cell_off"]), 0, int(t["starts"].numel()), p(t["starts"]), p(t["lens"]), 600,
                                p(flat), p(small[0]), p(small[1]), p(small[2]), cap, p(out), None)
    torch.cuda.synchronize()
    assert rc == 0 and out.tolist() == [len(exp), 0]
    assert flat[cap:].tolist() == [-7] * 64 and all(x[cap:].tolist() == [-7] * 64 for x in small)
    got = _as_dict([flat[:cap]] + [x[:cap] for x in small], 600)
    assert len(got) == cap and all(exp[bp] == v for bp, v in got.items())
    out = HipEngine().window_pair_count(t["partner"], t["cell_off"], 0, t["starts"], t["lens"], 600, cap=cap)
    assert _as_dict(out, 600) == exp


def test_rank_order_and_first_fit_on_the_concatenated_axis():
    """The device sort into the rank order and ONE first fit for all records, against the sorted() key and the sequential pass
    per record, at the five limits."""
    import torch
    from squarna_amd.engine import HipEngine
    from squarna_amd.fold_windows import _rank_order, _within_records
    from tests.fold_windows_checks import by_cell_only, ranked_table
    eng = HipEngine()
    ties_matter = 0
    for seed, (Ns, window, step) in enumerate([([300, 64, 1, 257], 64, 5), ([600], 65, 7), ([90, 20, 75, 400], 40, 3), ([257, 30], 64, 1)]):
        t, per_rec = _device_tables(Ns, window, step, 40 + seed)
        Ltot, T = sum(Ns), int(t["starts"].numel())
        flat, count, cover, first = eng.window_pair_count(t["partner"], t["cell_off"], 0, t["starts"], t["lens"], Ltot)
        pos_off = torch.tensor([sum(Ns[:r]) for r in range(len(Ns) + 1)], dtype=torch.int64).cuda()
        rec = torch.searchsorted(pos_off, flat // Ltot, right=True) - 1
        freq = count.double() / cover.double()
        order = _rank_order(torch, rec, freq, count, first, flat, T)
        tables = [ranked_table(mine, s, wlen) for s, wlen, mine in per_rec]
        exp, k0 = [], 0
        for r, (table, (s, wlen, mine)) in enumerate(zip(tables, per_rec)):
            off = sum(Ns[:r])
            exp += [((off + i) * Ltot + off + j, c, cov, k0 + f) for i, j, c, cov, f in table]
            k0 += len(s)
        got = list(zip(flat[order].tolist(), count[order].tolist(), cover[order].tolist(), first[order].tolist()))
        assert got == exp, (Ns, window, step)
        for lim in LIMITS:
            part, info = eng.first_fit(flat[order][freq[order] >= lim], Ltot, 0)
            status, rounds, npairs, live = info.tolist()
            assert status == 0 and live == 0 and rounds <= Ltot // 2 + 1
            want = [first_fit(table, lim, N) for table, N in zip(tables, Ns)]
            assert _within_records(torch, part, pos_off).tolist() == [p for row in want for p in row], (Ns, lim)
            ties_matter += any(first_fit(table, lim, N, key=by_cell_only) != w for table, N, w in zip(tables, Ns, want))
    assert ties_matter >= 1, "no case in which the order of equal frequencies matters"


def test_asymmetric_entry_gives_status_2():
    import torch
    from squarna_amd import _lib
    from squarna_amd.engine import HipEngine
    Ns = [120]
    t, per_rec = _device_tables(Ns, 30, 4, 8)
    s, wlen, mine = per_rec[0]
    k = 5
    free = [q for q, p in enumerate(mine[k]) if p == -1]
    paired = [q for q, p in enumerate(mine[k]) if p > q]
    a, b = free[0], paired[0]
    partner = t["partner"].clone()
    partner[int(t["cell_off"][k]) + a] = b                                  # (a points at b, b at its own partner)
    mine[k][a] = b                                                         # (the dict count skips the entry: row[b] != a)
    exp = expected_global(per_rec, Ns)
    with pytest.raises(RuntimeError, match="sq_window_pair_count"):
        HipEngine().window_pair_count(partner, t["cell_off"], 0, t["starts"], t["lens"], 120)
    cap = len(exp) + 8
    flat = torch.empty(cap, dtype=torch.int64).cuda()
    small = [torch.empty(cap, dtype=torch.int32).cuda() for _ in range(3)]
    out = torch.empty(2, dtype=torch.int64).cuda()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = _lib.load().sq_window_pair_count(p(partner), p(t["cell_off"]), 0, len(s), p(t["starts"]), p(t["lens"]), 120, p(flat), p(small[0]),
                                          p(small[1]), p(small[2]), cap, p(out), None)
    torch.cuda.synchronize()
    assert rc == 0 and out.tolist() == [len(exp), 2]
    assert _as_dict([flat[:len(exp)]] + [x[:len(exp)] for x in small], 120) == exp   # (the rest is counted)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib
    L = _lib.load()
    buf = torch.full((64,), 5, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    calls = [(p, p, -1, 1, p, p, 40, p, p, p, p, 4, p, None),                # rec0 below 0
             (p, p, 0, -1, p, p, 40, p, p, p, p, 4, p, None),                # a negative number of windows
             (p, p, 0, 1, p, p, 0, p, p, p, p, 4, p, None),                  # no position
             (p, p, 0, 1, p, p, 2 ** 31, p, p, p, p, 4, p, None),            # 2^31 positions
             (p, p, 0, 1, p, p, 40, p, p, p, p, -1, p, None),                # a negative cap
             (p, p, 0, 1, p, p, 40, None, p, p, p, 4, p, None),              # no result buffer
             (p, p, 0, 1, p, p, 40, p, p, p, p, 4, None, None),              # no result words
             (None, p, 0, 1, p, p, 40, p, p, p, p, 4, p, None),              # no table
             (p, p, 0, 1, None, p, 40, p, p, p, p, 4, p, None)]              # no starts
    for args in calls:
        assert L.sq_window_pair_count(*args) == -1
        assert b"sq_window_pair_count" in L.sq_last_error()
    torch.cuda.synchronize()
    assert buf.tolist() == [5] * 64
