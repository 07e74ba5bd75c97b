"""GPU tests of FoldDuplex() and its device entry sq_duplex_summary: the interaction screen whose summary is formed on the
device, against the CPU-built result under the OracleEngine and the plain-Python restatement of tests/fold_duplex_checks.py
(subsets of the duplex row's set of pairs, the solo rows' pairs it lacks, a per-position count).  All comparisons are exact."""
import ctypes
import random

import pytest

from tests.fold_duplex_checks import (BOUNDARY_LENGTHS, ROW_KINDS, check_equal, check_result, duplex_row, expected_summary, pack_tables,
                                      random_row, random_seq, revcomp)

pytestmark = pytest.mark.gpu

T0 = "GGGGCUAAAAGCCCCAAAAAAUCAGGUCAUCG"
TARGETS = [T0, random_seq(71, 64), random_seq(72, 90)]
QUERIES = [revcomp(T0[2:14]), revcomp(TARGETS[1][20:34]), random_seq(73, 20), "A" * 10]
SMALL = [random_seq(81, 40), random_seq(82, 65), random_seq(83, 30)], [random_seq(84, 21), revcomp(random_seq(82, 65)[10:31]), "U" * 12]
# the screen at its ordinary size: duplexes of 278-323 nt, the list form of the pool round kernel on the bit words of
# sq_bits_direct_kernel (several 256-diagonal tiles per word-row)
LONG_TARGETS = [random_seq(91, 300), random_seq(92, 257)]
LONG_QUERIES = [revcomp(LONG_TARGETS[0][140:162]), random_seq(93, 21), "A" * 20]

CALLS = {"screen": lambda: (dict(targets=TARGETS, queries=QUERIES, configfile="greedynobpp"), TARGETS, QUERIES),
         "interchainonly_long_targets": lambda: (dict(targets=LONG_TARGETS, queries=LONG_QUERIES, configfile="greedynobpp", interchainonly=True),
                                                 LONG_TARGETS, LONG_QUERIES),
         "three_by_three_nobpp": lambda: (dict(targets=SMALL[0], queries=SMALL[1], configfile="nobpp"), SMALL[0], SMALL[1]),
         "interchainonly": lambda: (dict(targets=TARGETS, queries=QUERIES, configfile="greedynobpp", interchainonly=True), TARGETS, QUERIES)}


@pytest.mark.parametrize("tag", sorted(CALLS))
def test_result_stays_on_the_device_and_equals_the_cpu_built_one(tag):
    from squarna_amd import FoldDuplex, engine as E
    from tests.oracle_engine import OracleEngine
    kw, targets, queries = CALLS[tag]()
    pairs = [(a, b) for a in range(len(targets)) for b in range(len(queries))]
    res = FoldDuplex(**kw)
    assert res.source == "device" and res.device.type == "cuda"
    assert res.solos.partner.is_cuda and res.folds.partner.is_cuda and res.solos.source == res.folds.source == "device"
    assert all(getattr(res, key).is_cuda for key in res._TENSORS)
    _, _, summary = check_result(res, targets, queries, pairs)
    assert any(s[0] > 0 for s in summary) and any(s[3] > 0 for s in summary)
    if tag.startswith("interchainonly"):
        assert all(s[1] == 0 and s[2] == 0 for s in summary)
    if tag == "screen":
        assert summary[0][:4] == [12, 0, 0, 6] and all(summary[4 * a + 3][0] == 0 and summary[4 * a + 3][3] == 0 for a in range(3))
    with E.use_engine(OracleEngine()):
        exp = FoldDuplex(**kw)
    assert exp.source == "host"
    check_equal(res, exp)


def test_targets_against_themselves_and_no_pair():
    from squarna_amd import FoldDuplex
    res = FoldDuplex(targets=TARGETS[:2], homodimers=True, configfile="greedynobpp")
    assert res.source == "device"
    check_result(res, TARGETS[:2], None, [(0, 0), (0, 1), (1, 1)])
    one = FoldDuplex(targets=TARGETS[:1], configfile="greedynobpp")
    assert one.source == "device" and one.bound.is_cuda
    check_result(one, TARGETS[:1], None, [])


def _upload(t, a_of, b_of):
    """The tables of pack_tables as device tensors; one allocation when the packer made one table."""
    import torch
    up = lambda a, dt: torch.tensor(a, dtype=dt).cuda()
    partner_s = up(t["partner_s"], torch.int32)
    if t["same"]:                                                           # (views of ONE table: offsets and lengths from the first duplex on)
        partner_d = partner_s
    else:
        partner_d = up(t["partner_d"], torch.int32)
    return dict(partner_s=partner_s, cell_off_s=up(t["cell_off_s"], torch.int64), lengths_s=up(t["lengths_s"], torch.int64),
                partner_d=partner_d, cell_off_d=up(t["cell_off_d"], torch.int64), lengths_d=up(t["lengths_d"], torch.int64),
                a_rec=up(a_of, torch.int32), b_rec=up(b_of, torch.int32), pos_off=up(t["pos_off"], torch.int64))


def _call(eng, d, Ltot):
    return eng.duplex_summary(d["partner_s"], d["cell_off_s"], d["lengths_s"], d["partner_d"], d["cell_off_d"], d["lengths_d"], d["a_rec"],
                              d["b_rec"], d["pos_off"], Ltot)


def _synthetic(seed):
    """One solo record per boundary length; every length is chain A and chain B of some duplex, with every kind of row, a
    homodimer per length, the duplexes in no order of their chains."""
    rng = random.Random(seed)
    solo_rows = [random_row(rng, n, 0.8) for n in BOUNDARY_LENGTHS]
    ns = len(solo_rows)
    pairs = [(a, (a * 3 + shift) % ns) for a in range(ns) for shift in (1, 4, 6)] + [(a, a) for a in range(ns)]
    rng.shuffle(pairs)
    dup_rows = [duplex_row(rng, ROW_KINDS[k % len(ROW_KINDS)], solo_rows[a], solo_rows[b]) for k, (a, b) in enumerate(pairs)]
    return rng, solo_rows, dup_rows, [a for a, _ in pairs], [b for _, b in pairs]


@pytest.mark.parametrize("one_table", [True, False])
def test_summary_against_the_sets(one_table):
    import torch
    from squarna_amd.engine import HipEngine
    rng, solo_rows, dup_rows, a_of, b_of = _synthetic(19 + one_table)
    assert set(a_of) == set(b_of) == set(range(len(BOUNDARY_LENGTHS))) and a_of != sorted(a_of) and b_of != sorted(b_of)
    t = pack_tables(rng, solo_rows, dup_rows, one_table=one_table, unrelated=2)
    assert all(t["cell_off_s"][r + 1] - t["cell_off_s"][r] > t["lengths_s"][r] for r in range(len(solo_rows)) if t["lengths_s"][r])
    d = _upload(t, a_of, b_of)
    assert (d["partner_d"].data_ptr() == d["partner_s"].data_ptr()) == one_table
    summary, bound = _call(HipEngine(), d, t["Ltot"])
    assert summary.is_cuda and bound.is_cuda and (summary.dtype, bound.dtype) == (torch.int32, torch.int32)
    assert tuple(summary.shape) == (len(a_of), 9) and tuple(bound.shape) == (t["Ltot"],)
    exp_summary, exp_bound = expected_summary(solo_rows, dup_rows, a_of, b_of)
    assert summary.tolist() == exp_summary and bound.tolist() == exp_bound
    assert all(any(r[c] > 0 for r in exp_summary) for c in range(5)) and max(r[6] for r in exp_summary) > 128
    assert max(r[7] for r in exp_summary) > 64 and any(r[3] > 0 and r[0] == 0 for r in exp_summary)


def test_more_duplexes_than_the_grid():
    """One 9-nt hairpin A fully paired to one 9-nt hairpin B in every duplex: all the atomic additions of the call go to the
    same 18 words."""
    import torch
    from squarna_amd import device_calls
    from squarna_amd.engine import HipEngine
    P = 4 * 4 * device_calls.DUPLEX_SUMMARY_MAX_BLOCKS + 37                  # (4 waves per block: four grid strides and a rest)
    A, B = [8, 7, 6, -1, -1, -1, 2, 1, 0], [-1, 7, 6, -1, -1, -1, 2, 1, -1]
    D = [18 - t for t in range(9)] + [-1] + [8 - u for u in range(9)]
    assert expected_summary([A, B], [D], [0], [1]) == ([[9, 0, 0, 3, 2, 0, 8, 0, 8]], [1] * 18)
    partner_s = torch.tensor(A + B, dtype=torch.int32).cuda()
    cell_off_s = torch.tensor([0, 9, 18], dtype=torch.int64).cuda()
    lengths_s = torch.tensor([9, 9], dtype=torch.int64).cuda()
    partner_d = torch.tensor(D, dtype=torch.int32).repeat(P).cuda()
    cell_off_d = (torch.arange(P + 1, dtype=torch.int64) * 19).cuda()
    lengths_d = torch.full((P,), 19, dtype=torch.int64).cuda()
    a_rec, b_rec = torch.zeros(P, dtype=torch.int32).cuda(), torch.ones(P, dtype=torch.int32).cuda()
    pos_off = torch.tensor([0, 9, 18], dtype=torch.int64).cuda()
    summary, bound = HipEngine().duplex_summary(partner_s, cell_off_s, lengths_s, partner_d, cell_off_d, lengths_d, a_rec, b_rec, pos_off, 18)
    assert tuple(summary.shape) == (P, 9)
    assert bool((summary == torch.tensor([9, 0, 0, 3, 2, 0, 8, 0, 8], dtype=torch.int32).cuda()).all())
    assert bound.tolist() == [P] * 18


def test_no_duplex_and_identical_empty_rows():
    import torch
    from squarna_amd.engine import HipEngine
    eng = HipEngine()
    rng = random.Random(3)
    solo_rows = [[-1] * n for n in (30, 64, 131)]
    a_of, b_of = [0, 1, 1, 2, 0], [1, 1, 2, 0, 0]
    dup_rows = [[-1] * (len(solo_rows[a]) + 1 + len(solo_rows[b])) for a, b in zip(a_of, b_of)]
    t = pack_tables(rng, solo_rows, dup_rows)
    d = _upload(t, a_of, b_of)
    summary, bound = _call(eng, d, t["Ltot"])
    assert summary.tolist() == [[0, 0, 0, 0, 0, -1, -1, -1, -1]] * 5 and bound.tolist() == [0] * t["Ltot"]
    none = dict(d, a_rec=d["a_rec"][:0], b_rec=d["b_rec"][:0])
    for tables in (none, dict(none, partner_d=None, cell_off_d=None, lengths_d=None)):
        summary, bound = _call(eng, tables, t["Ltot"])
        assert tuple(summary.shape) == (0, 9) and summary.dtype == torch.int32 and bound.tolist() == [0] * t["Ltot"]


def _raw_call(d, Ltot):
    import torch
    from squarna_amd import _lib
    P = int(d["a_rec"].numel())
    summary = torch.full((P, 9), -7, dtype=torch.int32).cuda()
    bound = torch.full((Ltot,), -7, dtype=torch.int32).cuda()
    out = torch.full((2,), -7, dtype=torch.int64).cuda()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = _lib.load().sq_duplex_summary(p(d["partner_s"]), p(d["cell_off_s"]), p(d["lengths_s"]), int(d["lengths_s"].numel()), p(d["partner_d"]),
                                       p(d["cell_off_d"]), p(d["lengths_d"]), P, p(d["a_rec"]), p(d["b_rec"]), p(d["pos_off"]), Ltot,
                                       p(summary), p(bound), p(out), None)
    torch.cuda.synchronize()
    return rc, summary, bound, out


def test_invalid_entry_gives_status_2():
    from squarna_amd.engine import HipEngine
    rng = random.Random(8)
    solo_rows = [random_row(rng, 90), random_row(rng, 70), random_row(rng, 50)]
    a_of, b_of = [0, 2, 0, 1, 2], [1, 2, 1, 1, 0]
    dup_rows = [duplex_row(rng, kind, solo_rows[a], solo_rows[b]) for kind, a, b in zip(("bind", "random", "dropped", "inter_only", "bind"), a_of, b_of)]
    exp_summary, exp_bound = expected_summary(solo_rows, dup_rows, a_of, b_of)
    row = dup_rows[3]                                                       # (chains 1 and 1: solo record 1 alone is touched)
    a = [q for q, p in enumerate(row) if p == -1 and q != 70][0]
    b = [q for q, p in enumerate(row) if p > q][0]
    row[a] = b                                                              # (a points at b, b at its own partner)
    t = pack_tables(rng, solo_rows, dup_rows, unrelated=1)
    d = _upload(t, a_of, b_of)
    with pytest.raises(RuntimeError, match="sq_duplex_summary"):
        _call(HipEngine(), d, t["Ltot"])
    rc, summary, bound, out = _raw_call(d, t["Ltot"])
    assert rc == 0 and out.tolist() == [0, 2]
    assert [summary[k].tolist() for k in (0, 1, 2, 4)] == [exp_summary[k] for k in (0, 1, 2, 4)]
    others = expected_summary(solo_rows, [dup_rows[k] for k in (0, 1, 2, 4)], [a_of[k] for k in (0, 1, 2, 4)], [b_of[k] for k in (0, 1, 2, 4)])[1]
    assert bound[:90].tolist() == others[:90] and bound[160:].tolist() == others[160:]     # (the untouched solos' counts are whole)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib
    L = _lib.load()
    buf = torch.full((64,), 5, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    good = [p, p, p, 1, p, p, p, 1, p, p, p, 40, p, p, p, None]
    change = lambda at, value: good[:at] + [value] + good[at + 1:]
    calls = [change(3, -1),                                                  # a negative number of solo records
             change(7, -1),                                                  # a negative number of duplexes
             change(11, 0), change(11, -3), change(11, 2 ** 31)]             # no position, a negative number, 2^31 positions
    calls += [change(at, None) for at in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)]      # every pointer a duplex needs
    none = change(7, 0)
    calls += [none[:13] + [None] + none[14:], none[:14] + [None] + none[15:]]             # no counts / no result words, also without a duplex
    for args in calls:
        assert L.sq_duplex_summary(*args) == -1
        assert b"sq_duplex_summary" in L.sq_last_error()
    torch.cuda.synchronize()
    assert buf.tolist() == [5] * 64
