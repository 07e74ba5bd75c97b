"""GPU tests of FoldMutants() and its device entry sq_variant_diff: the mutational scan whose summary is formed on the device,
against the CPU-built result under the OracleEngine and the plain-Python restatement of tests/fold_mutants_checks.py (set
differences of the rows' sets of pairs, a per-position comparison and count).  All comparisons are exact."""
import ctypes
import random

import pytest

from tests.fold_mutants_checks import (LETTERS, check_equal, check_result, expected_flat, nested_row, pack_records, pair_set, perturbed,
                                       random_row, random_seq)

pytestmark = pytest.mark.gpu


def _explicit_case():
    seq = random_seq(63, 50)
    other = lambda p, step=1: LETTERS[(LETTERS.index(seq[p]) + step) % 4]
    variants = [[[(4, other(4)), (40, other(40, 2).lower())], [(17, other(17, 3))], [(9, seq[9])]]]
    return dict(records=[("wt", seq, None, None, None)], variants=variants, configfile="greedynobpp"), dict(variants=variants)


CALLS = {"three_records": lambda: (dict(records=[random_seq(61, 40), random_seq(62, 65), random_seq(64, 130)], configfile="greedynobpp"), {}),
         "one_nobpp": lambda: (dict(inputseq=random_seq(65, 70), configfile="nobpp"), {}),
         "explicit": _explicit_case}


@pytest.mark.parametrize("tag", sorted(CALLS))
def test_result_stays_on_the_device_and_equals_the_cpu_built_one(tag):
    from squarna_amd import FoldMutants, engine as E
    from tests.oracle_engine import OracleEngine
    kw, given = CALLS[tag]()
    res = FoldMutants(**kw)
    assert res.source == "device" and res.device.type == "cuda" and res.folds.partner.is_cuda and res.folds.source == "device"
    assert all(getattr(res, key).is_cuda for key in res._TENSORS)
    _, per_rec = check_result(res, **given)
    assert any(d[3] > 0 for mine in per_rec for d in mine)
    if tag == "explicit":
        assert res.diff[2].tolist()[:2] == [0, 0] and res.diff[2].tolist()[3:] == [0, -1, -1]
    with E.use_engine(OracleEngine()):
        exp = FoldMutants(**kw)
    assert exp.source == "host"
    check_equal(res, exp)


def _upload(partner, cell_off, lengths, pos_off, wt_of):
    import torch
    t = lambda a, dt: torch.tensor(a, dtype=dt).cuda()
    return dict(partner=t(partner, torch.int32), cell_off=t(cell_off, torch.int64), lengths=t(lengths, torch.int64),
                pos_off=t(pos_off, torch.int64), wt_rec=t(wt_of, torch.int32))


WT_LENGTHS = [1, 2, 63, 64, 65, 128, 129, 300]


def _synthetic(seed, extra):
    """Wild types of WT_LENGTHS with 1, 3, 4 and 5 variants, the wild types interleaved in the variants' order."""
    rng = random.Random(seed)
    wt_rows = [random_row(rng, n) for n in WT_LENGTHS]
    order = [(rng.random(), r) for r, count in enumerate([1, 3, 4, 5, 1, 3, 4, 5]) for _ in range(count)]
    wt_of = [r for _, r in sorted(order)]
    var_rows = [perturbed(rng, wt_rows[r]) if rng.random() < 0.8 else random_row(rng, len(wt_rows[r])) for r in wt_of]
    return wt_rows, var_rows, wt_of, pack_records(rng, wt_rows, var_rows, wt_of, extra=extra)


@pytest.mark.parametrize("extra", [0, 2])
def test_diff_against_the_sets(extra):
    import torch
    from squarna_amd.engine import HipEngine
    wt_rows, var_rows, wt_of, (partner, cell_off, lengths, rec0, pos_off, Ltot) = _synthetic(11 + extra, extra)
    assert rec0 == len(WT_LENGTHS) + extra and sorted(set(wt_of)) == list(range(8)) and wt_of != sorted(wt_of)
    assert any(cell_off[r + 1] - cell_off[r] > lengths[r] for r in range(len(lengths)))          # (row 0 is not the whole record)
    t = _upload(partner, cell_off, lengths, pos_off, wt_of)
    diff, pos_changed = HipEngine().variant_diff(t["partner"], t["cell_off"], t["lengths"], rec0, t["wt_rec"], t["pos_off"], Ltot)
    assert diff.is_cuda and pos_changed.is_cuda and (diff.dtype, pos_changed.dtype) == (torch.int32, torch.int32)
    assert tuple(diff.shape) == (len(wt_of), 6) and tuple(pos_changed.shape) == (Ltot,)
    exp_diff, exp_pos = expected_flat(wt_rows, var_rows, wt_of)
    assert diff.tolist() == exp_diff and pos_changed.tolist() == exp_pos
    assert max(d[5] for d in exp_diff) > 128 and sum(d[0] > 0 for d in exp_diff) > 10 and sum(d[1] > 0 for d in exp_diff) > 10


def test_more_variants_than_the_grid():
    """One fully nested 20-nt wild type, every variant all-unpaired: every variant changes every position, so all the atomic
    additions of the call go to the same 20 words."""
    import torch
    from squarna_amd import device_calls
    from squarna_amd.engine import HipEngine
    V = 4 * 4 * device_calls.VARIANT_DIFF_MAX_BLOCKS + 37                    # (4 waves per block: four grid strides and a rest)
    partner = torch.cat((torch.tensor(nested_row(20), dtype=torch.int32), torch.full((20 * V,), -1, dtype=torch.int32))).cuda()
    cell_off = (torch.arange(V + 2, dtype=torch.int64) * 20).cuda()
    lengths = torch.full((V + 1,), 20, dtype=torch.int64).cuda()
    wt_rec = torch.zeros(V, dtype=torch.int32).cuda()
    pos_off = torch.tensor([0, 20], dtype=torch.int64).cuda()
    diff, pos_changed = HipEngine().variant_diff(partner, cell_off, lengths, 1, wt_rec, pos_off, 20)
    assert tuple(diff.shape) == (V, 6)
    assert bool((diff == torch.tensor([10, 0, 0, 20, 0, 19], dtype=torch.int32).cuda()).all())
    assert pos_changed.tolist() == [V] * 20


def test_no_variant_and_identical_rows():
    import torch
    from squarna_amd.engine import HipEngine
    eng = HipEngine()
    rng = random.Random(3)
    wt_rows = [random_row(rng, n, density=0.9) for n in (30, 64, 131)]
    wt_of = [0, 1, 1, 2, 0]
    var_rows = [list(wt_rows[r]) for r in wt_of]
    partner, cell_off, lengths, rec0, pos_off, Ltot = pack_records(rng, wt_rows, var_rows, wt_of)
    t = _upload(partner, cell_off, lengths, pos_off, wt_of)
    diff, pos_changed = eng.variant_diff(t["partner"], t["cell_off"], t["lengths"], rec0, t["wt_rec"], t["pos_off"], Ltot)
    npairs = [len(pair_set(w)) for w in wt_rows]
    assert min(npairs) > 5 and diff.tolist() == [[0, 0, npairs[r], 0, -1, -1] for r in wt_of] and pos_changed.tolist() == [0] * Ltot
    diff, pos_changed = eng.variant_diff(t["partner"], t["cell_off"], t["lengths"], rec0, t["wt_rec"][:0], t["pos_off"], Ltot)
    assert tuple(diff.shape) == (0, 6) and diff.dtype == torch.int32 and pos_changed.tolist() == [0] * Ltot


def _raw_call(t, rec0, Ltot):
    import torch
    from squarna_amd import _lib
    V = int(t["wt_rec"].numel())
    diff = torch.full((V, 6), -7, dtype=torch.int32).cuda()
    pos_changed = torch.full((Ltot,), -7, dtype=torch.int32).cuda()
    out = torch.full((2,), -7, dtype=torch.int64).cuda()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = _lib.load().sq_variant_diff(p(t["partner"]), p(t["cell_off"]), p(t["lengths"]), rec0, V, p(t["wt_rec"]), p(t["pos_off"]), Ltot,
                                     p(diff), p(pos_changed), p(out), None)
    torch.cuda.synchronize()
    return rc, diff, pos_changed, out


def test_invalid_entry_gives_status_2():
    from squarna_amd.engine import HipEngine
    rng = random.Random(8)
    wt_rows = [random_row(rng, 90), random_row(rng, 70)]
    wt_of = [0, 1, 0, 0, 1]
    var_rows = [perturbed(rng, wt_rows[r]) for r in wt_of]
    exp_diff, exp_pos = expected_flat(wt_rows, var_rows, wt_of)
    row = var_rows[2]
    a = [q for q, p in enumerate(row) if p == -1][0]
    b = [q for q, p in enumerate(row) if p > q][0]
    row[a] = b                                                              # (a points at b, b at its own partner)
    partner, cell_off, lengths, rec0, pos_off, Ltot = pack_records(rng, wt_rows, var_rows, wt_of)
    t = _upload(partner, cell_off, lengths, pos_off, wt_of)
    with pytest.raises(RuntimeError, match="sq_variant_diff"):
        HipEngine().variant_diff(t["partner"], t["cell_off"], t["lengths"], rec0, t["wt_rec"], t["pos_off"], Ltot)
    rc, diff, pos_changed, out = _raw_call(t, rec0, Ltot)
    assert rc == 0 and out.tolist() == [0, 2]
    assert [diff[m].tolist() for m in (0, 1, 3, 4)] == [exp_diff[m] for m in (0, 1, 3, 4)]
    assert pos_changed[90:].tolist() == exp_pos[90:]                        # (the other wild type's counts are whole)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib
    L = _lib.load()
    buf = torch.full((64,), 5, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    calls = [(p, p, p, -1, 1, p, p, 40, p, p, p, None),                      # rec0 below 0
             (p, p, p, 1, -1, p, p, 40, p, p, p, None),                      # a negative number of variants
             (p, p, p, 1, 1, p, p, 0, p, p, p, None),                        # no position
             (p, p, p, 1, 1, p, p, -3, p, p, p, None),                       # a negative number of positions
             (p, p, p, 1, 1, p, p, 2 ** 31, p, p, p, None),                  # 2^31 positions
             (None, p, p, 1, 1, p, p, 40, p, p, p, None),                    # no table
             (p, None, p, 1, 1, p, p, 40, p, p, p, None),                    # no offsets
             (p, p, None, 1, 1, p, p, 40, p, p, p, None),                    # no lengths
             (p, p, p, 1, 1, None, p, 40, p, p, p, None),                    # no wild types
             (p, p, p, 1, 1, p, None, 40, p, p, p, None),                    # no positions' offsets
             (p, p, p, 1, 1, p, p, 40, None, p, p, None),                    # no result rows
             (p, p, p, 1, 1, p, p, 40, p, None, p, None),                    # no counts per position
             (p, p, p, 1, 0, p, p, 40, p, None, p, None),                    # ... also without a variant
             (p, p, p, 1, 1, p, p, 40, p, p, None, None)]                    # no result words
    for args in calls:
        assert L.sq_variant_diff(*args) == -1
        assert b"sq_variant_diff" in L.sq_last_error()
    torch.cuda.synchronize()
    assert buf.tolist() == [5] * 64
