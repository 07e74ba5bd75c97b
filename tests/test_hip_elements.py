"""GPU tests of Elements() / HipEngine.elements_tensors / sq_elements_rows: the annotation of given structures on the device,
against the literal table of the specification, the naive reference of tests/elements_checks.py, the CPU path of Elements
on the same rows and the ranking tail's own levels of a fold.  All comparisons are exact (integers)."""
import os

import numpy as np
import pytest

from tests import elements_checks as EC
from tests import score_checks as SC
from tests.fold_checks import DATA

pytestmark = pytest.mark.gpu


def _cpu_elements(**kw):
    from squarna_amd import Elements
    from squarna_amd import engine as E
    from tests.oracle_engine import OracleEngine
    with E.use_engine(OracleEngine()):
        return Elements(**kw)


def _is_device(res):
    import torch
    assert res.source == "device"
    for key in res._TENSORS:
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.is_cuda, key
    assert res.element.dtype == torch.int8 and res.level.dtype == torch.int16 and res.loop_of.dtype == torch.int32
    assert res.loops.dtype == torch.int32 and res.loop_off.dtype == torch.int64 and res.cell_off.dtype == torch.int64


@pytest.fixture
def kernel_calls(monkeypatch):
    """Every HipEngine.elements_tensors call of the test: (the partner tensor's address, whether it is on the GPU, the kernels'
    own status as it left the device -- BEFORE Elements hands status-2 rows to the host)."""
    from squarna_amd.engine import HipEngine
    seen, inner = [], HipEngine.elements_tensors

    def spy(self, records, partner, row_start, row_rec):
        out = inner(self, records, partner, row_start, row_rec)
        seen.append((partner.data_ptr(), partner.is_cuda, out["status"].cpu().tolist()))
        return out
    monkeypatch.setattr(HipEngine, "elements_tensors", spy)
    return seen


def _none_handed_back(calls, results=()):
    """No row left the kernels with status 2: the device annotated them, not the host behind it."""
    assert calls
    for _, _, status in calls:
        assert 2 not in status
    assert all(res.recomputed == 0 for res in results)


def _single(dbn, seq=None):
    """Elements of one row on the device and on the CPU path; both, after the comparison with each other and the reference."""
    from squarna_amd import Elements
    seq = "A" * len(dbn) if seq is None else seq
    row = EC.partner_row(dbn) if isinstance(dbn, str) else dbn
    pad = np.asarray(row, np.int32)[None, None]
    res = Elements(records=[seq], structures=pad)
    _is_device(res)
    EC.equal_results(res, _cpu_elements(records=[seq], structures=pad))
    return res


def test_the_literal_table_on_the_device(kernel_calls):
    """The table in the three forms; the padded form is a CUDA tensor, which the kernels read where it is and leave unchanged."""
    import torch
    from squarna_amd import Elements
    cs = EC.table_cases()
    recs = [c["seq"] for c in cs]
    a = Elements(records=recs, structures=SC.strings_form(cs))
    padded, nstruct = SC.padded_form(cs, extra=5)
    dev = torch.from_numpy(padded).cuda()
    before = dev.clone()
    b = Elements(records=recs, structures=dev, nstruct=nstruct)
    assert kernel_calls[-1][:2] == (dev.data_ptr(), True) and torch.equal(dev, before)
    fr = SC.fold_result_form(cs, device="cuda")
    c = Elements(structures=fr)
    assert kernel_calls[-1][:2] == (fr.partner.data_ptr(), True) and len(kernel_calls) == 3
    _none_handed_back(kernel_calls, (a, b, c))
    for res in (a, b, c):
        _is_device(res)
        EC.check_table(res)


def test_mixed_records_in_one_call(kernel_calls):
    """Widths 0 to 263 around the wave, gaps, a separator and 0 to 6 rows of 0 to 6 crossing helices in ONE call: the naive
    reference, the CPU path, and one call per record."""
    from squarna_amd import Elements
    recs, rows = EC.mixed_records()
    assert [len(rec[1]) for rec in recs] == [0, 1, 63, 64, 65, 129, 263] and [len(r) for r in rows] == list(range(7))
    pad, nstruct = EC.padded(rows, extra=1)
    res = Elements(records=recs, structures=pad, nstruct=nstruct)
    _is_device(res)
    EC.check_naive(res, recs, rows)
    EC.equal_results(res, _cpu_elements(records=recs, structures=pad, nstruct=nstruct))
    host = res.cpu()
    for r, rec in enumerate(recs):
        one = Elements(records=[rec], structures=pad[r:r + 1], nstruct=nstruct[r:r + 1]).cpu()
        a, b = int(host.row_off[r]), int(host.row_off[r + 1])
        ca, cb, la, lb = (int(x) for x in (host.cell_off[a], host.cell_off[b], host.loop_off[a], host.loop_off[b]))
        assert one.element.tolist() == host.element[ca:cb].tolist() and one.level.tolist() == host.level[ca:cb].tolist(), rec[0]
        assert one.loop_of.tolist() == host.loop_of[ca:cb].tolist() and one.loops.tolist() == host.loops[la:lb].tolist(), rec[0]
        assert one.nlevels.tolist() == host.nlevels[a:b].tolist() and one.npairs.tolist() == host.npairs[a:b].tolist(), rec[0]
    _none_handed_back(kernel_calls, (res,))


def test_stems_at_the_chunk_boundaries(kernel_calls):
    """The levels kernel decides "starts a stem" at the first position of a chunk of 64 from the last lane of the chunk
    before, as the score kernels do: the golden rows of Score() that put stems across, up to and from positions 63 | 64 and
    127 | 128 -- stacked and not, 63 unpaired or a closer, behind gap columns, a pair dropped by a gap on the boundary --
    in ONE call against the naive reference and the CPU path."""
    from squarna_amd import Elements
    cs = [c for c in SC.cases() if c["name"].startswith("boundary_") or c["name"] == "gap_on_the_boundary_pair"]
    assert len(cs) == 7 and sum(len(c["rows"]) for c in cs) == 59 and sum("-" in c["seq"] for c in cs) == 4
    recs = [c["seq"] for c in cs]
    rows = [[SC.partner_row(row["dbn"]) for row in c["rows"]] for c in cs]
    pad, nstruct = EC.padded(rows, extra=1)
    res = Elements(records=recs, structures=pad, nstruct=nstruct)
    _is_device(res)
    _none_handed_back(kernel_calls, (res,))
    assert res.status.count_nonzero().item() == 0
    EC.check_naive(res, recs, rows)
    EC.equal_results(res, _cpu_elements(records=recs, structures=pad, nstruct=nstruct))
    assert res.npairs.tolist() == [sum(s[2] for s in row["stems"]) for c in cs for row in c["rows"]]


def test_random_rows_on_the_device(kernel_calls):
    from squarna_amd import Elements
    made = [EC.random_row(7 * w + k, w, k=k, gaps=g, sep=s) for w in (5, 30, 150) for k in range(7) for g, s in ((False, False), (True, True))]
    recs, rows = [seq for seq, _ in made], [[row] for _, row in made]
    res = Elements(records=recs, structures=EC.padded(rows)[0])
    EC.check_naive(res, recs, rows)
    _none_handed_back(kernel_calls, (res,))


def _ladder(npairs):
    """npairs single pairs that all cross one another: as many levels."""
    row = np.full(2 * npairs, -1, np.int32)
    row[:npairs], row[npairs:] = np.arange(npairs, 2 * npairs), np.arange(npairs)
    return row


def test_sixty_four_levels_stay_on_the_device(kernel_calls):
    res = _single(_ladder(64))
    _none_handed_back(kernel_calls, (res,))
    assert res.nlevels.tolist() == [64] and res.npairs.tolist() == [64] and res.text(0) == "S" + "K" * 63 + "S" + "K" * 63
    assert sorted(abs(v) for v in res.level.tolist()) == sorted(list(range(1, 65)) * 2)


def test_sixty_five_levels_come_back_from_the_host(kernel_calls):
    from squarna_amd import Elements
    row = _ladder(65)
    pad = np.stack([EC.partner_row("((..))".ljust(130, ".")), row, EC.partner_row("(...)".ljust(130, "."))])[None]
    res = Elements(records=["A" * 130], structures=pad)
    assert kernel_calls[-1][2] == [0, 2, 0] and res.recomputed == 1 and res.status.tolist() == [0, 0, 0]
    _is_device(res)
    assert res.nlevels.tolist() == [1, 65, 1] and res.nloops.tolist() == [2, 2, 2] and res.loop_off.tolist() == [0, 2, 4, 6]
    EC.check_naive(res, ["A" * 130], [list(pad[0])])
    EC.equal_results(res, _cpu_elements(records=["A" * 130], structures=pad))


@pytest.mark.parametrize("stems", [512, 513])
def test_the_register_and_the_lds_form_of_the_levels(kernel_calls, stems):
    """512 one-pair stems are levelled in registers, 513 in LDS (sq_stem_levels_wave); the first two stems cross."""
    dbn = "([.)]" + "(.)" * (stems - 2)
    res = _single(dbn)
    _none_handed_back(kernel_calls, (res,))
    assert res.nlevels.tolist() == [2] and res.npairs.tolist() == [stems] and res.dbn(0) == dbn
    EC.check_naive(res, ["A" * len(dbn)], [[EC.partner_row(dbn)]])


def test_more_loops_than_lanes(kernel_calls):
    """An exterior loop of 70 branches (71 loops), 70 bulges inside one another, a multiloop of 66 hairpins."""
    for dbn in ("(...)" * 70, "(." * 70 + "..." + ")" * 70, "(" + "(...)" * 66 + ")"):
        res = _single(dbn)
        EC.check_naive(res, ["A" * len(dbn)], [[EC.partner_row(dbn)]])
        assert int(res.nloops[0]) > 64
    _none_handed_back(kernel_calls)


def test_a_long_record(kernel_calls):
    """30,000 nt: the levels kernel's LDS is sized for 11,264 stems, beyond the 64 KB a launch gets unasked."""
    dbn = ("([.)]" + "(...)" * 50 + "((..((...))..((...))..))").ljust(30000, ".")
    res = _single(dbn)
    _none_handed_back(kernel_calls, (res,))
    assert res.nlevels.tolist() == [2] and res.nloops.tolist() == [1 + 1 + 50 + 3] and res.dbn(0) == dbn


def test_the_levels_are_the_ranking_tails(kernel_calls):
    """The fold's device tail computes the levels of its structures from its own stem log and prints them as brackets:
    Elements of the fold's rows must give the same strings."""
    from squarna_amd import Elements, Fold
    fold = Fold(inputfile=os.path.join(DATA, "datasets", "SRtest150.fas"), inputformat="qf", configfile="nobpp")
    res = Elements(structures=fold)
    _is_device(res)
    _none_handed_back(kernel_calls, (res,))
    assert kernel_calls[-1][0] == fold.partner.data_ptr()
    host, ro = res.cpu(), res.row_off.cpu().numpy()
    assert (np.diff(ro) == 1 + fold.nstruct.cpu().numpy()).all() and host.status.count_nonzero().item() == 0
    checked = 0
    for r in range(len(fold)):
        assert host.dbn(int(ro[r])) == fold.consensus(r), fold.names[r]
        for k in range(int(ro[r + 1] - ro[r]) - 1):
            assert host.dbn(int(ro[r]) + 1 + k) == fold.dbn(r, k), (fold.names[r], k)
            checked += 1
    assert checked > 200 and int(host.nlevels.max()) >= 2


def test_invalid_rows_on_the_device():
    from squarna_amd import Elements
    for name, seq, row in SC.INVALID:
        if name == "nothing_to_score":
            continue
        good = np.full(len(seq), -1, np.int32)
        pad = np.stack([good, np.asarray(row, np.int32)])[None]
        with pytest.raises(ValueError, match=r"^Elements: record 0 \(>r\), row 1"):
            Elements(records=[(">r", seq, None, None, None)], structures=pad)
        res = Elements(records=[(">r", seq, None, None, None)], structures=pad, strict=False)
        _is_device(res)
        EC.equal_results(res, _cpu_elements(records=[(">r", seq, None, None, None)], structures=pad, strict=False))
        assert res.status.tolist() == [0, 1] and res.text(1) == "?" * len(seq) and res.nloops.tolist() == [1, 0], name
    res = Elements(records=["-&-"], structures=[["..."]])
    assert res.status.tolist() == [0] and res.text(0) == "-&-"
