"""GPU tests of Fold() / HipEngine.fold_tensors / sq_result_pairs_dev: the results path that stays on the device, against
HipEngine.fold_records on the same records, the reference's output text (tests/golden/text/*.txt) and the CPU oracle.
All comparisons are exact: integers, and doubles bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.fold_checks import DATA, check_against_golden, check_against_tuples, check_dense_forms
from tests.test_hip_parity import conf
from tests.test_hip_parity2 import _chain_records

pytestmark = pytest.mark.gpu

RANKBY_R = (2, 0, 1)                     # Predict's (and Fold's) default rankby="r" (SQUARNA.py:810-820)


def _parse(inputfile, inputformat="qtrf"):
    from squarna_amd.inputs import ParseInput
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return list(ParseInput(None, inputfile, inputformat)[0])


def _engine_tuples(inputs, psets, **opts):
    """(tuples, reference scores) of HipEngine.fold_records for parsed input records."""
    from squarna_amd.engine import HipEngine
    eng = HipEngine()
    opts.setdefault("rankby", RANKBY_R)
    out = eng.fold_records([(rec[1], rec[2], rec[3], rec[4], psets, None) for rec in inputs], **opts)
    return out, eng.last_ref_scores


def _is_device(res):
    import torch
    for key in ("lengths", "nstruct", "row_off", "cell_off", "partner", "scores", "pset_mask", "metrics"):
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.is_cuda, key
    assert res.partner.dtype == torch.int32 and res.scores.dtype == torch.float64 and res.pset_mask.dtype == torch.int64
    assert res.metrics.dtype == torch.float64 and tuple(res.metrics.shape) == (len(res), 16)


def test_srtest150_nobpp_stays_on_the_device():
    """219 records with reference lines under all five algorithms: tensors on the GPU, formed by the device path, equal to
    fold_records' tuples (metrics and reference scores included) and to the structure lines the reference printed."""
    from squarna_amd import Fold
    path = os.path.join(DATA, "datasets", "SRtest150.fas")
    res = Fold(inputfile=path, inputformat="qf", configfile="nobpp")
    _is_device(res)
    assert res.source == "device" and len(res) == 219
    names, psets = conf("nobpp")
    assert all(pn == names for pn in res.paramset_names)
    tuples, refsc = _engine_tuples(_parse(path, "qf"), psets, keep=5)
    assert all(r is not None for r in refsc)
    check_against_tuples(res, tuples, keep=5, ref_scores=refsc)
    check_against_golden(res, "SRtest150_nobpp")
    check_dense_forms(res)
    host = res.cpu()
    assert host.partner.device.type == "cpu" and host.partner.tolist() == res.partner.tolist()


def test_shape_input_fastest_with_reactivities():
    from squarna_amd import Fold
    path = os.path.join(DATA, "examples", "shape_input.fas")
    res = Fold(inputfile=path, configfile="fastest")
    _is_device(res)
    assert res.source == "device"
    tuples, refsc = _engine_tuples(_parse(path), conf("fastest")[1], keep=5)
    check_against_tuples(res, tuples, keep=5, ref_scores=refsc)
    check_against_golden(res, "shape_input_fastest")


@pytest.mark.parametrize("poollim", [1, 100])
def test_synthetic_set_across_the_kernel_boundaries(poollim):
    """16-1,200 nt with reactivities, restraints (pairs included), gaps, separators: both sides of the 256- and 1,024-nt
    kernel boundaries, width-1 pools (chained rounds) and pools of a hundred (device pools); every record against
    fold_records, a sample against the oracle."""
    from oracle import sqrn_oracle as O
    from squarna_amd import Fold
    names, psets = conf("fastest")
    raw = _chain_records(34, 7117, 16, 1200) + _chain_records(6, 7118, 1030, 1200) + _chain_records(8, 7119, 240, 270)
    lens = [len(s) for s, _, _ in raw]
    assert min(lens) < 100 and any(256 < n <= 1024 for n in lens) and max(lens) > 1024
    assert any("-" in s for s, _, _ in raw) and any("&" in s for s, _, _ in raw) and any(x and "(" in x for _, _, x in raw)
    inputs = [(">r%d" % k, s, r, x, None) for k, (s, r, x) in enumerate(raw)]
    res = Fold(records=inputs, configfile="fastest", poollim=poollim, outplim=1000)
    _is_device(res)
    assert res.source == "device"
    tuples, _ = _engine_tuples(inputs, psets, poollim=poollim, keep=1000)
    check_against_tuples(res, tuples)
    assert any("[" in d for t in tuples for d, _, _ in t[1]), "no pseudoknotted structure in the set"
    assert max(len(t[1]) for t in tuples) > (1 if poollim > 1 else 0)
    sample = sorted(range(len(raw)), key=lambda k: lens[k])[:8:2] + [k for k in range(len(raw)) if 256 < lens[k] <= 420][:2]
    exp = {k: O.SQRNdbnseq(raw[k][0], raw[k][1], raw[k][2], None, psets, poollim=poollim, rankby=RANKBY_R) for k in sample}
    sub = Fold(records=[inputs[k] for k in sample], configfile="fastest", poollim=poollim, outplim=1000)
    check_against_tuples(sub, [exp[k] for k in sample])
    check_dense_forms(sub)


@pytest.mark.parametrize("opts,engine_opts", [(dict(rankby="dr"), dict(rankbydiff=True)), (dict(conslim=3), dict(conslim=3)),
                                              (dict(hardrest=True), dict(hardrest=True))])
def test_options_of_the_host_tail_give_the_same_content(opts, engine_opts):
    """rankbydiff, a consensus of several structures and forced restraint pairs keep the host tail: the tables are then
    converted from the packed records -- source "host", the content fold_records'."""
    from squarna_amd import Fold
    names, psets = conf("nobpp")
    raw = _chain_records(60, 911, 20, 200)
    assert any(x and "(" in x for _, _, x in raw)
    inputs = [(">r%d" % k, s, r, x, None) for k, (s, r, x) in enumerate(raw)]
    res = Fold(records=inputs, configfile="nobpp", **opts)
    _is_device(res)
    assert res.source == "host"
    tuples, _ = _engine_tuples(inputs, psets, keep=5, **engine_opts)
    check_against_tuples(res, tuples, keep=5)


def test_several_batches_equal_one_call_on_the_device(monkeypatch):
    from squarna_amd import Fold, api
    path = os.path.join(DATA, "examples", "seq_input.fas")
    one = Fold(inputfile=path, configfile="nobpp").cpu()
    monkeypatch.setattr(api, "BATCH_RECORDS", 4)
    many = Fold(inputfile=path, configfile="nobpp")
    _is_device(many)
    assert many.source == "device"
    for key in ("lengths", "nstruct", "row_off", "cell_off", "partner", "pset_mask"):
        assert getattr(many, key).tolist() == getattr(one, key).tolist(), key
    assert many.scores.cpu().numpy().tobytes() == one.scores.numpy().tobytes()
    assert many.metrics.cpu().numpy().tobytes() == one.metrics.numpy().tobytes()
    check_against_golden(many, "seq_input_nobpp")


# ---- the C entry directly ------------------------------------------------------------------------------------------
def _pairs_call(b, rows_cap=None, cells_cap=None, sentinel=None):
    """sq_result_pairs_size + sq_result_pairs_dev on torch buffers: (status, rows, cells, dict of host arrays)."""
    import torch
    L = b.L
    rows, cells = C.c_int64(-1), C.c_int64(-1)
    rc = L.sq_result_pairs_size(b.h, C.byref(rows), C.byref(cells))
    if rc:
        return rc, None, None, None
    rows, cells = rows.value, cells.value
    dev = b.device
    fill = -7 if sentinel is None else sentinel
    t = dict(partner=torch.full((max(cells, 1),), fill, dtype=torch.int32, device=dev),
             scores=torch.full((max(rows, 1), 3), float(fill), dtype=torch.float64, device=dev),
             pset_mask=torch.full((max(rows, 1),), fill, dtype=torch.int64, device=dev),
             metrics=torch.full((b.nseq, 16), float(fill), dtype=torch.float64, device=dev),
             row_off=torch.full((b.nseq + 1,), fill, dtype=torch.int64, device=dev),
             cell_off=torch.full((b.nseq + 1,), fill, dtype=torch.int64, device=dev))
    torch.cuda.synchronize(dev)
    rc = L.sq_result_pairs_dev(b.h, t["partner"].data_ptr(), cells if cells_cap is None else cells_cap, t["scores"].data_ptr(),
                               t["pset_mask"].data_ptr(), rows if rows_cap is None else rows_cap, t["metrics"].data_ptr(),
                               t["row_off"].data_ptr(), t["cell_off"].data_ptr(), C.c_void_p(b.stream.cuda_stream))
    torch.cuda.synchronize(dev)
    host = {k: v.cpu().numpy() for k, v in t.items()}
    host["partner"], host["scores"], host["pset_mask"] = host["partner"][:cells], host["scores"][:rows], host["pset_mask"][:rows]
    return rc, rows, cells, host


def _same_tables(got, b):
    """The entry's tables against the batch's packed records, converted on the host (results.packed_pair_tables)."""
    from squarna_amd.results import packed_pair_tables
    exp, nstruct, lengths = packed_pair_tables(*b.pack_all(copy=True))
    for key in ("row_off", "cell_off", "partner", "pset_mask"):
        assert got[key].tolist() == exp[key].tolist(), key
    assert got["scores"].tobytes() == exp["scores"].tobytes() and got["metrics"].tobytes() == exp["metrics"].tobytes()
    assert nstruct.tolist() == [int(b.L.sq_result_nstruct(b.h, k)) for k in range(b.nseq)]
    return nstruct


def test_c_entry_capacities_limit_and_second_fold():
    from squarna_amd import _lib
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf("nobpp")
    raw = _chain_records(48, 515, 14, 330)
    dbns = [None] * len(raw)
    prepared = [Prepared(s, r, x, d) for (s, r, x), d in zip(raw, dbns)]
    n = len(prepared)
    with Batch(prepared, [psets] * n, fp32=False) as b:
        b.fold(poollim=100, rankby=RANKBY_R)
        assert b.fold_paths & 1
        rc, rows, cells, got = _pairs_call(b)
        assert rc == 0 and rows > n and cells > 0
        first = _same_tables(got, b)
        assert first.max() > 2
        # capacities one short: an error, the message names the sizes, nothing is written
        for kw in (dict(rows_cap=rows - 1), dict(cells_cap=cells - 1), dict(rows_cap=0, cells_cap=0)):
            rc, _, _, buf = _pairs_call(b, sentinel=-7, **kw)
            assert rc < 0 and rc != -3, rc
            assert str(rows) in _lib.load().sq_last_error().decode() and str(cells) in _lib.load().sq_last_error().decode()
            assert all((v == -7).all() for v in buf.values())
        # a lower limit after the fold: the records no longer show what the tail left -- the caller reads the packed ones
        b.limit_results(1)
        assert _pairs_call(b)[0] == 1
        b.limit_results(0)
        assert _pairs_call(b)[0] == 0
        # a limit set before the fold is the fold's
        b.limit_results(2)
        b.fold(poollim=100, rankby=RANKBY_R)
        rc, rows2, cells2, got = _pairs_call(b)
        assert rc == 0 and rows2 < rows
        limited = _same_tables(got, b)
        assert limited.tolist() == np.minimum(first, 2).tolist()
        b.limit_results(0)
        # the same batch folded again under other options: the second call gives the second fold's results
        b.fold(poollim=1, conslim=0, rankby=(1, 2, 0))
        rc, rows3, cells3, got3 = _pairs_call(b)
        assert rc == 0
        third = _same_tables(got3, b)
        assert third.tolist() != first.tolist()
        off = got3["cell_off"]
        lens = np.diff(b.seq_off)
        for k in range(n):                                               # conslim == 0: an empty consensus row
            assert (got3["partner"][off[k]:off[k] + lens[k]] == -1).all()
        # the host tail's fold: not the device tail's form
        b.fold(poollim=1, rankbydiff=True)
        assert not (b.fold_paths & 1)
        assert _pairs_call(b)[0] == 1
        assert b.result_tensors() is None


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_sub_batches_of_fold_tensors_equal_one_batch(lanes, monkeypatch):
    """Fewer pool slots than the records' pools want: fold_tensors goes through the planner's sub-batches like fold_records
    (one after the other also under SQ_ENGINE_SUBLANES=2: the tables of a lane's stream are not cut), their tables
    concatenated with the offsets rebased -- the tables of ONE batch."""
    from squarna_amd import engine as E
    names, psets = conf("nobpp")
    raw = _chain_records(90, 6464, 60, 330)
    recs = [(s, r, x, None, psets, None) for s, r, x in raw]
    want = E.HipEngine().fold_tensors(recs, poollim=50, keep=20)
    assert want["source"] == "device"
    real_cap = E.pool_slot_cap
    monkeypatch.setattr(E, "pool_slot_cap", lambda maxn, want=None: min(real_cap(maxn), 9000))
    monkeypatch.setenv("SQ_ENGINE_SUBLANES", lanes)
    eng = E.HipEngine()
    made = []
    real_make = eng._make_batch
    monkeypatch.setattr(eng, "_make_batch", lambda *a, **k: made.append(len(a[0])) or real_make(*a, **k))
    got = eng.fold_tensors(recs, poollim=50, keep=20)
    assert len(made) > 1 and sum(made) == len(recs), made
    assert got["source"] == "device"
    for key in ("partner", "pset_mask", "row_off", "cell_off", "nstruct", "lengths"):
        assert got[key].tolist() == want[key].tolist(), key
    for key in ("scores", "metrics"):
        assert got[key].cpu().numpy().tobytes() == want[key].cpu().numpy().tobytes(), key


def test_a_row_beyond_64_kb_of_lds():
    """A 17,000-nt record: its row of partners (68 KB) takes the kernel's opt-in dynamic LDS; the helix that closes the
    whole sequence puts partners at both ends of the row.  Beside a short record, against fold_records."""
    from squarna_amd import Fold
    names, psets = conf("fastest")
    n = 17000
    long_seq = "GGGGGGCC" + "A" * (n - 16) + "GGCCCCCC"
    inputs = [(">long", long_seq, None, None, None), (">short", "GGGGAAAACCCC", None, None, None)]
    res = Fold(records=inputs, configfile="fastest", poollim=1)
    _is_device(res)
    assert res.source == "device" and res.lengths.tolist() == [n, 12]
    tuples, _ = _engine_tuples(inputs, psets, poollim=1, keep=5)
    check_against_tuples(res, tuples, keep=5)
    row = res.partner[int(res.cell_off[0]) + n:int(res.cell_off[0]) + 2 * n].tolist()      # the top structure
    assert row[0] == n - 1 and row[n - 1] == 0 and row[n // 2] == -1
