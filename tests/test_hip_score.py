"""GPU tests of Score() / HipEngine.score_tensors / sq_score_structs_dev: the scoring of given structures on the device,
against the values the reference returned (tests/golden/score.json), the CPU path of Score on the same rows, and the ranking
tail's own metrics of a fold.  All comparisons are exact: integers, and doubles bit for bit."""
import os

import numpy as np
import pytest

from tests import score_checks as SC
from tests.fold_checks import DATA

pytestmark = pytest.mark.gpu


def _cpu_score(**kw):
    from squarna_amd import Score
    from squarna_amd import engine as E
    from tests.oracle_engine import OracleEngine
    with E.use_engine(OracleEngine()):
        return Score(**kw)


def _is_device(res):
    import torch
    assert res.source == "device"
    for key in ("scores", "metrics", "status", "nstems", "npairs", "stems", "stem_off", "ref_scores", "row_off"):
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.is_cuda, key
    assert res.scores.dtype == torch.float64 and res.metrics.dtype == torch.float64 and res.ref_scores.dtype == torch.float64
    assert res.status.dtype == torch.int32 and res.stems.dtype == torch.int32 and res.stem_off.dtype == torch.int64


@pytest.fixture
def kernel_calls(monkeypatch):
    """Every HipEngine.score_tensors call of the test: (the partner tensor's address, whether it is on the GPU, the
    kernels' own status and ref_status as they left the device -- BEFORE Score hands status-2 rows to the host)."""
    from squarna_amd.engine import HipEngine
    seen, inner = [], HipEngine.score_tensors

    def spy(self, records, partner, row_start, row_rec):
        out = inner(self, records, partner, row_start, row_rec)
        seen.append((partner.data_ptr(), partner.is_cuda, out["status"].cpu().tolist(), out["ref_status"].cpu().tolist()))
        return out
    monkeypatch.setattr(HipEngine, "score_tensors", spy)
    return seen


def _none_handed_back(calls, results=()):
    """No row and no known structure left the kernels with status 2: the device scored them, not the host behind it."""
    assert calls
    for _, _, status, ref_status in calls:
        assert 2 not in status and 2 not in ref_status
    assert all(res.recomputed == 0 for res in results)


def test_golden_cases_on_the_device(kernel_calls):
    """Every golden case in the three forms; the padded form is a CUDA tensor, which the kernels read where it is."""
    import torch
    from squarna_amd import Score
    cs = SC.cases()
    recs = SC.records_of(cs)
    seen = kernel_calls
    a = Score(records=recs, structures=SC.strings_form(cs))
    padded, nstruct = SC.padded_form(cs, extra=5)
    dev = torch.from_numpy(padded).cuda()
    before = dev.clone()
    b = Score(records=recs, structures=dev, nstruct=nstruct)
    assert seen[-1][:2] == (dev.data_ptr(), True) and torch.equal(dev, before)
    fr = SC.fold_result_form(cs, device="cuda")
    c = Score(records=recs, structures=fr)
    assert seen[-1][:2] == (fr.partner.data_ptr(), True)
    assert len(seen) == 3
    _none_handed_back(seen, (a, b, c))                               # no row with status 2, as the kernels wrote it
    for res in (a, b, c):
        _is_device(res)
        SC.check_golden(res, cs)


def test_mixed_records_in_one_call(kernel_calls):
    """Lengths 1 to 263, 0 to 6 rows, with and without reactivities, gaps and known structures in ONE call: equal to one call
    per record and to the CPU path."""
    from squarna_amd import Score
    cs = SC.cases()
    structures = SC.strings_form(cs)
    for r in range(2, len(cs), 7):
        structures[r] = []                                           # K = 0
    recs = SC.records_of(cs)
    assert {len(c["seq"]) for c in cs} >= {1, 263} and {len(s) for s in structures} >= {0, 1, 6}
    res = Score(records=recs, structures=structures)
    _is_device(res)
    SC.equal_results(res, _cpu_score(records=recs, structures=structures))
    host = res.cpu()
    for r, rec in enumerate(recs):
        one = Score(records=[rec], structures=[structures[r]]).cpu()
        a, b = int(host.row_off[r]), int(host.row_off[r + 1])
        assert SC.same(one.scores.numpy(), host.scores[a:b].numpy()) and SC.same(one.metrics.numpy(), host.metrics[a:b].numpy()), rec[0]
        assert SC.same(one.ref_scores.numpy(), host.ref_scores[r:r + 1].numpy()), rec[0]
        assert one.stems.tolist() == host.stems[int(host.stem_off[a]):int(host.stem_off[b])].tolist(), rec[0]
    _none_handed_back(kernel_calls, (res,))


def test_invalid_rows_on_the_device():
    from squarna_amd import Score
    for name, seq, row in SC.INVALID:
        good = np.full(len(seq), -1, np.int32)
        padded = np.stack([good, np.asarray(row, np.int32)])[None]
        rec = [(">r", seq, None, None, "." * len(seq))]
        with pytest.raises(ValueError, match=r"record 0 \(>r\), row %d" % (0 if name == "nothing_to_score" else 1)):
            Score(records=rec, structures=padded)
        res = Score(records=rec, structures=padded, strict=False)
        SC.equal_results(res, _cpu_score(records=rec, structures=padded, strict=False))
        assert res.status.tolist()[1] == 1 and bool(np.isnan(res.scores[1].cpu().numpy()).all()), name


def test_agrees_with_the_ranking_tail_of_a_fold():
    """The fold's device tail computes the same metrics from its own stem log: the consensus row, the known structure's
    scores and the best of the top five structures must come out of Score(fold result) bit for bit.  (Fold's scores are NOT
    compared: the fold scores its stem sets as they were assembled, abutting stems unmerged.)"""
    import contextlib
    import io
    from squarna_amd import Fold, Score
    from squarna_amd.inputs import ParseInput
    path = os.path.join(DATA, "datasets", "SRtest150.fas")
    fold = Fold(inputfile=path, inputformat="qf", configfile="nobpp")
    with contextlib.redirect_stdout(io.StringIO()):
        recs = list(ParseInput(None, path, "qf")[0])
    assert all(rec[4] for rec in recs)
    res = Score(records=recs, structures=fold)
    _is_device(res)
    host, fm = res.cpu(), fold.metrics.cpu().numpy()
    ro = host.row_off.numpy()
    assert (np.diff(ro) == 1 + fold.nstruct.cpu().numpy()).all()
    assert SC.same(host.metrics.numpy()[ro[:-1]], fm[:, :6])
    assert SC.same(host.ref_scores.numpy(), fm[:, 13:16])
    checked = 0
    for r in range(len(recs)):
        top = host.metrics.numpy()[ro[r] + 1:ro[r] + 1 + min(int(ro[r + 1] - ro[r]) - 1, 5)]
        if not len(top):
            continue
        best = int(np.argmax(top[:, 3]))                             # (the first row with the highest FS, :1277)
        assert SC.same(np.append(top[best], best + 1), fm[r, 6:13]), recs[r][0]
        checked += 1
    assert checked > 200


def test_ten_thousand_rows_of_one_record(kernel_calls):
    """One 60-nt record with 10,000 candidate structures as a CUDA tensor: a grid of rows, equal to the CPU path on a sample."""
    import torch
    from squarna_amd import Score
    rng = np.random.default_rng(60)
    n, K = 60, 10000
    seq = ''.join(rng.choice(list("ACGU"), n))
    rows = np.full((1, K, n), -1, np.int32)
    for k in range(K):
        for _ in range(int(rng.integers(0, 5))):
            a, b, ln = int(rng.integers(0, n - 1)), int(rng.integers(1, n)), int(rng.integers(1, 6))
            for q in range(ln):
                v, w = a + q, b - q
                if v < w and rows[0, k, v] < 0 and rows[0, k, w] < 0:
                    rows[0, k, v], rows[0, k, w] = w, v
    known = "((((((....((((....))))...))))))".ljust(n, ".")
    rec = [(">one", seq, [float(x) for x in rng.random(n).round(3)], None, known)]
    res = Score(records=rec, structures=torch.from_numpy(rows).cuda())
    _is_device(res)
    assert tuple(res.scores.shape) == (K, 3) and res.status.count_nonzero().item() == 0
    _none_handed_back(kernel_calls, (res,))
    pick = np.sort(rng.choice(K, 200, replace=False))
    want = _cpu_score(records=rec, structures=rows[:, pick])
    host = res.cpu()
    assert SC.same(host.scores.numpy()[pick], want.scores.numpy()) and SC.same(host.metrics.numpy()[pick], want.metrics.numpy())
    assert host.nstems.numpy()[pick].tolist() == want.nstems.tolist()
    assert [host.stems_of(int(q)) for q in pick] == [want.stems_of(q) for q in range(200)]
    assert SC.same(host.ref_scores.numpy(), want.ref_scores.numpy())
