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


def test_the_full_sweep_of_the_metric_ratios(kernel_calls):
    """6,422 rows of six 200-nt records as one padded CUDA tensor: TP = 0 .. K known pairs and FP = 0 .. 96 others for known
    structures of 0, 1, 3, 16, 48 and 80 pairs.  TP FP FN FS PR RC equal plain Python's round(x, 3) of the ratios, bit for
    bit -- ties such as 9/16 and the near ties over 80 and 160 among them (tests/test_score_api.py counts those)."""
    import torch
    from squarna_amd import Score
    recs, rows, nstruct, want = SC.sweep()
    dev = torch.from_numpy(rows).cuda()
    res = Score(records=recs, structures=dev, nstruct=nstruct)
    _is_device(res)
    assert kernel_calls[-1][:2] == (dev.data_ptr(), True) and len(kernel_calls) == 1
    _none_handed_back(kernel_calls, (res,))
    host = res.cpu()
    assert host.row_off.tolist() == np.concatenate([[0], np.cumsum(nstruct)]).tolist()
    assert host.status.tolist() == [0] * len(want) and kernel_calls[-1][2] == [0] * len(want)
    assert host.npairs.tolist() == (want[:, 0] + want[:, 1]).tolist()
    got, counts = host.metrics.numpy(), SC.sweep_counts()
    wrong = [(counts[q], got[q].tolist(), want[q].tolist()) for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not wrong, (len(wrong), wrong[:5])


def _hands_back(c, stems):
    """A structure of case c with these golden stems (gap-free coordinates) holds a stem whose pair values sum above 4.0."""
    value = {"GC": 4.0, "CG": 4.0, "AU": 1.5, "UA": 1.5, "GU": -0.5, "UG": -0.5}
    short = ''.join(ch for ch in c["seq"].upper().replace("T", "U") if ch not in "-.~")
    return any(sum(value.get(short[i + t] + short[j - t], 0.0) for t in range(ln)) > 4.0 for i, j, ln in stems)


@pytest.mark.parametrize("form", ["strings", "padded"])
def test_rows_the_kernel_hands_back_are_scored_by_the_host(kernel_calls, monkeypatch, form):
    """With a power table of 9 entries (a single GC pair is its last) the kernel leaves every row and known structure that
    holds a stem summing above 4.0 with status 2, and Score() recomputes their scores and metrics on the host and writes
    them into the device tensors: the result still equals the reference's everywhere."""
    import torch
    from squarna_amd import Score
    from squarna_amd.dbn import DBNToPairs, PairsToStems, UnAlign
    from squarna_amd.engine import HipEngine
    full = HipEngine._pow17_table
    monkeypatch.setattr(HipEngine, "_pow17_table", lambda self, nmax: full(self, nmax)[:9])
    cs = SC.cases()
    recs = SC.records_of(cs)
    if form == "strings":
        res = Score(records=recs, structures=SC.strings_form(cs))
    else:
        padded, nstruct = SC.padded_form(cs, extra=5)
        res = Score(records=recs, structures=torch.from_numpy(padded).cuda(), nstruct=nstruct)
    _is_device(res)
    back = [int(_hands_back(c, row["stems"])) for c in cs for row in c["rows"]]
    ref_back = []                                                    # (the golden holds no stems of the known structures)
    for c in cs:
        known = PairsToStems(sorted(DBNToPairs(UnAlign(c["seq"], c["known"])[1]))) if c["known"] else []
        ref_back.append(int(_hands_back(c, [(st[0][0][0], st[0][0][1], st[1]) for st in known])))
    assert 40 < sum(back) < len(back) - 40 and 5 < sum(ref_back) < len(cs) - 5
    assert len(kernel_calls) == 1
    assert kernel_calls[0][2] == [2 * b for b in back] and kernel_calls[0][3] == [2 * b for b in ref_back]
    assert res.recomputed == sum(back) + sum(ref_back)
    assert res.status.tolist() == [0] * len(back)
    SC.check_golden(res, cs)                                         # (stems, nstems and npairs of every row are the device's)


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
    # Score and the tail share sq_scoring.h, so neither vouches for the other: the counts from the fold's own partner rows
    # and each record's known pairs with numpy, the ratios with Python's round, the known structure's scores from the host
    from squarna_amd.score import ScoreRecord
    partner, cell = fold.partner.cpu().numpy(), fold.cell_off.cpu().numpy()
    assert not any(ch in "-.~" for rec in recs for ch in rec[1])     # (columns are positions: no pair is dropped)
    mine = []
    for r, rec in enumerate(recs):
        n = len(rec[1])
        rows, known = partner[cell[r]:cell[r + 1]].reshape(-1, n), SC.partner_row(rec[4])
        opener = rows > np.arange(n)
        tp, npairs, nknown = (opener & (rows == known)).sum(1), opener.sum(1), int((known > np.arange(n)).sum())
        mine.extend(SC.sweep_metrics(nknown, int(t), int(p - t)) for t, p in zip(tp, npairs))
        own = ScoreRecord(rec[0], rec[1], rec[2], rec[4])
        assert SC.same(own.score(own.known), fm[r, 13:16]), rec[0]
    mine = np.array(mine, np.float64)
    assert mine.shape == host.metrics.shape and mine.tobytes() == host.metrics.numpy().tobytes()
    assert mine[ro[:-1]].tobytes() == fm[:, :6].tobytes()
    for r in range(len(recs)):
        top = mine[ro[r] + 1:ro[r] + 1 + min(int(ro[r + 1] - ro[r]) - 1, 5)]
        if len(top):
            best = int(np.argmax(top[:, 3]))
            assert np.append(top[best], best + 1).tobytes() == fm[r, 6:13].tobytes(), recs[r][0]


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
