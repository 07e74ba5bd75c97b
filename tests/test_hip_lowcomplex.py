"""GPU parity on low-complexity RNA: repeats, G/C blocks, two- and three-letter alphabets and a stem-free sequence
(tests/golden/lowcomplex.json, the reference's own folds).  Such inputs give thousands of runs per structure and mass ties in
finalscore -- what the kernels' fixed LDS queues, staging areas and capacity estimates were not tuned on.

The expected values come from the fixture, so these tests start no oracle processes.  Every forced-path fold asserts its
driver and path bits: a fold the host loop repeated (driver 3: a queue or a capacity overflowed) fails where the launched
kernels it is compared with stayed on the device, and so does one that took another route than the one it was meant to
check.
"""
import hashlib
import io
import os

import pytest

from tests.lowcomplex import GOLDEN, check, load
from tests.test_hip_parity import conf
from tests.test_hip_parity4 import _packed

pytestmark = pytest.mark.gpu

FIX = load()
CASES = FIX["cases"]
LIST_FORM = 8 | 64 | 128          # sq_fold_paths: round kernel, root lists, kept lists


def _case_id(c):
    return "%s-%s" % (c["tag"], c["config"])


def _prepared(cases):
    from squarna_amd.engine import Prepared
    return [Prepared(c["seq"], c["reacts"], c["restraints"]) for c in cases]


def _by_config(cases):
    out = {}
    for c in cases:
        out.setdefault(c["config"], []).append(c)
    return sorted(out.items())


@pytest.mark.parametrize("config", sorted({c["config"] for c in CASES}))
def test_default_paths_equal_the_reference(config):
    """Every fixture case through HipEngine.fold_records at its configuration's pool limit (the engine picks the route by
    itself): consensus, every dbn, the number of structures, the first scores and paramsets, the digest of the whole list."""
    from squarna_amd.engine import HipEngine
    names, psets = conf(config)
    cases = [c for c in CASES if c["config"] == config]
    kw = cases[0]["kw"]
    assert all(c["kw"] == kw for c in cases)
    got = HipEngine().fold_records([(c["seq"], c["reacts"], c["restraints"], None, psets, None) for c in cases], **kw)
    for c, g in zip(cases, got):
        check(g, c, _case_id(c))


@pytest.mark.parametrize("tag", sorted(FIX["texts"]))
def test_predict_text_on_repeats_matches_reference(tag):
    """Predict(c=500nobpp) on repeat records -- E, H and N on stem graphs full of equal-weight edges, the tie path of the
    step-exact blossom -- byte for byte the reference's text."""
    from squarna_amd import Predict
    dig = FIX["texts"][tag]
    buf = io.StringIO()
    Predict(inputfile=os.path.join(GOLDEN, "text", dig["inputfile"]), configfile=dig["configfile"], write_to=buf)
    txt = buf.getvalue()
    with open(os.path.join(GOLDEN, "text", tag + ".txt")) as f:
        exp = f.read()
    if txt != exp:
        tl, el = txt.split("\n"), exp.split("\n")
        bad = [(k, a, b) for k, (a, b) in enumerate(zip(tl, el)) if a != b][:3]
        raise AssertionError("text differs (%d vs %d lines): %r" % (len(tl), len(el), bad))
    assert hashlib.sha256(txt.encode()).hexdigest() == dig["sha256"]


# ---- forced paths, packed records byte for byte ----
# Batches get room for every child of a full pool (64 per structure) and generous candidate records: what is left of
# driver 3 is the overflow the launched kernels have by design too (more ties within range than ChooseStems holds), and
# such a case is compared on the host loop's terms only by test_default_paths_equal_the_reference.
CAND_PER_NT = 256


def _slots(cases, psets, copies=1):
    from squarna_amd.engine import pool_slot_cap
    ng = sum(1 for ps in psets if "G" in ps["algorithms"])
    want = sum(64 * min(c["kw"]["poollim"], 1024) * ng + 4096 for c in cases) * copies
    return int(min(want, pool_slot_cap(max(len(c["seq"]) for c in cases), want=want)))


def _fold_one(case, psets, env, monkeypatch, **kw):
    """(driver, paths, packed record, evaluations, result) of one case folded alone under `env`."""
    from squarna_amd.engine import Batch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        with Batch(_prepared([case]), [psets], max_structs=_slots([case], psets), cand_per_nt=CAND_PER_NT, fp32=False,
                   **kw) as b:
            b.fold(poollim=case["kw"]["poollim"])
            return b.fold_driver, b.fold_paths, _packed(b, 1)[0], b.evals(0), b.results_all()[0][0]
    finally:
        for k in env:
            monkeypatch.delenv(k)


LONG = [c for c in CASES if 256 < len(c["seq"]) <= 1024 and c["kw"]["poollim"] > 1]


def test_list_form_equals_the_other_pool_routes(monkeypatch):
    """Pools wider than one on 257-1,024 nt run the list form of the round kernel by default (sq_fold_paths bit 7).  Against
    the launched round kernels (SQ_NO_POOL_KEPT), the root lists alone (+ SQ_POOL_ROOT: bit 6), a page pool that runs dry at
    once (SQ_KEPT_GB: children start from the root list with no finalscore inherited -- the walks' queue fills fastest) and
    rounds cut into launches of 300 structures (SQ_POOL_CHUNK): the same packed records and evaluation counts, and the
    reference's fold.  Every case whose launched kernels stay on the device must stay there on every other route."""
    compared = []
    for case in LONG:
        cid = _case_id(case)
        names, psets = conf(case["config"])
        d0, p0, want, evals, res = _fold_one(case, psets, dict(SQ_NO_POOL_KEPT="1"), monkeypatch, pool_lists=True)
        assert d0 in (2, 3) and not (p0 & LIST_FORM), (cid, "launched", d0, p0)
        if d0 == 3:
            continue
        check(res, case, cid)
        for paths, env in ((LIST_FORM, {}), (8 | 64, dict(SQ_NO_POOL_KEPT="1", SQ_POOL_ROOT="1")),
                           (LIST_FORM, dict(SQ_KEPT_GB="0.02")), (LIST_FORM, dict(SQ_POOL_CHUNK="300"))):
            d, p, got, ev, _ = _fold_one(case, psets, env, monkeypatch, pool_lists=True)
            assert d == 2, (cid, env, "driver", d)
            assert p & LIST_FORM == paths, (cid, env, "paths", p)
            assert got == want, (cid, env)
            assert ev == evals, (cid, env)
        compared.append(case)
    assert len(compared) >= len(LONG) // 2, [_case_id(c) for c in compared]
    assert any(300 <= len(c["seq"]) <= 620 for c in compared), [_case_id(c) for c in compared]


SHORT = [c for c in CASES if len(c["seq"]) <= 256 and c["kw"]["poollim"] > 1]


@pytest.mark.parametrize("config,cases", _by_config(SHORT), ids=[k for k, _ in _by_config(SHORT)])
def test_scan_form_round_kernel_equals_the_launched_round(config, cases, monkeypatch):
    """Up to 256 nt a pool round is the scan form of the round kernel (sq_fold_paths bit 3), picked by itself with batches in
    flight: three batches of every record twice, folded at once, against each record alone on the launched state / scan /
    score / choose kernels (SQ_NO_POOL_ROUND) -- and those against the reference."""
    import torch
    from squarna_amd.engine import Batch, fold_concurrently
    names, psets = conf(config)
    poollim = cases[0]["kw"]["poollim"]
    want, evals, kept = [], [], []
    for c in cases:
        d, p, got, ev, res = _fold_one(c, psets, dict(SQ_NO_POOL_ROUND="1"), monkeypatch)
        assert d in (2, 3) and not (p & 8), (_case_id(c), d, p)
        if d == 2:
            check(res, c, _case_id(c))
            want.append(got), evals.append(ev), kept.append(c)
    assert len(kept) >= len(cases) // 2, [_case_id(c) for c in kept]
    n = len(kept)
    prepared = _prepared(kept)
    batches = []
    for _ in range(3):
        with torch.cuda.stream(torch.cuda.Stream()):
            batches.append(Batch(prepared * 2, [psets] * (2 * n), fp32=False, max_structs=_slots(kept, psets, 2),
                                 cand_per_nt=CAND_PER_NT))
    torch.cuda.synchronize()
    try:
        fold_concurrently(batches, poollim=poollim)
        for b in batches:
            assert b.fold_driver == 2 and (b.fold_paths & 8), (config, b.fold_driver, b.fold_paths)
            got = _packed(b, 2 * n)
            for k in range(2 * n):
                assert got[k] == want[k % n], (config, _case_id(kept[k % n]))
                assert b.evals(k) == evals[k % n], (config, _case_id(kept[k % n]))
    finally:
        for b in batches:
            b.close()


@pytest.mark.parametrize("config,cases", [(k, sorted(v, key=lambda c: len(c["seq"]))[:2]) for k, v in _by_config(SHORT)],
                         ids=[k for k, _ in _by_config(SHORT)])
def test_host_loop_equals_the_launched_round(config, cases, monkeypatch):
    """The host-driven loop (SQ_NO_POOL: driver 0) sorts and filters a round's records on the CPU, in sq_choose.h's order and
    with its conflict test: on the two shortest records of a configuration, the packed record and the evaluation count of the
    launched state / scan / score / choose kernels (SQ_NO_POOL_ROUND)."""
    names, psets = conf(config)
    for c in cases:
        d, p, want, evals, _ = _fold_one(c, psets, dict(SQ_NO_POOL_ROUND="1"), monkeypatch)
        assert d in (2, 3) and not (p & 8), (_case_id(c), d, p)
        d, p, got, ev, res = _fold_one(c, psets, dict(SQ_NO_POOL="1"), monkeypatch)
        assert d == 0, (_case_id(c), "driver", d, p)
        check(res, c, _case_id(c))
        assert got == want, _case_id(c)
        assert ev == evals, _case_id(c)


ONE = [c for c in CASES if c["kw"]["poollim"] == 1]


def test_persistent_rounds_equal_the_launched_rounds():
    """poollim = 1: one launch of the persistent round kernel (sq_fold_paths bit 2) against the launched rounds
    (SQ_NO_ROUNDS), up to the 1,000-nt repeats -- packed records byte for byte, evaluation counts, the reference's folds."""
    from squarna_amd.engine import Batch
    assert "SQ_NO_ROUNDS" not in os.environ and ONE
    names, psets = conf("fastest")
    prepared = _prepared(ONE)
    n = len(prepared)
    out = []
    for launched in (False, True):
        if launched:
            os.environ["SQ_NO_ROUNDS"] = "1"
        try:
            with Batch(prepared, [psets] * n, max_structs=64 * n, fp32=False) as b:
                b.fold(poollim=1)
                assert b.fold_driver == 1, (launched, b.fold_driver)
                assert bool(b.fold_paths & 4) == (not launched), (launched, b.fold_paths)
                out.append((_packed(b, n), [b.evals(k) for k in range(n)], b.results_all()))
        finally:
            os.environ.pop("SQ_NO_ROUNDS", None)
    (pa, ea, ra), (pb, eb, rb) = out
    for k, c in enumerate(ONE):
        assert pa[k] == pb[k], _case_id(c)
        assert ea[k] == eb[k], _case_id(c)
        check(ra[k][0], c, _case_id(c))
