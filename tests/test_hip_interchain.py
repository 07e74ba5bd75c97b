"""GPU: folds of multi-chain records on every route of the greedy pool loop, with interchainonly on and off
(tests/interchain_checks.py: two and three chains, three planted 12-nt reverse complements between chains).

With interchainonly the bit words come from sq_bits_direct_kernel and the persistent round kernel must not form words of its
own; until now no such fold was longer than 111 nt.  Every case is compared with the oracle's SQRNdbnseq(...,
interchainonly=...), four of them with the reference's own fold (tests/golden/interchain.json), and its default route --
asserted by driver and path bits, as in test_hip_lowcomplex.py -- byte for byte (packed record, evaluation count) with the
route it replaces.  No case may leave the device: driver 3 (a capacity overflowed and the host loop repeated the fold) fails."""
import os

import pytest

from tests import interchain_checks as I
from tests.bits_checks import load_golden
from tests.lowcomplex import check
from tests.test_hip_lowcomplex import CAND_PER_NT, LIST_FORM, _fold_one, _prepared, _slots
from tests.test_hip_parity import _same_fold, conf
from tests.test_hip_parity4 import _packed

pytestmark = pytest.mark.gpu

GOLDEN = {(c["tag"], c["config"]): c for c in load_golden()["folds"]}
ICO = pytest.mark.parametrize("interchainonly", [True, False], ids=["interchainonly", "all_pairs"])


def _cases(cases):
    return pytest.mark.parametrize("case", cases, ids=[I.case_id(c) for c in cases])


def _against_the_oracle(res, case, interchainonly, psets):
    """The fold against the oracle's (and the reference's, where the fixture has the case); under the chain test no pair of
    the consensus or of any structure joins two positions of one chain, and the fold is not the one without the switch (the
    library's own: the oracle's is what the all_pairs case of the same record is compared with)."""
    from oracle import sqrn_oracle as O
    cid = I.case_id(case)
    _same_fold(res, I.oracle_fold(cid, interchainonly), (cid, interchainonly))
    if interchainonly:
        chain = I.chain_of(case["seq"])
        rows = [res[0]] + [s[0] for s in res[1]]
        pairs = [bp for row in rows for bp in O.DBNToPairs(row)]
        assert len(O.DBNToPairs(res[0])) >= 12 and all(chain[v] != chain[w] for v, w in pairs), cid
        assert res[0] != _fold_one(case, psets, {}, None)[4][0], cid
        if (case["tag"], case["config"]) in GOLDEN:
            check(res, GOLDEN[(case["tag"], case["config"])], cid)


@ICO
@_cases(I.SCAN)
def test_scan_form_of_the_round_kernel(case, interchainonly, monkeypatch):
    """Up to 256 nt: three batches of the record twice, folded at once, take the scan form of the round kernel (sq_fold_paths
    bit 3); the record alone on the launched state / scan / score / choose kernels (SQ_NO_POOL_ROUND) gives the same bytes."""
    import torch
    from squarna_amd.engine import Batch, fold_concurrently
    names, psets = conf(case["config"])
    d, p, want, evals, res = _fold_one(case, psets, dict(SQ_NO_POOL_ROUND="1"), monkeypatch, interchainonly=interchainonly)
    assert d == 2 and not (p & 8), (I.case_id(case), "launched", d, p)
    _against_the_oracle(res, case, interchainonly, psets)
    prepared = _prepared([case])
    batches = []
    for _ in range(3):
        with torch.cuda.stream(torch.cuda.Stream()):
            batches.append(Batch(prepared * 2, [psets] * 2, fp32=False, max_structs=_slots([case], psets, 2), cand_per_nt=CAND_PER_NT,
                                 interchainonly=interchainonly))
    torch.cuda.synchronize()
    try:
        fold_concurrently(batches, poollim=case["kw"]["poollim"])
        for b in batches:
            assert b.fold_driver == 2 and (b.fold_paths & 8), (I.case_id(case), b.fold_driver, b.fold_paths)
            assert _packed(b, 2) == [want, want], I.case_id(case)
            assert [b.evals(0), b.evals(1)] == [evals, evals], I.case_id(case)
    finally:
        for b in batches:
            b.close()


@ICO
@_cases(I.LIST)
def test_list_form_of_the_round_kernel(case, interchainonly, monkeypatch):
    """257-1,024 nt with a pool: the list form (bits 3, 6, 7) against the launched round kernels (SQ_NO_POOL_KEPT) and the
    root lists alone (+ SQ_POOL_ROOT: bits 3, 6)."""
    names, psets = conf(case["config"])
    cid = I.case_id(case)
    kw = dict(pool_lists=True, interchainonly=interchainonly)
    d, p, want, evals, res = _fold_one(case, psets, dict(SQ_NO_POOL_KEPT="1"), monkeypatch, **kw)
    assert d == 2 and not (p & LIST_FORM), (cid, "launched", d, p)
    _against_the_oracle(res, case, interchainonly, psets)
    for paths, env in ((LIST_FORM, {}), (8 | 64, dict(SQ_NO_POOL_KEPT="1", SQ_POOL_ROOT="1"))):
        d, p, got, ev, _ = _fold_one(case, psets, env, monkeypatch, **kw)
        assert d == 2, (cid, env, "driver", d)
        assert p & LIST_FORM == paths, (cid, env, "paths", p)
        assert got == want, (cid, env)
        assert ev == evals, (cid, env)


@ICO
@_cases(I.ONE)
def test_persistent_round_kernel(case, interchainonly):
    """poollim = 1: one launch of the persistent round kernel (bit 2, driver 1) -- under the chain test on the words of
    sq_bits_direct_kernel, never its own -- against the launched rounds (SQ_NO_ROUNDS)."""
    from squarna_amd.engine import Batch
    assert "SQ_NO_ROUNDS" not in os.environ
    names, psets = conf(case["config"])
    out = []
    for launched in (False, True):
        if launched:
            os.environ["SQ_NO_ROUNDS"] = "1"
        try:
            with Batch(_prepared([case]), [psets], max_structs=64, fp32=False, interchainonly=interchainonly) as b:
                b.fold(poollim=1)
                assert b.fold_driver == 1, (launched, b.fold_driver)
                assert bool(b.fold_paths & 4) == (not launched), (launched, b.fold_paths)
                out.append((_packed(b, 1), b.evals(0), b.results_all()[0][0]))
        finally:
            os.environ.pop("SQ_NO_ROUNDS", None)
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1], I.case_id(case)
    _against_the_oracle(out[0][2], case, interchainonly, psets)


@ICO
@_cases(I.LAUNCHED)
def test_launched_forms_beyond_1024(case, interchainonly, monkeypatch):
    """1,025 nt with a pool of 5: the device pools on the launched kernels (no bit of the round kernel), against the oracle."""
    names, psets = conf(case["config"])
    d, p, _, _, res = _fold_one(case, psets, {}, monkeypatch, interchainonly=interchainonly)
    assert d == 2 and not (p & LIST_FORM), (I.case_id(case), d, p)
    _against_the_oracle(res, case, interchainonly, psets)
