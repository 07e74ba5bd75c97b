"""GPU parity, round 4: the persistent round kernel of width-1 pools (sq_rounds.hip: one launch per fold, a block per
structure that loops over its own rounds and keeps its list of runs between them) against the launched rounds
(sq_chain.hip, SQ_NO_ROUNDS) and against the oracle.

Every check goes through the C ABI (libsquarna_hip.so); the oracle (oracle/) is the checker.
"""
import os

import numpy as np
import pytest

from tests.test_hip_parity import GOLDEN, TOL, conf, load, mk_pset, prep, _same_fold, _synthetic  # noqa: F401
from tests.test_hip_parity2 import _chain_records

pytestmark = pytest.mark.gpu


def _packed_both_ways(prepared, psets, kernel_runs=True, **kw):
    """The packed records of one batch folded by the persistent round kernel and by the launched rounds."""
    from squarna_amd.engine import Batch
    out = []
    assert "SQ_NO_ROUNDS" not in os.environ
    for launched in (False, True):
        if launched:
            os.environ["SQ_NO_ROUNDS"] = "1"
        try:
            with Batch(prepared, psets, max_structs=max(len(prepared) * max(len(p) for p in psets), 1), fp32=False) as b:
                b.fold(**kw)
                assert b.fold_driver == 1, b.fold_driver
                assert bool(b.fold_paths & 4) == (kernel_runs and not launched), b.fold_paths
                buf, off = b.pack_all()
                out.append(([buf[off[k]:off[k + 1]].tobytes() for k in range(len(prepared))], [r[0] for r in b.results_all()],
                            [b.evals(k) for k in range(len(prepared))]))
        finally:
            os.environ.pop("SQ_NO_ROUNDS", None)
    return out


@pytest.mark.parametrize("config,count,nmin,nmax,sample", [("fastest", 400, 5, 420, 40), ("nobpp", 160, 12, 260, 20),
                                                           ("greedynobpp", 120, 12, 200, 16), ("alt", 120, 5, 300, 16)])
def test_persistent_rounds_equal_launched_rounds_and_oracle(config, count, nmin, nmax, sample):
    """poollim = 1 over random records with reactivities, restraints (incl. restraint pairs) and separators: the runs
    kept between rounds and cut against the chosen stem are AnnotateStems' output of every round -- packed records byte
    for byte those of the launched rounds, the same evaluation counts, and the oracle's structures and scores."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Prepared
    names, psets = conf(config)
    raw = _chain_records(count, 4343, nmin, nmax)
    prepared = [Prepared(s, r, x) for s, r, x in raw]
    (pa, ra, ea), (pb, rb, eb) = _packed_both_ways(prepared, [psets] * count, poollim=1)
    assert ea == eb
    for k in range(count):
        assert pa[k] == pb[k], (config, k, raw[k][0], ra[k][:2], rb[k][:2])
    for k in range(sample):
        s, r, x = raw[k]
        exp = O.SQRNdbnseq(s, r, x, None, psets, poollim=1)
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(ra[k], exp, (config, "persistent", k))


def test_persistent_rounds_maxstemnum_negative_weights_and_pseudoknots():
    """Retirement by stem count, paramsets whose pieces can outscore their run (negative GU weight with a low
    threshold), float reactivities outside the level table, and long GC-rich sequences with deep level stacks."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Prepared
    names, psets = conf("fastest")
    rng = np.random.default_rng(78)
    seqs = ["".join(rng.choice(list("ACGU"), int(n))) for n in rng.integers(60, 400, 40)]
    prepared = [Prepared(s) for s in seqs]
    for msn in (0, 1, 3):
        ps = [dict(psets[0], maxstemnum=msn)]
        (pa, ra, ea), (pb, rb, eb) = _packed_both_ways(prepared, [ps] * len(seqs), kernel_runs=msn > 0, poollim=1)
        assert pa == pb and ea == eb, msn
    # pieces that outscore their run: GU = -3, threshold low
    ps = [dict(psets[0], bpweights={"GC": 3.0, "AU": 2.0, "GU": -3.0}, minlen=2, minbpscore=4, minfinscorefactor=0.5)]
    (pa, ra, ea), (pb, rb, eb) = _packed_both_ways(prepared, [ps] * len(seqs), poollim=1)
    assert pa == pb and ea == eb
    for k in range(8):
        exp = O.SQRNdbnseq(seqs[k], None, None, None, ps, poollim=1)
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(ra[k], exp, ("negative", k))
    # float reactivities (more than 16 distinct values: factors per cell)
    reacts = [list(rng.random(len(s))) for s in seqs[:16]]
    prepared_r = [Prepared(s, r) for s, r in zip(seqs[:16], reacts)]
    (pa, ra, ea), (pb, rb, eb) = _packed_both_ways(prepared_r, [psets] * 16, poollim=1)
    assert pa == pb and ea == eb
    # long, GC-rich, pseudoknots free of charge
    longs = ["".join(rng.choice(list("ACGU"), int(n), p=[0.15, 0.35, 0.35, 0.15])) for n in (900, 1300, 1700)]
    ps = [dict(psets[0], orderpenalty=0.0, minlen=3, minbpscore=6)]
    (pa, ra, ea), (pb, rb, eb) = _packed_both_ways([Prepared(s) for s in longs], [ps] * 3, poollim=1)
    assert pa == pb and ea == eb
    deep = max(sum(ch in r[1][0][0] for ch in "[{<A") for r in ra)
    assert deep >= 3


@pytest.mark.parametrize("n,count,seed,reacts", [(1000, 96, 1001, False), (2000, 24, 2001, True), (300, 1500, 301, False)])
def test_persistent_rounds_on_the_baseline_shapes(n, count, seed, reacts):
    """S300 / S1000 / S2000 (+ SHAPE) shaped batches: byte-identical to the launched rounds."""
    from squarna_amd.engine import Prepared
    names, psets = conf("fastest")
    data = _synthetic(n, count, seed, reacts)
    (pa, ra, ea), (pb, rb, eb) = _packed_both_ways([Prepared(s, rc) for s, rc in data], [psets] * count, poollim=1)
    assert ea == eb
    assert pa == pb


# ---- device pools: a round of short structures as ONE kernel (sq_pool_round.hip) ---------------------------------------
def _pools_both_ways(prepared, psets, env=None, **kw):
    """Packed records of one batch folded with sq_pool_round_kernel (the default) and with the launched state / scan / score /
    choose kernels (SQ_NO_POOL_ROUND)."""
    from squarna_amd.engine import Batch, pool_slot_cap, pool_slots_wanted_many
    out = []
    lengths = [len(p.shortseq) for p in prepared]
    slots = int(min(pool_slots_wanted_many(lengths, psets, kw.get("poollim", 1000)).sum(), pool_slot_cap(max(lengths))))
    for launched in (False, True):
        extra = dict(env or {}) if not launched else {"SQ_NO_POOL_ROUND": "1"}
        assert not any(k in os.environ for k in extra)
        os.environ.update(extra)
        try:
            with Batch(prepared, psets, max_structs=max(slots, 4096), fp32=False) as b:
                b.fold(**kw)
                assert b.fold_driver == 2, b.fold_driver
                assert bool(b.fold_paths & 8) == (not launched), b.fold_paths
                buf, off = b.pack_all()
                out.append(([buf[off[k]:off[k + 1]].tobytes() for k in range(len(prepared))], [r[0] for r in b.results_all()],
                            [b.evals(k) for k in range(len(prepared))]))
        finally:
            for k in extra:
                os.environ.pop(k, None)
    return out


@pytest.mark.parametrize("config,count,nmin,nmax,poollim,sample,env", [
    ("nobpp", 200, 12, 220, 1000, 24, None), ("greedynobpp", 200, 12, 250, 3, 24, None), ("alt", 150, 5, 200, 1000, 16, None),
    ("greedynobpp", 100, 30, 250, 40, 12, {"SQ_POOL_ROUND_NSURV": "64"}), ("fastest", 150, 5, 250, 7, 16, None)])
def test_pool_round_kernel_equals_launched_round_and_oracle(config, count, nmin, nmax, poollim, sample, env):
    """Pools of any width over random records with reactivities, restraints and separators: the one-wave round kernel
    gives the packed records of the launched kernels byte for byte (also when its survivors spill out of LDS), the same
    evaluation counts, and the oracle's structures and scores."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Prepared
    names, psets = conf(config)
    raw = _chain_records(count, 900 + poollim, nmin, nmax)
    prepared = [Prepared(s, r, x) for s, r, x in raw]
    (pa, ra, ea), (pb, rb, eb) = _pools_both_ways(prepared, [psets] * count, env=env, poollim=poollim)
    assert ea == eb
    for k in range(count):
        assert pa[k] == pb[k], (config, poollim, k, raw[k][0], ra[k][:2], rb[k][:2])
    for k in range(sample):
        s, r, x = raw[k]
        exp = O.SQRNdbnseq(s, r, x, None, psets, poollim=poollim)
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(ra[k], exp, (config, "pool round", poollim, k))


def test_pool_round_kernel_on_srtest150_sets_in_flight():
    """The headline shape: several batches of SRtest150 copies in flight (the crowded mode picks the round kernel by itself)
    give the records of one batch folded alone with the launched kernels."""
    import torch
    from squarna_amd.engine import Batch, Prepared, fold_concurrently
    from squarna_amd.inputs import ParseDefaultInput
    names, psets = conf("nobpp")
    recs = list(ParseDefaultInput(os.path.join(os.path.dirname(os.path.dirname(__file__)), "squarna_amd", "data", "datasets", "SRtest150.fas"), "qf"))
    prepared = [Prepared(r[1], r[2], r[3], r[4]) for r in recs]
    os.environ["SQ_NO_POOL_ROUND"] = "1"
    try:
        with Batch(prepared, [psets] * len(prepared), fp32=False, max_structs=4096) as b:
            b.fold(poollim=1000)
            buf, off = b.pack_all()
            ref = [buf[off[k]:off[k + 1]].tobytes() for k in range(len(prepared))]
    finally:
        del os.environ["SQ_NO_POOL_ROUND"]
    batches = []
    for _ in range(3):
        with torch.cuda.stream(torch.cuda.Stream()):
            batches.append(Batch(prepared * 2, [psets] * (2 * len(prepared)), fp32=False, max_structs=8192))
    torch.cuda.synchronize()
    try:
        fold_concurrently(batches, poollim=1000)
        for b in batches:
            buf, off = b.pack_all()
            for k in range(2 * len(prepared)):
                assert buf[off[k]:off[k + 1]].tobytes() == ref[k % len(prepared)], k
    finally:
        for b in batches:
            b.close()


def test_log_of_final_structures_overflow_is_reported():
    """The device log of final structures with too little room for the stems: the fold must say so (no entry of the log may
    stay unwritten and be ranked as if it were a structure)."""
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf("nobpp")
    rng = np.random.default_rng(31)
    # (plain records: RunAlgo's filters run on the device and append their stemsets to the log themselves)
    prepared = [Prepared("".join(rng.choice(list("ACGU"), int(n)))) for n in rng.integers(60, 200, 40)]
    assert "SQ_FIN_STEM_CAP" not in os.environ
    os.environ["SQ_FIN_STEM_CAP"] = "64"
    try:
        with Batch(prepared, [psets] * len(prepared), max_structs=4096, fp32=False) as b:
            with pytest.raises(Exception) as ei:
                b.fold(poollim=1)
            assert "log of final structures" in str(ei.value) or "capacity" in str(ei.value), str(ei.value)
    finally:
        del os.environ["SQ_FIN_STEM_CAP"]
    with Batch(prepared, [psets] * len(prepared), max_structs=4096, fp32=False) as b:     # the same batch with room: fine
        b.fold(poollim=1)
        assert b.fold_paths & 1


def test_shape_records_run_the_device_runalgo_and_equal_the_oracle():
    """SRtest150 with encoded reactivity lines ("_+#") and records with float reactivities under nobpp (E, H, N and two
    greedy paramsets), mixed with plain records: every job's RunAlgo stays on the device (sq_fold_paths bit 1; stemscore **
    1.7 of the jobs with reactivity factors comes from the host's libm in bulk), packed records equal the host-driven form
    byte for byte and the oracle's structures and scores."""
    from oracle import sqrn_oracle as O
    from squarna_amd.dbn import ProcessReacts, ReactDict
    from squarna_amd.engine import Batch, Prepared
    from squarna_amd.inputs import ParseDefaultInput
    names, psets = conf("nobpp")
    rng = np.random.default_rng(150)
    recs = list(ParseDefaultInput(os.path.join(os.path.dirname(os.path.dirname(__file__)), "squarna_amd", "data", "datasets", "SRtest150.fas"), "qf"))
    data = []
    for k, r in enumerate(recs[:150]):
        seq = r[1]
        if k % 5 == 4:
            data.append((seq, None))                                              # plain records in between
        elif k % 5 == 3:
            data.append((seq, [float(x) for x in rng.random(len(seq))]))          # float reactivities
        else:
            line = rng.choice(list("_+#"), len(seq), p=[0.5, 0.3, 0.2])
            data.append((seq, ProcessReacts([ReactDict[c] for c in line], M=1.8, B=-0.6)))
    prepared = [Prepared(s, rc) for s, rc in data]
    with Batch(prepared, [psets] * len(prepared), fp32=False, max_structs=8192) as b:
        b.fold(poollim=1000)
        assert b.fold_paths & 2, b.fold_paths
        buf, off = b.pack_all()
        dev = [buf[off[k]:off[k + 1]].tobytes() for k in range(len(prepared))]
        got = [r[0] for r in b.results_all()]
        assert "SQ_NO_DEVICE_ALGOS" not in os.environ
        os.environ["SQ_NO_DEVICE_ALGOS"] = "1"
        try:
            b.fold(poollim=1000)
            assert not (b.fold_paths & 2)
            buf, off = b.pack_all()
            host = [buf[off[k]:off[k + 1]].tobytes() for k in range(len(prepared))]
        finally:
            del os.environ["SQ_NO_DEVICE_ALGOS"]
    assert dev == host
    for k in range(0, len(data), 6):
        s, rc = data[k]
        exp = O.SQRNdbnseq(s, rc, None, None, psets, poollim=1000)
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(got[k], exp, ("shape", k))


def test_soak_slice_2000_random_records_under_nobpp():
    """A 2,000-record slice of the parity soak (tools/fuzz_parity.py: random sequences with reactivities, restraints,
    chains, gaps; all five algorithms; the CPU oracle in worker processes against the HIP engine).  At this size the
    batch runs the crowded forms: sq_pool_round_kernel, one wave per Nussinov job, the blossom kernel with several
    graphs per block and several queue vertices per scan pass -- whose resolution of two lists' claims to one vertex rests
    on LDS executing one wave's stores in program order: re-checked on every run of the GPU suite."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "2000", "nobpp", "401"],
                       cwd=root, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0 and "2000 records (config nobpp, poollim 1000), 0 mismatches" in r.stdout, tail


def test_pool_overflow_keeps_the_stemsets_of_the_device_runalgo():
    """Device pools that outgrow their slots hand the greedy part to the host loop; the E / H / N stemsets the device RunAlgo
    has logged by then must survive (round 3 emptied the whole log there): same records as a fold with room, and as the
    oracle."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf("nobpp")
    raw = _chain_records(90, 5150, 30, 170)
    prepared = [Prepared(s, r, x) for s, r, x in raw]
    with Batch(prepared, [psets] * len(prepared), max_structs=16384, fp32=False) as b:
        b.fold(poollim=1000)
        assert b.fold_driver == 2 and (b.fold_paths & 2)
        buf, off = b.pack_all()
        want = [buf[off[k]:off[k + 1]].tobytes() for k in range(len(prepared))]
        got0 = b.results_all()[0][0]
        assert "SQ_POOL_SLOTS" not in os.environ
        os.environ["SQ_POOL_SLOTS"] = str(2 * len(prepared) + 3)        # room for the first generation only
        try:
            for _ in range(3):
                b.fold(poollim=1000)
                assert b.fold_driver == 3 and (b.fold_paths & 2), (b.fold_driver, b.fold_paths)
                buf, off = b.pack_all()
                assert [buf[off[k]:off[k + 1]].tobytes() for k in range(len(prepared))] == want
        finally:
            del os.environ["SQ_POOL_SLOTS"]
    s, r, x = raw[0]
    exp = O.SQRNdbnseq(s, r, x, None, psets, poollim=1000)
    exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
    _same_fold(got0, exp, ("overflow", 0))


def test_shared_bit_matrices_equal_one_matrix_per_job():
    """Jobs of a sequence whose paramsets pair the same letters read ONE diagonal bit matrix (a-1 built once per record
    instead of once per paramset); a paramset with another letter set keeps its own.  Packed records byte for byte those
    of a batch created with SQ_NO_SHARED_BITS, with restraints, reactivities and separators in the records."""
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf("nobpp")
    odd = dict(psets[0], bpweights={"GC": 3.25, "AU": 1.25})           # no GU pairs: another boolean matrix
    mixed = list(psets) + [odd]
    raw = _chain_records(90, 977, 8, 180)
    prepared = [Prepared(s, r, x) for s, r, x in raw]
    packs = []
    assert "SQ_NO_SHARED_BITS" not in os.environ
    for own in (False, True):
        if own:
            os.environ["SQ_NO_SHARED_BITS"] = "1"
        try:
            with Batch(prepared, [mixed] * len(prepared), max_structs=8192, fp32=False) as b:
                for pl in (1000, 1):
                    b.fold(poollim=pl)
                    buf, off = b.pack_all()
                    packs.append(bytes(buf[:off[-1]]))
        finally:
            os.environ.pop("SQ_NO_SHARED_BITS", None)
    assert packs[0] == packs[2] and packs[1] == packs[3]


def test_blossom_large_graphs_hubs_and_stars_match_networkx():
    """Round 4's blossom kernel against networkx.max_weight_matching itself where its new parts work hardest: graphs of
    200-600 vertices (more than the 192 entries the dual step keeps in registers: its chunked form; adjacency and state
    beyond one wave's reach), hubs with hundreds of neighbours (lists longer than the wave: a chunk per pass; edge chunks that
    name one vertex dozens of times: the adjacency's rank rounds), stars and double stars, few distinct weights (ties
    everywhere), edges shuffled.  Pairs and their (u, v) orientation (SQRNalgos.py:96-110)."""
    import random
    import networkx as nx
    import squarna_amd as S
    from tests.matching_checks import mwm_dims, mwm_launch
    rng = random.Random(20261004)
    cases, forms = [], []
    for trial in range(10):
        n = rng.randrange(200, 600)
        deg = rng.choice((2, 3, 5, 8))
        weights = rng.choice(((1.0,), (1.0, 2.0), (0.5, 1.5, 4.0, 4.5, 8.0), tuple(float(x) for x in range(1, 40))))
        pairs = set()
        hubs = rng.sample(range(n), rng.randrange(1, 4))
        for v in range(n):
            for _ in range(rng.randrange(1, deg + 1)):
                w = rng.choice(hubs) if rng.random() < 0.3 else rng.randrange(n)
                if rng.random() < 0.3:
                    w = (v + rng.choice((1, 2, 3))) % n
                if w != v:
                    pairs.add((min(v, w), max(v, w)))
        cases.append((n, [(a, b, rng.choice(weights)) for a, b in pairs]))
    # a star, a double star with a bridge, a hub in front of a long odd cycle
    cases.append((130, [(0, v, float(1 + v % 3)) for v in range(1, 130)]))
    cases.append((200, [(0, v, 2.0) for v in range(2, 100)] + [(1, v, 2.0) for v in range(100, 200)] + [(0, 1, 3.0)]))
    cases.append((151, [(v, v + 1, 1.0) for v in range(1, 150)] + [(150, 1, 1.0)] + [(0, v, 1.0) for v in range(1, 151, 2)]))
    for k, (n, edges) in enumerate(cases):
        rng.shuffle(edges)
        G = nx.Graph()
        G.add_weighted_edges_from(edges)
        exp = sorted(nx.max_weight_matching(G))
        got = S.Edmonds([[[(u, v)], 1, w] for u, v, w in edges], power=1.0)
        assert got == exp, (k, n, len(edges))
        forms += mwm_launch([mwm_dims(edges)])["forms"]
    # one graph per call, a block of 150 KB: the graphs of 465, 554, 435 and 585 vertices keep only the hot part of their state
    # in LDS, the others all of it (tests/test_hip_matching_forms.py has every form in both kernels)
    assert forms == [1, 1, 2, 1, 1, 2, 1, 1, 2, 2, 1, 1, 1]


def _packed(b, n):
    buf, off = b.pack_all()
    return [buf[off[k]:off[k + 1]].tobytes() for k in range(n)]


@pytest.mark.parametrize("host_tail", [False, True])
def test_optimistic_chains_ties_handoff_and_pool_overflow(host_tail, monkeypatch):
    """Pools that may branch but rarely do (range factor 1.0, poollim > 1: `fastest` at the default pool limit) run as chains
    on the persistent round kernel (sq_fold_paths bit 4 = 16); a structure that meets a run tied with the best finalscore AND
    sharing a base with it stops, and the device pools fold its job.  Against the pools alone (SQ_NO_OPT_CHAIN), against the
    oracle, with the device tail and the host tail, and with the pools overflowing into the host loop (SQ_POOL_SLOTS) after
    the chains have already finished part of the jobs."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf("fastest")
    rng = np.random.default_rng(777)
    raw = _chain_records(140, 9191, 20, 260)
    # sequences that tie: over two letters runs of equal finalscore that share a base with the best one are common (a third
    # of such records branch in the reference) -- the branch the chains must hand over
    for rep in range(48):
        raw.append(("".join(rng.choice(list("GC"), int(rng.integers(25, 90)))), None, None))
    prepared = [Prepared(s, r, x) for s, r, x in raw]
    n = len(prepared)
    if host_tail:
        monkeypatch.setenv("SQ_NO_DEVICE_TAIL", "1")
    with Batch(prepared, [psets] * n, max_structs=16384, fp32=False) as b:
        monkeypatch.setenv("SQ_NO_OPT_CHAIN", "1")
        b.fold(poollim=1000)
        assert b.fold_driver == 2 and not (b.fold_paths & 16), (b.fold_driver, b.fold_paths)
        want = _packed(b, n)
        res = b.results_all()
        monkeypatch.delenv("SQ_NO_OPT_CHAIN")
        for _ in range(2):
            b.fold(poollim=1000)
            assert b.fold_paths & 16, b.fold_paths
            assert bool(b.fold_paths & 1) == (not host_tail), b.fold_paths
            assert _packed(b, n) == want
        # the pools overflow after the chains have finished their share: the host loop repeats EVERY greedy job
        monkeypatch.setenv("SQ_POOL_SLOTS", "3")
        for _ in range(2):
            b.fold(poollim=1000)
            assert b.fold_paths & 16, b.fold_paths
            assert _packed(b, n) == want
        monkeypatch.delenv("SQ_POOL_SLOTS")
        handed = b.fold_driver
    assert handed in (2, 3)
    branched = 0
    for k in list(range(0, 140, 12)) + list(range(140, n, 2)):
        s, r, x = raw[k]
        exp = O.SQRNdbnseq(s, r, x, None, psets, poollim=1000)
        branched += len(exp[1]) > 1
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(res[k][0] if isinstance(res[k], tuple) else res[k], exp, ("optimistic chains", k))
    assert branched > 0, "no sampled record branched: the tie hand-off was not exercised"


@pytest.mark.parametrize("case", ["gc1500", "minlen1"])
def test_capacity_overflow_is_repeated_with_a_larger_batch_not_raised(case):
    """The reference builds Python lists and has no capacities (SQRNdbnseq.py:427-495).  Inputs with several times the runs of
    a random sequence -- GC-only, 1,500 nt; minlen = 1 on GC-rich sequences -- outgrow the candidate records a batch sizes for
    random sequences: the engine repeats the fold with a larger batch instead of raising, and the result is the oracle's."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import HipEngine
    rng = np.random.default_rng(31)
    if case == "gc1500":
        names, psets = conf("fastest")
        seqs = ["".join(rng.choice(list("GC"), 1500)), "".join(rng.choice(list("ACGU"), 300))]
        poollim = 1
    else:
        names, psets = conf("greedynobpp")
        psets = [dict(psets[0], minlen=1, minbpscore=0.0, bpweights={"GC": 3.25, "AU": 1.25, "GU": 1.0})]
        seqs = ["".join(rng.choice(list("GCGCGU"), n)) for n in (180, 240, 90)]
        poollim = 1
    eng = HipEngine(cand_per_nt=1)                                   # (the estimate for random sequences alone sizes the records)
    got = eng.fold_records([(s, None, None, None, psets, None) for s in seqs], poollim=poollim)
    if case == "gc1500":                                             # (minlen = 1: the estimate covers isolated cells by design)
        assert getattr(eng, "capacity_retries", 0) >= 1, "the case did not outgrow the first batch: it no longer tests the repeat"
    for s, g in zip(seqs, got):
        e = O.SQRNdbnseq(s, None, None, None, psets, poollim=poollim)
        e = [e[0], [[d, list(sc), list(p)] for d, sc, p in e[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(g, e, (case, len(s)))


def test_pools_long_sample_equals_the_oracle():
    """bench.py's pools_long workload -- random 500-nt sequences under 500nobpp (the reference's configuration from 500 nt on:
    two greedy paramsets whose pools branch, + E / H / N) at the default pool limit -- on a 16-record sample against the
    oracle (worker processes, started before that process touches the GPU: ~7 s of CPU per record), through the engine's
    sub-batching path."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "16", "500nobpp"], cwd=root,
                       env=dict(os.environ, FUZZ_SET="pools_long"), capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0 and "16 records (config 500nobpp, poollim 1000), 0 mismatches" in r.stdout, tail


@pytest.mark.gpu
@pytest.mark.parametrize("config,poollim", [("nobpp", 1000), ("greedynobpp", 5), ("alt", 1000)])
def test_pool_rounds_enqueued_ahead_equal_the_exact_grids(config, poollim, monkeypatch):
    """A batch alone enqueues the rounds of the device pools ahead of the host (sq_fold_paths bit 5 = 32: every launch covers
    all slots, blocks beyond the generation's size leave, the host follows the published headers): packed records, evaluation
    counts and the largest generation are those of the rounds launched one by one with exact grids (SQ_POOL_AHEAD=0), for
    depths 1, 3 and 6 -- also when a generation outgrows the slots and the host loop repeats the fold -- and the oracle's."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf(config)
    raw = _chain_records(64, 4242 + poollim, 10, 200)
    prepared = [Prepared(s, r, x) for s, r, x in raw]
    n = len(prepared)
    with Batch(prepared, [psets] * n, max_structs=8192, fp32=False) as b:
        monkeypatch.setenv("SQ_POOL_AHEAD", "0")
        b.fold(poollim=poollim)
        assert b.fold_driver == 2 and (b.fold_paths & 8) and not (b.fold_paths & 32), (b.fold_driver, b.fold_paths)
        want, evals, peak = _packed(b, n), [b.evals(k) for k in range(n)], b.fold_peak_structs
        res = b.results_all()
        for depth in ("1", "3", "6"):
            monkeypatch.setenv("SQ_POOL_AHEAD", depth)
            for _ in range(2):
                b.fold(poollim=poollim)
                assert b.fold_driver == 2 and (b.fold_paths & 32), (depth, b.fold_driver, b.fold_paths)
                assert _packed(b, n) == want, depth
                assert [b.evals(k) for k in range(n)] == evals
                assert b.fold_peak_structs == peak, (depth, b.fold_peak_structs, peak)
        monkeypatch.delenv("SQ_POOL_AHEAD")
        b.fold(poollim=poollim)                                  # the default depth
        assert (b.fold_paths & 32) and _packed(b, n) == want
        monkeypatch.setenv("SQ_POOL_CHUNK", "3000")              # a generation in three launches over the candidate arena
        b.fold(poollim=poollim)
        assert (b.fold_paths & 32) and _packed(b, n) == want
        monkeypatch.setenv("SQ_POOL_CHUNK", "1000")              # too many launches per round: the exact grids, chunked
        b.fold(poollim=poollim)
        assert not (b.fold_paths & 32) and _packed(b, n) == want
        monkeypatch.delenv("SQ_POOL_CHUNK")
        if peak > 2 * n + 8:                                     # the pools outgrow their slots mid-way: the host loop takes over
            monkeypatch.setenv("SQ_POOL_SLOTS", str(2 * n + 8))
            b.fold(poollim=poollim)
            assert b.fold_driver == 3, b.fold_driver
            assert _packed(b, n) == want
            monkeypatch.delenv("SQ_POOL_SLOTS")
    for k in range(0, n, 8):
        s, r, x = raw[k]
        exp = O.SQRNdbnseq(s, r, x, None, psets, poollim=poollim)
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(res[k][0], exp, (config, "ahead", poollim, k))


def test_pooled_score_kernel_block_sizes_agree(monkeypatch):
    """Generations of thousands of structures on sequences beyond 256 nt (the launched round kernels: state / scan / score /
    choose / extend) with 64, 128 and 512 threads per structure of the score kernel (SQ_SCORE_POOL_THREADS; default 128 from
    2,048 structures on): the same packed records, the largest generation beyond 2,048, and the oracle's structures."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf("nobpp")
    rng = np.random.default_rng(2048)
    seqs = ["".join(rng.choice(list("ACGU"), int(n))) for n in rng.integers(262, 300, 20)]
    prepared = [Prepared(s) for s in seqs]
    packs = {}
    with Batch(prepared, [psets] * len(prepared), max_structs=65536, fp32=False) as b:
        for thr in ("64", "128", "512"):
            monkeypatch.setenv("SQ_SCORE_POOL_THREADS", thr)
            b.fold(poollim=1000)
            assert b.fold_driver == 2 and not (b.fold_paths & 8), (b.fold_driver, b.fold_paths)
            assert b.fold_peak_structs >= 2048, b.fold_peak_structs
            packs[thr] = _packed(b, len(prepared))
        res = b.results_all()
    assert packs["64"] == packs["128"] == packs["512"]
    for k in (0, 7):
        exp = O.SQRNdbnseq(seqs[k], None, None, None, psets, poollim=1000)
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(res[k][0], exp, ("pooled score threads", k))


def test_pool_rounds_over_root_lists_equal_the_launched_kernels(monkeypatch):
    """SQ_POOL_ROOT=1 (opt-in): pools on sequences of 257-1,024 nt run the one-wave round kernel over per-job root lists -- the
    runs of the empty structure with their bpscores, checked against every structure's partner array (sq_fold_paths bit 6 = 64)
    -- instead of the launched state / scan / score / choose / extend kernels: the same packed records and evaluation counts,
    with reactivities, restraints (pairs included), separators, survivors beyond the LDS room and chunked generations; and the
    oracle's structures."""
    from oracle import sqrn_oracle as O
    from squarna_amd.engine import Batch, Prepared
    names, psets = conf("nobpp")
    raw = _chain_records(28, 6464, 257, 420)
    prepared = [Prepared(s, r, x) for s, r, x in raw]
    n = len(prepared)
    assert min(len(r[0]) for r in raw) > 256
    with Batch(prepared, [psets] * n, max_structs=65536, fp32=False) as b:
        b.fold(poollim=1000)
        assert b.fold_driver == 2 and not (b.fold_paths & 64), (b.fold_driver, b.fold_paths)
        want, evals = _packed(b, n), [b.evals(k) for k in range(n)]
        res = b.results_all()
        monkeypatch.setenv("SQ_POOL_ROOT", "1")
        for extra in ({}, {"SQ_POOL_ROUND_NSURV": "64"}, {"SQ_POOL_CHUNK": "700"}):
            for k, v in extra.items():
                monkeypatch.setenv(k, v)
            b.fold(poollim=1000)
            assert b.fold_driver == 2 and (b.fold_paths & 64), (extra, b.fold_driver, b.fold_paths)
            assert _packed(b, n) == want, extra
            assert [b.evals(k) for k in range(n)] == evals
            for k in extra:
                monkeypatch.delenv(k)
    for k in (0, 9, 17):
        s, r, x = raw[k]
        exp = O.SQRNdbnseq(s, r, x, None, psets, poollim=1000)
        exp = [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7]
        _same_fold(res[k][0], exp, ("root lists", k))
