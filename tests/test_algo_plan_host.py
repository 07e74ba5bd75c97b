"""The plan of a matching chunk (squarna_amd/csrc/sq_algo_plan.h), compiled for the host with a plain C++ compiler.

tests/golden/algo_plan.json.gz holds what the driver computed BEFORE the plan became a unit of its own: every chunk and every
blossom launch of SRtest150 under nobpp folded alone and as three batches in flight, and of the low-complexity 500nobpp records,
each on the device-side and on the host-driven RunAlgo (SQ_NO_DEVICE_ALGOS).  The header must give every recorded value -- the
cut, the totals, both layouts, the LDS needs, the launch order, the classes, the blossom bins -- exactly.  The same program
checks the layouts' and the orders' properties on synthetic job lists."""
import gzip
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "algo_plan_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "algo_plan_host")
CHUNK_KEYS = ("k1", "bytes", "scratch", "outints", "nedges", "vids", "carve", "stage", "need", "sorted_pos", "classes")
MWM_KEYS = ("nbins", "waves", "lds", "all_in_lds", "slices", "bin_head")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(os.path.join(HERE, "golden", "algo_plan.json.gz"), "rt") as f:
        return json.load(f)


def _line(r):
    flat = " ".join("%d %d" % (n, m) for n, m in r["jobs"])
    if r["kind"] == "chunk":
        return "C %d %d %d %d %d %d %d %s" % (r["algo"], r["inflight"], r["region_bytes"], r["dev"], r["lsap_classes"], r["mwm_classes"],
                                              len(r["jobs"]), flat)
    return "M %d %d %d %d %d %d %s" % (r["inflight"], r["bin_waves"], r["bin_bytes"], r["all_cap"], r["nolds"], len(r["jobs"]), flat)


def test_the_header_gives_the_recorded_plans(exe, recorded):
    rows = recorded["records"]
    res = subprocess.run([exe], input="\n".join(_line(r) for r in rows) + "\n", capture_output=True, text=True, check=True)
    got = [json.loads(x) for x in res.stdout.strip().split("\n")]
    assert len(got) == len(rows)
    for k, (r, g) in enumerate(zip(rows, got)):
        for key in (CHUNK_KEYS if r["kind"] == "chunk" else MWM_KEYS):
            assert g[key] == r[key], (k, r["scenario"], r["kind"], r.get("algo"), key)
    # what the recording covers: both forms, alone and crowded, all three algorithms, one- and multi-wave blossom launches
    chunks = [r for r in rows if r["kind"] == "chunk"]
    mwm = [r for r in rows if r["kind"] == "mwm"]
    assert {(r["algo"], r["dev"], r["inflight"] > 1) for r in chunks} >= {(a, d, c) for a in (2, 4, 8) for d in (0, 1) for c in (False, True)}
    assert any(len(r["classes"]) > 1 for r in chunks) and any(r["waves"] == 1 for r in mwm) and any(r["waves"] > 1 for r in mwm)
    assert {r["scenario"] for r in rows} == set(recorded["scenarios"]) and len(recorded["scenarios"]) == 12


def test_layout_and_order_properties_on_synthetic_job_lists(exe):
    res = subprocess.run([exe, "props"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    assert res.stdout.strip().endswith("plans checked, 0 failures") and int(res.stdout.split()[0]) >= 2000, res.stdout


def _mwm_line(dims, inflight=1, bin_waves=0, bin_bytes=0, all_cap=0, nolds=False):
    return "M %d %d %d %d %d %d %s" % (inflight, bin_waves, bin_bytes, all_cap, int(nolds), len(dims), " ".join("%d %d" % d for d in dims))


def test_the_python_mirror_of_the_blossom_launch_equals_the_header(exe, recorded):
    """tests/matching_checks.mwm_launch -- by which the GPU tests of tests/test_hip_matching_forms.py assert the storage form,
    the waves and the bins of every call -- against sq_mwm_plan and the kernel's two tests computed from SqBlossom's own
    functions: on every graph set of that module under every switch setting it is sent with, and on the recorded launches."""
    from tests import matching_checks as M
    (sizes,) = [json.loads(x) for x in subprocess.run([exe], input="S 193 437\n", capture_output=True, text=True, check=True).stdout.split("\n") if x]
    assert sizes["hdr"] == M.MWM_HDR and sizes["edge"] == M.mwm_edge_bytes(437)
    for t in (0, 1, 2):
        assert sizes["t%d" % t] == [M.mwm_hot_bytes(193, 437, t), M.mwm_cold_bytes(193, 437, t), M.mwm_scratch_bytes(193, 437, t),
                                    M.mwm_queue_cap(193, 437, t), M.mwm_pool_capacity(193, 437, t), M.mwm_frame_ints(193, t)], t
    # (the two sizes the module's docstrings quote)
    assert M.mwm_hot_bytes(600, 600, 2) + 16 + M.MWM_HDR == 41294
    assert (M.mwm_scratch_bytes(300, 1800, 1) + 1800 * 16 + 16, M.mwm_hot_bytes(300, 1800, 2) + 16) == (187694, 21782)
    cases = [(M.forms_set(s), {}) for s in ("crowd", "three", "single")]
    cases += [(M.forms_set(s), kw) for _, sets, kw in M.FORMS_SCENARIOS.values() for s in sets]
    cases += [([g], {}) for g in M.forms_set("few")[:8]]                   # one graph per call, as core.Edmonds sends it
    cases = [([M.mwm_dims(g) for g in graphs], kw) for graphs, kw in cases]
    rows = [r for r in recorded["records"] if r["kind"] == "mwm"]
    cases += [([tuple(j) for j in r["jobs"]], dict(inflight=r["inflight"], bin_waves=r["bin_waves"], bin_bytes=r["bin_bytes"],
                                                   all_cap=r["all_cap"], nolds=bool(r["nolds"]))) for r in rows]
    res = subprocess.run([exe], input="\n".join(_mwm_line(d, **kw) for d, kw in cases) + "\n", capture_output=True, text=True, check=True)
    got = [json.loads(x) for x in res.stdout.strip().split("\n")]
    assert len(got) == len(cases) and len(rows) >= 10
    seen = set()
    for k, ((dims, kw), g) in enumerate(zip(cases, got)):
        mine = M.mwm_launch(dims, **kw)
        assert g["hdr"] == M.MWM_HDR
        for key in MWM_KEYS:
            assert (int(mine[key]) if key == "all_in_lds" else mine[key]) == g[key], (k, kw, key)
        assert [-1 if f is None else f for f in mine["forms"]] == g["forms"], (k, kw)
        assert mine["lds_bytes"] == [s[1] for s in g["slices"]] and sorted(q for b in mine["bins"] for q in b) == list(range(len(dims)))
        seen |= {(mine["waves"] == 1, f) for f in mine["forms"]}
    assert seen >= {(single, f) for single in (False, True) for f in (0, 1, 2, None)}
    # the recorded rows themselves: the mirror gives what the driver computed before the plan was a unit
    for r in rows:
        mine = M.mwm_launch([tuple(j) for j in r["jobs"]], r["inflight"], r["bin_waves"], r["bin_bytes"], r["all_cap"], bool(r["nolds"]))
        assert all((int(mine[key]) if key == "all_in_lds" else mine[key]) == r[key] for key in MWM_KEYS), r["scenario"]


def test_the_python_mirror_of_the_nussinov_block_size(exe):
    from tests import matching_checks as M
    crowd = [(len(s), len(c)) for s, c in M.nussinov_crowd_set()]
    few = [(len(s), len(c)) for s, c in M.nussinov_problem_set()]
    cases = [(crowd, 1, 0), (few, 1, 0), (few, 2, 0), (few, 1, 64), (few, 1, 128), (crowd[:1023], 1, 0), ([(65, 3)], 1, 0), ([(300, 3)], 1, 0)]
    text = "".join("N %d %d %d %s\n" % (inflight, thr, len(d), " ".join("%d %d" % x for x in d)) for d, inflight, thr in cases)
    got = [json.loads(x)["threads"] for x in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    assert got == [M.nussinov_threads(d, inflight, thr) for d, inflight, thr in cases] == [64, 256, 256, 64, 128, 256, 128, 256]
