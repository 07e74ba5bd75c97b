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
