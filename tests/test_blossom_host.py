"""The product's blossom restatement (squarna_amd/csrc/sq_blossom.h), compiled for the host, against
networkx.max_weight_matching on random graphs with many ties (the reference's a-9 dependency)."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "blossom_host.cpp")
EXE = os.path.join(HERE, "native", "_build", "blossom_host")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EXE, SRC])
    return EXE


def _graphs(seed, count, nmax=22, mmax=60):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.randint(2, nmax)
        m = rng.randint(1, min(mmax, n * (n - 1) // 2))
        pairs = set()
        while len(pairs) < m:
            a, b = rng.sample(range(n), 2)
            pairs.add((min(a, b), max(a, b)))
        pairs = list(pairs)
        rng.shuffle(pairs)
        small = rng.random() < 0.6                        # few distinct weights -> non-unique optima
        edges = [(a, b, float(rng.randint(1, 4)) if small else round(rng.uniform(1, 30), 3) ** 1.7) for a, b in pairs]
        out.append(edges)
    return out


@pytest.mark.parametrize("seed,count,nmax,mmax", [(7, 400, 22, 60), (11, 60, 120, 700)])
def test_blossom_matches_networkx(exe, seed, count, nmax, mmax):
    """(the second set: graphs of the size of SRtest150's -- nested blossoms, expansions, lists scanned in chunks)"""
    nx = pytest.importorskip("networkx")
    graphs = _graphs(seed, count, nmax, mmax)
    lines, idmaps = [str(len(graphs))], []
    for edges in graphs:
        ids = {}
        for a, b, _ in edges:                              # vertex ids in first-appearance order == nx node order
            ids.setdefault(a, len(ids))
            ids.setdefault(b, len(ids))
        idmaps.append(ids)
        lines.append("%d %d" % (len(ids), len(edges)))
        lines += ["%d %d %r" % (ids[a], ids[b], w) for a, b, w in edges]
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip().split("\n")
    assert len(rows) == len(graphs)
    for edges, ids, row in zip(graphs, idmaps, rows):
        G = nx.Graph()
        for a, b, w in edges:
            G.add_edge(a, b, weight=w)
        exp = nx.max_weight_matching(G)
        nums = list(map(int, row.split()))
        n = len(nums) // 2
        mate, mord = nums[:n], nums[n:]
        inv = {v: k for k, v in ids.items()}
        # networkx returns each pair as (u, v) with u the endpoint that entered its `mate` dict first
        # (matching_dict_to_set); Edmonds() sorts those tuples (SQRNalgos.py:109), so the orientation is observable
        got = {(inv[v], inv[mate[v]]) for v in range(n) if mate[v] >= 0 and mord[v] < mord[mate[v]]}
        assert got == exp, (edges, got, exp)


def _run(exe, graphs, tight):
    """blossom_host on edge lists whose vertex ids are already in graph order: one output row per graph."""
    lines = [str(len(graphs))]
    for n, edges in graphs:
        lines.append("%d %d" % (n, len(edges)))
        lines += ["%d %d %r" % e for e in edges]
    res = subprocess.run([exe, str(tight)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    rows = res.stdout.strip().split("\n")
    assert len(rows) == len(graphs)
    return rows


def test_the_graphs_of_the_storage_form_tests_stay_inside_the_tight_capacities(exe):
    """The blossom kernel reruns a graph in global memory when a run with the tight capacities (all state in LDS: tight = 1; the
    hot part alone, with the short queue: tight = 2) overflows one of them -- queue, pool, frames.  A GPU test of such a form
    on a graph that overflows would pass on the rerun.  So every graph that tests/test_hip_matching_forms.py sends to the GPU
    runs here under the three capacities: no error, mates and first-assignment ranks of the tight runs equal to the generous
    one's, and its pairs those of networkx.max_weight_matching with their (u, v) orientation."""
    pytest.importorskip("networkx")
    from tests import matching_checks as M
    graphs, labels, exp = [], [], []
    for name in ("crowd", "three", "single", "few", "bins", "mixed"):
        for edges in M.forms_set(name):
            if not edges:
                continue
            ids, uniq = {}, {}
            for u, v, x in edges:                              # as sq_graph.hip builds the job: vertices in first-appearance
                a, b = ids.setdefault(u, len(ids)), ids.setdefault(v, len(ids))    # order, a repeated edge keeps its first
                key = (min(a, b), max(a, b))                   # position and takes the last weight
                uniq[key] = (uniq[key][0] if key in uniq else (a, b), x)
            graphs.append((len(ids), [(a, b, x) for (a, b), x in uniq.values()]))
            assert (len(ids), len(uniq)) == M.mwm_dims(edges)
            labels.append({k: u for u, k in ids.items()})
            exp.append(M.networkx_pairs(edges))
    assert len(graphs) >= 2200
    rows = [_run(exe, graphs, tight) for tight in (0, 1, 2)]
    for tight in (0, 1, 2):
        assert not [k for k, row in enumerate(rows[tight]) if "ERROR" in row], tight
        assert rows[tight] == rows[0], (tight, [k for k in range(len(graphs)) if rows[tight][k] != rows[0][k]][:5])
    for (n, _), lab, row, e in zip(graphs, labels, rows[0], exp):
        nums = list(map(int, row.split()))
        mate, mord = nums[:n], nums[n:]
        assert len(nums) == 2 * n
        assert sorted((lab[v], lab[mate[v]]) for v in range(n) if mate[v] >= 0 and mord[v] < mord[mate[v]]) == e, (n, e[:4])
