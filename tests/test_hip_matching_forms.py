"""GPU: every storage form of the blossom kernel in both of its kernels, against networkx.max_weight_matching itself.

sq_mwm_one (csrc/sq_match.hip) runs a graph with all its state and the edge list in LDS (form 1), with the hot part alone there
(form 2: blossom structure and adjacency in the graph's global scratch, the short queue) or with everything in global memory
(form 0), by the LDS the launch gives it; sq_mwm_single_kernel runs one graph per block, sq_mwm_kernel up to eight, one per
wave, in bins chained through the job table.  Every array is addressed differently in each form.  Here each form is judged in
each kernel, the three forms in one launch of the bin kernel, bins of 3, 4 and 8 waves (tests/test_hip_matching_many.py has 2),
the crowd plan (4 waves, 40 KB bins, hot parts only: what every run with batches in flight uses), and the Nussinov kernel at one
wave per problem, whatever its length.

tests/matching_checks.mwm_launch mirrors the plan's and the kernel's decisions (pinned against the header on the CPU:
tests/test_algo_plan_host.py); before every call it is asserted that the call takes the forms, waves and bins the test is about.
A run that overflows a tight capacity of form 1 or 2 is rerun in form 0 and would pass on the rerun:
tests/test_blossom_host.py shows on the CPU that no graph sent from here does.  Every comparison is integer equality of
sorted pair lists, the (u, v) orientation of every pair included; every graph of every call is compared.

The SQ_MWM_* switches and SQ_NUSS_THREADS are read once per process, so the forms they select run in fresh child processes
(`python -m tests.matching_checks forms NAME`), one per scenario, which print their pair lists; the comparison is made here."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import matching_checks as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: seconds a child process may take: twice its own wall time on an MI355X -- interpreter start, imports, the process's first
#: GPU call and its printing included --, in whole seconds; measured: nolds 2.2 s, hot 2.4 s, mixed 2.1 s, waves8 2.1 s,
#: nuss64 2.1 s, nuss128 2.1 s
CHILD_TIMEOUT = {"nolds": 5, "hot": 5, "mixed": 5, "waves8": 5, "nuss64": 5, "nuss128": 5}

_memo = {}
_dead = []                       # the child that ended by a signal, at its limit or in an error: no further child is started


def _once(key, make):
    """A reference computed once per process and left unchanged."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in M.FORMS_SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _expected(name):
    return _once(("networkx", name), lambda: [M.networkx_pairs(e) for e in M.forms_set(name)])


def _plan(name, **kw):
    graphs = M.forms_set(name)
    plan = M.mwm_launch([M.mwm_dims(e) for e in graphs], **kw)
    assert [f is None for f in plan["forms"]] == [not e for e in graphs]
    # graphs without an edge at the head, in the middle and at the end of the call, and a repeated edge somewhere
    assert not graphs[0] and not graphs[-1] and any(not e for e in graphs[1:-1])
    assert any(len(e) > M.mwm_dims(e)[1] for e in graphs)
    return plan


def _max_degree(edges):
    deg = {}
    for u, v in {(min(u, v), max(u, v)) for u, v, _ in edges}:
        deg[u], deg[v] = deg.get(u, 0) + 1, deg.get(v, 0) + 1
    return max(deg.values(), default=0)


def _forms(plan):
    return {f for f in plan["forms"] if f is not None}


def _check_mwm(name, got, poff):
    graphs, exp = M.forms_set(name), _expected(name)
    assert len(got) == len(graphs) and len(poff) == len(graphs) + 1 and poff[0] == 0
    for g, (e, p) in enumerate(zip(exp, got)):
        assert [tuple(x) for x in p] == e, (name, g, M.mwm_dims(graphs[g]), p[:5], e[:5])
        assert poff[g + 1] - poff[g] == len(e), (name, g)


# ------------------------------------------------------------------ in process: no switch
def test_crowd_of_graphs_hot_parts_in_four_wave_bins_matches_networkx():
    """1,030 graphs in one call are a crowd (sq_mwm_crowd): blocks of 4 waves and 40 KB, every graph with the hot part of its
    state alone in LDS -- the classic blossom cases, the sizes at the edges of the kernel's loops, hubs of 70 and 100
    neighbours, a star, a hub in front of a long odd cycle among a thousand graphs of 2 .. 24 vertices -- but the sparse graph
    of 600 vertices, whose hot part (41,294 bytes with the algorithm object) is beyond a bin: in global memory, on a wave of
    the same launch."""
    graphs = M.forms_set("crowd")
    plan = _plan("crowd")
    dims = [M.mwm_dims(e) for e in graphs]
    assert len(graphs) >= 1024 and M.mwm_crowd(dims) and (plan["waves"], plan["cap"], plan["lds"]) == (4, 40 * 1024, 40 * 1024)
    assert [d for d, f in zip(dims, plan["forms"]) if f == 0] == [(600, 600)] and _forms(plan) == {0, 2}
    assert M.mwm_hot_bytes(600, 600, 2) + 16 + M.MWM_HDR == 41294
    assert max(len(b) for b in plan["bins"]) == 4 and len(plan["bins"][-1]) < 4
    assert {n for n, _ in dims} >= set(M.MWM_EDGE_SIZES) | set(range(2, 25))
    assert sum(1 for e in graphs if _max_degree(e) > 64) >= 3 and any(_max_degree(e) == len(e) >= 100 for e in graphs)     # hubs, a star
    _check_mwm("crowd", *M.mwm_many(graphs))


def test_three_graphs_per_block_match_networkx():
    """600 graphs of 2 .. 40 vertices: three waves per block, all state in LDS."""
    plan = _plan("three")
    assert (plan["waves"], plan["nbins"]) == (3, 200) and _forms(plan) == {1}
    _check_mwm("three", *M.mwm_many(M.forms_set("three")))


def test_one_graph_per_block_all_state_and_hot_part_alone_in_one_launch_match_networkx():
    """24 graphs, one per block: a graph of 300 vertices and 1,800 edges, whose state and edge list (187,694 bytes) are beyond
    the 150 KB a block may have, keeps its hot part (21,782 bytes) in LDS beside graphs of 100 .. 150 vertices that keep all."""
    graphs = M.forms_set("single")
    plan = _plan("single")
    dims = [M.mwm_dims(e) for e in graphs]
    assert len(graphs) < 257 and plan["waves"] == 1
    assert [d for d, f in zip(dims, plan["forms"]) if f == 2] == [(300, 1800)] and _forms(plan) == {1, 2}
    assert (M.mwm_scratch_bytes(300, 1800, 1) + 1800 * 16 + 16, M.mwm_hot_bytes(300, 1800, 2) + 16) == (187694, 21782)
    assert all(100 <= n <= 150 for (n, _), f in zip(dims, plan["forms"]) if f == 1) and plan["forms"].count(1) == 19
    _check_mwm("single", *M.mwm_many(graphs))


def test_nussinov_one_wave_per_problem_matches_oracle():
    """1,034 problems in one call: sq_nussinov_threads gives every block ONE wave (a crowded chip), so a lane takes up to five
    cells of an anti-diagonal of the problems of 65 .. 300 nt."""
    probs = M.nussinov_crowd_set()
    exp = _once("nussinov crowd", lambda: [M.oracle_nussinov(seq, cells) for seq, cells in probs])
    dims = [(len(s), len(c)) for s, c in probs]
    assert len(probs) >= 1024 and M.nussinov_threads(dims) == 64 and M.nussinov_threads(dims[:1023]) == 256
    assert {n for n, _ in dims} >= {63, 64, 65, 128, 129, 192, 193, 256, 257, 300} | set(range(5, 25))
    assert sum(1 for e in exp if e) >= 900 and sum(1 for s, _ in probs if ";" in s or "&" in s) >= 50
    got = M.nussinov_many(probs)
    assert len(got) == len(probs)
    for g, ((seq, cells), e, p) in enumerate(zip(probs, exp, got)):
        assert p == e, (g, len(seq), len(cells), p[:6], e[:6])
        if ";" not in seq and "&" not in seq:
            M.check_nussinov_pairs(len(seq), cells, p)


# ------------------------------------------------------------------ child processes: one switch each
def _child(name):
    """The JSON a scenario's child process prints.  A child that ends by a signal, at its time limit or in an error fails its
    test with the tail of its output, and no further child is started: the remaining tests skip, naming it."""
    if _dead:
        pytest.skip("no further child process after %s" % _dead[0])
    env = {k: v for k, v in os.environ.items() if k not in M.FORMS_SWITCHES}
    env.update(M.FORMS_SCENARIOS[name][0])
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, "-m", "tests.matching_checks", "forms", name], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT[name])
    except subprocess.TimeoutExpired as e:
        _dead.append("the child of '%s', ended at its limit of %d s" % (name, CHILD_TIMEOUT[name]))
        tail = "".join(x.decode(errors="replace") if isinstance(x, bytes) else x or "" for x in (e.stdout, e.stderr))[-2000:]
        pytest.fail("%s\n%s" % (_dead[0], tail))
    print("child %s: %.1f s" % (name, time.time() - t0))
    lines = [x for x in r.stdout.split("\n") if x.startswith("FORMS ")]
    if r.returncode != 0 or len(lines) != 1:
        _dead.append("the child of '%s', ended with status %d" % (name, r.returncode))
        pytest.fail("%s\n%s" % (_dead[0], (r.stdout[-1000:] + r.stderr)[-2000:]))
    return json.loads(lines[0][6:])


def _check_child_mwm(out, sets):
    assert sorted(out) == sorted(sets)
    for s in sets:
        _check_mwm(s, out[s]["pairs"], out[s]["poff"])


def test_everything_in_global_memory_in_both_kernels_matches_networkx():
    """SQ_MWM_NOLDS=1: form 0 for 40 graphs of 63 .. 200 vertices at one graph per block, and for 300 graphs in two-wave bins."""
    env, sets, kw = M.FORMS_SCENARIOS["nolds"]
    few, bins = _plan("few", **kw), _plan("bins", **kw)
    assert (few["waves"], bins["waves"], bins["nbins"]) == (1, 2, 150) and _forms(few) == _forms(bins) == {0}
    _check_child_mwm(_child("nolds"), sets)


def test_hot_part_alone_in_lds_in_both_kernels_matches_networkx():
    """SQ_MWM_ALL_CAP=1: no graph may keep all its state in LDS -- form 2 for the same two calls (at one graph per block every
    graph sees the launch-wide LDS, the hot part of the largest: the 40 graphs are all too large to fit that whole)."""
    env, sets, kw = M.FORMS_SCENARIOS["hot"]
    few, bins = _plan("few", **kw), _plan("bins", **kw)
    assert (few["waves"], bins["waves"], bins["nbins"]) == (1, 2, 150) and _forms(few) == _forms(bins) == {2}
    dims = [M.mwm_dims(e) for e in M.forms_set("bins")]
    assert {n for n, _ in dims} >= set(M.MWM_EDGE_SIZES) and {n for n, _ in (M.mwm_dims(e) for e in M.forms_set("few"))} >= set(M.MWM_EDGE_SIZES)
    _check_child_mwm(_child("hot"), sets)


def test_three_forms_in_one_launch_of_the_bin_kernel_match_networkx():
    """SQ_MWM_BIN_BYTES=8192: of 300 graphs of 2 .. 150 vertices the small ones keep all their state in their slice of the block,
    those of up to about 100 vertices the hot part, the larger ones nothing -- waves of one launch, some of one block."""
    env, sets, kw = M.FORMS_SCENARIOS["mixed"]
    plan = _plan("mixed", **kw)
    assert plan["waves"] == 2 and plan["cap"] == plan["lds"] == M.MIXED_BIN_BYTES
    assert all(plan["forms"].count(f) >= 20 for f in (0, 1, 2)), [plan["forms"].count(f) for f in (0, 1, 2)]
    assert any(len({plan["forms"][q] for q in b}) == 2 for b in plan["bins"])
    assert max(n for n, _ in (M.mwm_dims(e) for e in M.forms_set("mixed"))) == 150
    _check_child_mwm(_child("mixed"), sets)


def test_eight_graphs_per_block_match_networkx():
    """SQ_MWM_BIN_WAVES=8: blocks of 512 threads, 300 graphs with all their state in LDS, the last bin partly filled."""
    env, sets, kw = M.FORMS_SCENARIOS["waves8"]
    plan = _plan("bins", **kw)
    assert 64 * plan["waves"] == 512 and _forms(plan) == {1}
    assert max(len(b) for b in plan["bins"]) == 8 and len(plan["bins"][-1]) < 8
    _check_child_mwm(_child("waves8"), sets)


@pytest.mark.parametrize("threads", [64, 128])
def test_nussinov_block_of_one_and_two_waves_matches_oracle(threads):
    """SQ_NUSS_THREADS: the problems of tests/test_hip_matching_many.py (up to 300 nt, separators among them), which a call of
    their number gives 256 threads, in blocks of 64 and of 128."""
    probs = M.nussinov_problem_set()
    exp = _once("nussinov", lambda: [M.oracle_nussinov(seq, cells) for seq, cells in probs])
    dims = [(len(s), len(c)) for s, c in probs]
    assert M.nussinov_threads(dims) == 256 and M.nussinov_threads(dims, nuss_threads=threads) == threads
    assert max(n for n, _ in dims) == 300 and sum(1 for s, _ in probs if ";" in s or "&" in s) >= 3
    out = _child("nuss%d" % threads)
    assert sorted(out) == ["nussinov"] and len(out["nussinov"]) == len(probs)
    for g, ((seq, cells), e, p) in enumerate(zip(probs, exp, out["nussinov"])):
        p = [tuple(x) for x in p]
        assert p == e, (g, len(seq), len(cells), p[:6], e[:6])
        if ";" not in seq and "&" not in seq:
            M.check_nussinov_pairs(len(seq), cells, p)
