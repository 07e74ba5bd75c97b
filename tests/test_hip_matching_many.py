"""GPU: the graph-level entries sq_nussinov / sq_lsap / sq_mwm (csrc/sq_graph.hip) with SEVERAL problems per call -- the
drop-ins of core.py always pass one, the fold path builds its own job tables --, on adversarial inputs (tests/matching_checks.py)
against the oracle's Nussinov and a plain DP, scipy.optimize.linear_sum_assignment and networkx.max_weight_matching themselves.
Every comparison is exact: integer equality of assignments and pair lists, == on sums of multiples of 1/8."""
import pytest

from tests import matching_checks as M

pytestmark = pytest.mark.gpu

_memo = {}


def _once(key, make):
    """A reference computed once per process and left unchanged."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


# ------------------------------------------------------------------ sq_nussinov
NUSS_SIZES = M.NUSS_SIZES


def _nussinov_problems():
    def make():
        probs = M.nussinov_problem_set()                     # (shared with tests/test_hip_matching_forms.py)
        exp = [M.oracle_nussinov(seq, cells) for seq, cells in probs]
        for (seq, cells), pairs in zip(probs, exp):          # the reference itself is an optimum (test_matching_reference.py)
            if ";" not in seq and "&" not in seq:
                M.check_nussinov_pairs(len(seq), cells, pairs)
        return probs, exp
    return _once("nussinov", make)


def _check_nussinov(probs, exp, got):
    assert len(got) == len(probs)
    for g, ((seq, cells), e, p) in enumerate(zip(probs, exp, got)):
        assert p == e, (g, len(seq), len(cells), p[:6], e[:6])
        if ";" not in seq and "&" not in seq:
            M.check_nussinov_pairs(len(seq), cells, p)


def test_nussinov_many_problems_per_call_match_oracle_and_plain_dp():
    probs, exp = _nussinov_problems()
    assert len(probs) >= 40 and {len(s) for s, _ in probs} == set(NUSS_SIZES)
    assert sum(1 for e in exp if e) >= 30 and sum(1 for s, _ in probs if ";" in s or "&" in s) >= 3
    _check_nussinov(probs, exp, M.nussinov_many(probs))


def test_nussinov_one_problem_per_call_gives_the_same_lists():
    probs, exp = _nussinov_problems()
    _check_nussinov(probs, exp, [M.nussinov_many([p])[0] for p in probs])


@pytest.mark.parametrize("first", ["largest", "n1"])
def test_nussinov_first_problem_of_a_call(first):
    """Every problem's count is filed under its own index: a call that begins with the largest problem, one that begins
    with n = 1 (whose count is 0 and whose block ends first)."""
    probs, exp = _nussinov_problems()
    order = sorted(range(len(probs)), key=lambda g: -len(probs[g][0]) if first == "largest" else (len(probs[g][0]) != 1, g))
    assert len(probs[order[0]][0]) == (300 if first == "largest" else 1)
    assert len(exp[order[0]]) > 10 if first == "largest" else exp[order[0]] == []
    sub = [probs[g] for g in order]
    _check_nussinov(sub, [exp[g] for g in order], M.nussinov_many(sub))
    two = [sub[0], sub[1], sub[0]]                           # ... and the same problem at both ends of a short call
    _check_nussinov(two, [exp[order[0]], exp[order[1]], exp[order[0]]], M.nussinov_many(two))


# ------------------------------------------------------------------ sq_lsap
def _lsap_problems():
    def make():
        import numpy as np
        fams = M.DYADIC + (M.CONTINUOUS,)
        probs = [M.lsap_case(4000, 0, 0), M.lsap_case(4001, 1, 0), M.lsap_case(4002, 2, 0), M.lsap_case(4003, 2, 1),
                 M.lsap_case(4004, 3, 0), M.lsap_case(4005, 3, 2, M.DYADIC[0]), M.lsap_case(4006, 3, 3, M.CONTINUOUS, repeats=0.7)]
        # one mask word and two (31, 32, 33), the wave (63, 64, 65), one scan chunk of 192 columns and two (192, 193), 385;
        # m = 0 is the all-zero matrix: nothing but the tie rule
        for t, n in enumerate((31, 32, 33, 63, 64, 65, 192, 193, 385)):
            for d, m in enumerate((0, n // 2, 2 * n, 8 * n)):
                probs.append(M.lsap_case(4100 + 10 * t + d, n, m, fams[(t + d) % 4]))
        probs.append(M.lsap_case(4200, 40, 40 * 39 // 2, M.DYADIC[1]))           # dense: every cell set
        probs.append(M.lsap_case(4201, 40, 40 * 39 // 2, M.CONTINUOUS))
        order = np.random.default_rng(41).permutation(len(probs))
        probs = [probs[int(t)] for t in order]
        return probs, [M.scipy_col_ind(n, cells) for n, cells in probs]
    return _once("lsap", make)


def _check_lsap(probs, exp, got):
    assert len(got) == len(probs)
    for g, ((n, cells), e, c) in enumerate(zip(probs, exp, got)):
        assert c == e, (g, n, len(cells), [(r, c[r], e[r]) for r in range(n) if c[r] != e[r]][:5])


def test_lsap_many_problems_per_call_match_scipy():
    probs, exp = _lsap_problems()
    assert 40 <= len(probs) <= 50
    dims = [(n, len(M.dedup_cells(cells))) for n, cells in probs]
    assert all(M.lsap_form(n, m, dims) == "a" for n, m in dims if n)
    assert any(v > w for _, cells in probs for v, w, _ in cells)
    assert any(len(M.dedup_cells(cells)) < len(cells) for _, cells in probs)
    _check_lsap(probs, exp, M.lsap_many(probs))
    for g in (0, 7, len(probs) - 1):                         # ... and alone: the same slice
        assert M.lsap_many([probs[g]]) == [exp[g]]


def _big(n, m, seed):
    """(problem, scipy's col_ind, distinct cells), once per process."""
    def make():
        prob = M.lsap_case(seed, n, m, M.DYADIC[2])
        return prob, M.scipy_col_ind(*prob), len(M.dedup_cells(prob[1]))
    return _once(("big", n, m, seed), make)


def test_lsap_dense_cost_in_global_memory_matches_scipy():
    """Form (b): n = 800, m = 3,000 -- sq_lsap_lds_bytes(800, 3000) = 191,284 bytes, over the 150 KB (153,600 bytes) a block
    may have (155,284 already without a cell; 123,284 at n = 700), so the cost matrix is dense in global memory and the
    vectors (33,600 bytes) stay in LDS."""
    prob, exp, m = _big(800, 3000, 4300)
    assert m == 3000 and M.lsap_lds_bytes(800, m) == 191284 and M.lsap_form(800, m, [(800, m)]) == "b"
    _check_lsap([prob], [exp], M.lsap_many([prob]))


def test_lsap_last_size_with_vectors_in_lds_matches_scipy():
    """n = 3,655: sq_lsap_vec_bytes + 64 = 153,584 bytes, the last size of form (b)."""
    prob, exp, m = _big(3655, 6000, 4301)
    assert M.lsap_vec_bytes(3655) + 64 == 153584 and M.lsap_form(3655, m, [(3655, m)]) == "b"
    _check_lsap([prob], [exp], M.lsap_many([prob]))


def test_lsap_everything_in_global_memory_matches_scipy():
    """n = 3,656: sq_lsap_vec_bytes + 64 = 153,616 bytes, the first size of form (c) -- vectors in global scratch, lane 0's
    stores fenced before the wave's reads."""
    prob, exp, m = _big(3656, 6000, 4302)
    assert M.lsap_vec_bytes(3656) + 64 == 153616 and M.lsap_form(3656, m, [(3656, m)]) == "c"
    _check_lsap([prob], [exp], M.lsap_many([prob]))


def test_lsap_three_storage_forms_in_one_launch_match_scipy():
    """n = 3,656 beside n = 100 and n = 800: forms (c), (a) and (b) under one launch-wide LDS size; the largest n and the largest
    sparse form belong to different problems."""
    big, big_exp, bm = _big(3656, 6000, 4302)
    mid, mid_exp, mm = _big(800, 3000, 4300)
    small = M.lsap_case(4303, 100, 200, M.DYADIC[1])
    dims = [(3656, bm), (100, len(M.dedup_cells(small[1]))), (800, mm)]
    assert [M.lsap_form(n, m, dims) for n, m in dims] == ["c", "a", "b"]
    _check_lsap([big, small, mid], [big_exp, M.scipy_col_ind(*small), mid_exp], M.lsap_many([big, small, mid]))


# ------------------------------------------------------------------ sq_mwm
def _mwm_graphs():
    def make():
        import numpy as np
        rng = np.random.default_rng(51)
        graphs = []
        for g in range(300):
            n = 2 + g % 39 if g < 78 else int(rng.integers(2, 41))       # every size of 2..40 twice, then at random
            graphs.append(M.mwm_case(5000 + g, n, zero_edges=g in (0, 7, 130, 131, 258, 299), repeat_edge=g % 50 == 3))
        return graphs, [M.networkx_pairs(e) for e in graphs]
    return _once("mwm", make)


@pytest.mark.parametrize("count", [1, 2, 300])
def test_mwm_many_graphs_per_call_match_networkx(count):
    """1 and 2 graphs: one graph per block (sq_mwm_single_kernel); 300: two graphs per block, one per wave (sq_mwm_kernel, from
    257 graphs on), the last bin half full.  Pairs and their (u, v) orientation as networkx returns them, sorted."""
    graphs, exp = _mwm_graphs()
    first = {1: 3, 2: 6, 300: 0}[count]                      # (graph 3 has the repeated edge, graph 7 no edge)
    sub, sub_exp = graphs[first:first + count], exp[first:first + count]
    got, poff = M.mwm_many(sub)
    assert len(got) == count and len(poff) == count + 1
    for g in range(count):
        assert got[g] == sub_exp[g], (g, len(sub[g]), got[g][:5], sub_exp[g][:5])
        assert poff[g + 1] - poff[g] == len(sub_exp[g])
    assert poff[0] == 0 and poff[-1] == sum(len(e) for e in sub_exp)
    if count == 300:
        assert sum(1 for e in sub if not e) == 6 and sum(1 for e in sub_exp for u, v in e if u > v) > 100
        labels = {u for e in sub for u, _, _ in e}
        assert min(labels) >= 7 and all((u - 7) % 3 == 0 for u in labels)


# ------------------------------------------------------------------ refusals (before any kernel is launched, or after all have ended)
def _refused(call, code, text):
    from squarna_amd import _lib
    with pytest.raises(_lib.CapacityError if code == -3 else RuntimeError, match=text) as err:
        call()
    assert ("(code %d)" % code) in str(err.value) and text in M.last_error()


def test_refusals_return_their_codes_and_a_correct_call_follows():
    seq, cells = M.nussinov_case(6000, 40, 60)
    exp = M.oracle_nussinov(seq, cells)
    assert len(exp) >= 3
    good = lambda: M.nussinov_many([("A", []), (seq, cells)]) == [[], exp]
    uniq = [(v, w, x) for (v, w), x in M.dedup_cells(cells).items()]    # (the workspace sizes count a repeated cell twice)
    assert good()
    for call, code, text in (
            (lambda: M.nussinov_many([(seq, cells), (seq, [(9, 2, 1.0)])]), -1, "Nussinov cells must have v < w"),
            (lambda: M.nussinov_many([(seq, cells + [(3, 40, 1.0)])]), -1, "cell outside the matrix"),
            (lambda: M.nussinov_many([(seq, cells + [(5, 5, 1.0)])]), -1, "cell outside the matrix"),
            (lambda: M.nussinov_many([(seq, cells), ("A" * 32001, [])]), -1, "matrix size out of range"),
            (lambda: M.lsap_many([(40, cells), (32001, [])]), -1, "matrix size out of range"),
            (lambda: M.lsap_many([(40, cells + [(40, 3, 1.0)])]), -1, "cell outside the matrix"),
            (lambda: M.mwm_many([[(1, 2, 1.0)], [(3, -4, 1.0)]]), -1, "non-negative"),
            (lambda: M.nussinov_many([(seq, uniq)], ws_short=1), -2, "workspace too small"),
            (lambda: M.lsap_many([(40, uniq)], ws_short=1), -2, "workspace too small"),
            (lambda: M.mwm_many([uniq], ws_short=1), -2, "workspace too small"),
            (lambda: M.nussinov_many([(seq, cells)], ws_shift=8), -2, "256-byte aligned"),
            (lambda: M.lsap_many([(40, cells)], ws_shift=8), -2, "256-byte aligned"),
            (lambda: M.mwm_many([cells], ws_shift=8), -2, "256-byte aligned"),
            (lambda: M.nussinov_many([("A", []), (seq, cells)], pair_cap=len(exp) - 1), -3, "pair_cap too small"),
            (lambda: M.mwm_many([[], cells], pair_cap=len(M.networkx_pairs(cells)) - 1), -3, "pair_cap too small")):
        _refused(call, code, text)
        assert good()
    assert M.nussinov_many([("A", []), (seq, cells)], pair_cap=len(exp)) == [[], exp]       # the exact capacity holds
