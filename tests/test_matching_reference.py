"""The references of tests/test_hip_matching_many.py against each other, on the CPU: the oracle's Nussinov (the C restatement
of SQRNalgos.py:44-93) and the plain fp64 DP of tests/matching_checks.py must agree on the generators' cases before either
judges the kernel, and scipy_col_ind must give the assignments of two matrices small enough to solve by hand."""
import pytest

from tests import matching_checks as M

#: (seed, n, cells, weight family): about 60 cases of n = 2..70, cell counts from none to 3 n
SMALL = [(1000 + t, 2 + (t * 37) % 69, ((0, 1, 3, 8, 20)[t % 5] * (2 + (t * 37) % 69)) // 7, (M.DYADIC + (M.DYADIC[2],))[t % 4])
         for t in range(60)]
LARGE = [(2001, 257, 700, M.DYADIC[2]), (2002, 300, 900, M.DYADIC[1])]


def test_small_case_sizes_cover_the_range():
    ns = sorted({c[1] for c in SMALL})
    assert ns[0] == 2 and ns[-1] == 70 and len(ns) >= 50
    assert max(c[2] / c[1] for c in SMALL) > 2.5 and any(c[2] == 0 for c in SMALL)


@pytest.mark.parametrize("seed,n,ncells,family", SMALL + LARGE, ids=lambda v: str(v) if isinstance(v, int) else "w%d" % len(v))
def test_oracle_nussinov_is_an_optimum_of_the_plain_dp(seed, n, ncells, family):
    """The oracle's pairs are cells of the input, vertex-disjoint, nested, and their scores sum to -D[0][n-1] of the plain DP."""
    seq, cells = M.nussinov_case(seed, n, ncells, family)
    assert len(seq) == n and all(w - v >= 4 and 0 <= v and w < n for v, w, _ in cells)
    pairs = M.oracle_nussinov(seq, cells)
    M.check_nussinov_pairs(n, cells, pairs)
    if n >= 5 and ncells:
        assert pairs and M.nussinov_optimum(n, cells) < 0


def test_generator_repeats_cells_with_other_scores():
    seq, cells = M.nussinov_case(7, 60, 150)
    keys = [(v, w) for v, w, _ in cells]
    assert len(set(keys)) < len(keys)
    assert any(a[:2] == b[:2] and a[2] != b[2] for k, a in enumerate(cells) for b in cells[k + 1:])
    n, lc = M.lsap_case(7, 40, 200)
    assert any(v > w for v, w, _ in lc) and len(M.dedup_cells(lc)) == 200 < len(lc)


def test_nussinov_degenerate_cases():
    for n in (0, 1, 5):
        assert M.oracle_nussinov("A" * n, []) == [] and M.nussinov_optimum(n, []) == 0.0
    for n in (5, 6, 64):
        cells = [(0, n - 1, 1.5)]
        assert M.oracle_nussinov("A" * n, cells) == [(0, n - 1)] and M.nussinov_optimum(n, cells) == -1.5
        M.check_nussinov_pairs(n, cells, [(0, n - 1)])
    # a repeated cell takes the last score; two nested cells and one that crosses them
    cells = [(0, 9, 1.0), (1, 8, 2.0), (2, 12, 2.0), (0, 9, 0.5)]
    assert M.nussinov_optimum(13, cells) == -2.5 and M.dedup_cells(cells)[(0, 9)] == 0.5
    assert M.oracle_nussinov("A" * 13, cells) == [(0, 9), (1, 8)]
    M.check_nussinov_pairs(13, cells, [(0, 9), (1, 8)])
    with pytest.raises(AssertionError):
        M.check_nussinov_pairs(13, cells, [(2, 12)])                    # a valid structure, but 2.0 is not the optimum
    with pytest.raises(AssertionError):
        M.check_nussinov_pairs(13, cells, [(1, 8), (2, 12)])            # crossing


def test_scipy_col_ind_on_hand_made_matrices():
    # 3 x 3, the one cell (0, 2) of weight 2: rows 0 and 2 take each other's column (cost -4, the cell counts in both
    # orientations), every other permutation costs 0 or -2
    assert M.scipy_col_ind(3, [(0, 2, 2.0)]) == [2, 1, 0]
    # 4 x 4, cells (0,1) = 3, (1,2) = 4.5, (2,3) = 3, (0,3) = 0.5 and (0,1) again as (1, 0) with weight 1, which wins:
    #   0<->3 with 1<->2 costs -(0.5 + 0.5 + 4.5 + 4.5) = -10; 1<->2 alone -9; the cycle 0->1->2->3->0 -(1 + 4.5 + 3 + 0.5) = -9;
    #   0<->1 with 2<->3 -(1 + 1 + 3 + 3) = -8 -- it would cost -12 and win had the first weight of (0, 1) stayed
    cells = [(0, 1, 3.0), (1, 2, 4.5), (2, 3, 3.0), (0, 3, 0.5), (1, 0, 1.0)]
    assert M.scipy_col_ind(4, cells) == [3, 2, 1, 0]
    assert M.scipy_col_ind(4, cells[:4]) == [1, 0, 3, 2]
    # all zero: scipy's own tie rule, pinned here as the identity
    assert M.scipy_col_ind(3, []) == [0, 1, 2]
    assert M.scipy_col_ind(0, []) == [] and M.scipy_col_ind(1, []) == [0]


def test_lsap_forms_by_size():
    """The sizes the GPU test picks for the three storage forms of sq_lsap_kernel, from the byte counts of csrc/sq_match.h."""
    assert M.lsap_lds_bytes(800, 3000) == 191284 and M.lsap_lds_bytes(800, 0) > M.LSAP_LDS_CAP > M.lsap_lds_bytes(700, 0)
    assert M.lsap_form(385, 3080, [(385, 3080)]) == "a"
    assert M.lsap_form(800, 3000, [(800, 3000)]) == "b"
    assert M.lsap_form(3655, 6000, [(3655, 6000)]) == "b" and M.lsap_form(3656, 6000, [(3656, 6000)]) == "c"
    mixed = [(3656, 6000), (100, 200), (800, 3000)]
    assert [M.lsap_form(n, m, mixed) for n, m in mixed] == ["c", "a", "b"]
