"""CPU tests of Distances() / DistancesResult (no GPU): the numpy path under the test-only OracleEngine against the naive
reference of tests/distances_checks.py (sets of pairs).  Integer comparisons are exact; f1 and the means are one IEEE
division of two exact integers and are compared with Python's own quotient with ==."""
import numpy as np
import pytest

from squarna_amd import engine as E
from tests.distances_checks import as_lists, chain_rows, check_result, distance_matrix, family_rows, naive, pairs_of, partners_of, random_rows
from tests.oracle_engine import OracleEngine


def distances(structures, **kw):
    from squarna_amd import Distances
    with E.use_engine(OracleEngine()):
        return Distances(structures, **kw)


def threshold_of(kw):
    if "relative" in kw:
        return "relative", int(round(kw["relative"] * 10000))
    return "radius", kw.get("radius", 0)


def check(res, groups, **kw):
    import torch
    S = sum(len(g) for g in groups)
    mode, threshold = threshold_of(kw)
    assert res.source == "host" and res.device.type == "cpu" and (res.S, res.G, len(res)) == (S, len(groups), S)
    assert (res.radius, res.relative_bp) == ((threshold, None) if mode == "radius" else (None, threshold))
    for key in ("status", "npairs", "neighbours", "leader"):
        assert getattr(res, key).dtype == torch.int32 and tuple(getattr(res, key).shape) == (S,), key
    assert res.keep.dtype == torch.bool and res.row_off.dtype == res.mat_off.dtype == torch.int64
    off = np.concatenate(([0], np.cumsum([len(g) for g in groups])))
    assert res.row_off.tolist() == off.tolist() and res.mat_off.tolist() == np.concatenate(([0], np.cumsum(np.diff(off) ** 2))).tolist()
    check_result(as_lists(res), naive(groups, mode, threshold, res.common is not None), ([len(g) for g in groups], mode, threshold))


SIZES = [0, 1, 3, 64, 65, 2, 0, 130]


def grouped(seed, sizes, L, **kw):
    rows = family_rows(seed, sum(sizes), L, **kw)
    cut = np.concatenate(([0], np.cumsum(sizes))).tolist()
    return [rows[a:b] for a, b in zip(cut, cut[1:])]


@pytest.mark.parametrize("sizes,L", [([1], 1), ([2], 2), ([11], 30), ([65], 70), ([129], 40), (SIZES, 33)])
def test_the_numpy_path_against_the_naive_reference(sizes, L):
    groups = grouped(sum(sizes) * 1000 + L, sizes, L, families=3, knots=L % 2 == 0)
    for kw in (dict(), dict(radius=0), dict(radius=1), dict(radius=4), dict(relative=0.0), dict(relative=0.25), dict(relative=1.0)):
        check(distances(groups, **kw), groups, **kw)
    res = distances(groups)
    assert (res.groups, res.radius, res.relative_bp) == ("record", 0, None) and res.names == [">record%d" % (k + 1) for k in range(len(sizes))]
    everything = [[r for g in groups for r in g]]
    check(distances(groups, groups="all", radius=2), everything, radius=2)


def test_groups_all_takes_rows_of_different_widths():
    groups = [family_rows(3, 6, 12), family_rows(4, 5, 30), ["()", ".."]]
    res = distances(groups, groups="all", radius=1, names=["a", "b", "c"])
    # (the naive reference reads pairs, not widths: columns beyond a row's width are unpaired)
    check(res, [[r for g in groups for r in g]], radius=1)
    assert res.names == ["a", "b", "c"] and res.G == 1 and res.rows_of(0) == (0, 13)


def test_keyword_errors():
    rows = [["(())", "(..)"]]
    for kw in (dict(radius=1, relative=0.5), dict(radius=-1), dict(radius=1.5), dict(radius=True), dict(radius="2"), dict(relative=1.5),
               dict(relative=-0.1), dict(relative="high"), dict(groups="records"), dict(groups=None), dict(matrix="yes"), dict(matrix=1.5),
               dict(names=["one", "two"]), dict(nstruct=[1])):
        with pytest.raises(ValueError, match="Distances"):
            distances(rows, **kw)
    for structures in (None, "(())", ["(())"], [["(())", "(.)"]], np.zeros((2, 3), np.int32), np.zeros((1, 2, 3), np.float32)):
        with pytest.raises(ValueError, match="Distances"):
            distances(structures)


def padded(groups, dtype=np.int32):
    K, Lmax = max(len(g) for g in groups), max(len(r) for g in groups for r in g)
    out = np.full((len(groups), K, Lmax), -1, dtype)
    for r, g in enumerate(groups):
        for k, dbn in enumerate(g):
            out[r, k, :len(dbn)] = partners_of(dbn)
    return out, np.array([len(g) for g in groups])


def test_the_three_input_forms_give_one_result():
    import torch
    from squarna_amd import Fold
    groups = grouped(11, [4, 0, 7, 1], 25, families=2, knots=True)
    strings = distances(groups, radius=2)
    arr, nstruct = padded(groups)
    for form in (arr, arr.astype(np.int16), arr.astype(np.int64), torch.from_numpy(arr)):
        res = distances(form, nstruct=nstruct, radius=2)
        assert as_lists(res) == as_lists(strings) and res.row_off.tolist() == strings.row_off.tolist()
    full = distances(arr[:, :1, :], radius=2)                            # (without nstruct: all K rows of every record)
    assert full.S == 4 and full.row_off.tolist() == [0, 1, 2, 3, 4]
    with E.use_engine(OracleEngine()):
        fold = Fold(records=["GGGAAAACCCAAGGGAAACCC", "GGGGAAAACCCC", "ACGUACGUAGCUAGCUAGCGC"], configfile="nobpp")
        res = distances(fold, radius=1)
        rows = [[fold.consensus(r)] + [fold.dbn(r, k) for k in range(int(fold.nstruct[r]))] for r in range(len(fold))]
    assert res.names == list(fold.names) and res.S == sum(len(g) for g in rows)
    check(res, rows, radius=1)


def test_strict_and_invalid_rows():
    arr, nstruct = padded([["(())..", "(())..", "......"], ["((()))", "(....)"]])
    arr[0, 1, 0] = 0                                                      # p[i] == i
    arr[1, 1, 5] = 1                                                      # p[p[5]] = p[1] = -1 != 5
    with pytest.raises(ValueError, match=r"Distances: record 0 \(>record1\), row 1"):
        distances(arr, nstruct=nstruct)
    res = distances(arr, nstruct=nstruct, strict=False, radius=4)
    exp = naive([["(())..", None, "......"], ["((()))", None]], "radius", 4)
    check_result(as_lists(res), exp)
    assert res.status.tolist() == [0, 1, 0, 0, 1] and res.leader.tolist() == [0, -1, 0, 3, -1] and res.neighbours.tolist() == [2, 0, 2, 1, 0]
    # (an invalid row is no candidate, and counts as an empty structure in the others' sums: row 0 has 2 + 2, row 2 has 2 + 0)
    assert res.medoid().tolist() == [2, 3] and res.distance_of(0, 1)["neighbours"] is False and res.kept().tolist() == [0, 3]
    for bad in ([7, -1, -1], [-2, -1, -1], [1, 2, 0]):
        with pytest.raises(ValueError, match="row 0"):
            distances(np.array([[bad]], np.int32))


def test_matrix_false_refuses_the_matrix_methods():
    groups = grouped(2, [5, 3], 20)
    res = distances(groups, matrix=False, radius=2)
    check(res, groups, radius=2)
    assert res.common is None
    for call in (lambda: res.common_of(0), lambda: res.distance(0), lambda: res.f1(0), lambda: res.distance_of(0, 1), lambda: res.nearest(0),
                 lambda: res.mean_distance(), lambda: res.medoid(), lambda: res.neighbours_at(radius=1)):
        with pytest.raises(ValueError, match="matrix=True"):
            call()
    assert res.kept().tolist() == [a for a, k in enumerate(naive(groups, "radius", 2)["keep"]) if k]
    assert distances(groups, matrix=True).common is not None and distances(groups).common is not None


def test_the_derived_methods_against_the_naive_reference():
    import torch
    groups = grouped(9, [7, 0, 1, 12, 2], 24, families=2, edits=2, knots=True) + [["....", "...."]]
    res = distances(groups, relative=0.3)
    exp = naive(groups, "relative", 3000)
    first = 0
    means, medoids = [], []
    for g, rows in enumerate(groups):
        n, d = len(rows), distance_matrix(rows)
        sets = [pairs_of(r) for r in rows]
        assert res.rows_of(g) == (first, n)
        assert res.distance(g).tolist() == d and res.distance(g).dtype == torch.int64 and tuple(res.distance(g).shape) == (n, n)
        assert res.common_of(g).tolist() == [[len(a & b) for b in sets] for a in sets]
        f1 = [[2 * len(a & b) / (len(a) + len(b)) if len(a) + len(b) else 1.0 for b in sets] for a in sets]
        assert res.f1(g).tolist() == f1 and res.f1(g).dtype == torch.float64
        best, at = res.nearest(g)
        others = [[(d[a][b], b) for b in range(n) if b != a] for a in range(n)]
        assert best.tolist() == [min(o)[0] if o else 0 for o in others] and at.tolist() == [first + min(o)[1] if o else -1 for o in others]
        pairs = n * (n - 1) // 2
        means.append(sum(d[a][b] for a in range(n) for b in range(a + 1, n)) / pairs if pairs else 0.0)
        sums = [sum(row) for row in d]
        medoids.append(first + sums.index(min(sums)) if n else -1)
        for a in range(n):
            for b in range(n):
                rec = res.distance_of(first + a, first + b)
                assert rec == dict(common=len(sets[a] & sets[b]), npairs_a=len(sets[a]), npairs_b=len(sets[b]), distance=d[a][b], f1=f1[a][b],
                                   neighbours=a != b and d[a][b] * 10000 <= 3000 * (len(sets[a]) + len(sets[b])))
        first += n
    assert res.mean_distance().tolist() == means and res.mean_distance().dtype == torch.float64
    assert res.medoid().tolist() == medoids and res.medoid().dtype == torch.int64
    assert res.neighbours_at(relative=0.3).tolist() == exp["neighbours"] and res.neighbours_at(relative=0.3).dtype == torch.int32
    for kw in (dict(radius=0), dict(radius=3), dict(relative=0.0), dict(relative=1.0), dict()):
        assert res.neighbours_at(**kw).tolist() == naive(groups, *threshold_of(kw))["neighbours"], kw
    with pytest.raises(ValueError, match="neighbours_at"):
        res.neighbours_at(radius=1, relative=0.1)
    with pytest.raises(ValueError, match="one group"):
        res.distance_of(0, 8)
    kept = [a for a, k in enumerate(exp["keep"]) if k]
    leaders, sizes = res.clusters()
    assert res.kept().tolist() == leaders.tolist() == kept and sizes.tolist() == [exp["leader"].count(a) for a in kept] and int(sizes.sum()) == res.S


def test_ties_go_to_the_lowest_row():
    rows = ["(())....", "....(())", "(())....", "........", "....(())"]    # rows 0 = 2, 1 = 4; row 3 is 2 away from everyone
    res = distances([rows], radius=0)
    assert res.nearest(0)[1].tolist() == [2, 4, 0, 0, 1] and res.nearest(0)[0].tolist() == [0, 0, 0, 2, 0]
    assert res.medoid().tolist() == [3]                                    # sums 10 10 10 8 10
    assert distances([["()..", "..()"]]).medoid().tolist() == [0] and distances([["()"]]).nearest(0)[1].tolist() == [-1]
    assert res.leader.tolist() == [0, 1, 0, 3, 1] and [t.tolist() for t in res.clusters()] == [[0, 1, 3], [2, 2, 1]]
    chain = distances([chain_rows(9)], radius=2)
    assert chain.keep.tolist() == [k % 2 == 0 for k in range(9)] and chain.leader.tolist() == [k - k % 2 for k in range(9)]


def test_no_rows_and_cpu():
    import torch
    for structures in ([], [[], []], np.zeros((0, 2, 5), np.int32), np.zeros((2, 3, 5), np.int32)):
        kw = dict(nstruct=[0, 0]) if hasattr(structures, "shape") and structures.shape[0] else {}
        res = distances(structures, **kw)
        assert res.S == 0 and res.status.numel() == 0 and res.common.numel() == 0 and res.keep.dtype == torch.bool
        assert res.kept().tolist() == [] and res.mean_distance().tolist() == [0.0] * res.G and res.medoid().tolist() == [-1] * res.G
        assert res.neighbours_at(radius=3).tolist() == [] and [t.tolist() for t in res.clusters()] == [[], []]
    res = distances([random_rows(1, 4, 12)], radius=3)
    host = res.cpu()
    assert host is not res and as_lists(host) == as_lists(res) and host.row_off.tolist() == res.row_off.tolist() and host.radius == 3
