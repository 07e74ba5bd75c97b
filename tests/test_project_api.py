"""CPU tests of Project() / Lift() and their results (no GPU): the numpy path under the test-only OracleEngine against the
naive reference of tests/project_checks.py (plain loops over characters), against dbn.UnAlign / dbn.ReAlign and the oracle's
UnAlign row by row, and against Covariation on the example alignment.  All comparisons are exact."""
import numpy as np
import pytest

from squarna_amd import dbn as D
from squarna_amd import engine as E
from squarna_amd.project import CLASSES
from tests.oracle_engine import OracleEngine
from tests.project_checks import (GAP_CHARS, WIDTHS, aligned_rows, check_equal, class_line, lift_lists, naive, naive_lift, project_lists,
                                  short_lines, special_rows, structure_line)

ALI = "examples/ali_input.afa"


def project(**kw):
    from squarna_amd import Project
    with E.use_engine(OracleEngine()):
        return Project(**kw)


def lift(**kw):
    from squarna_amd import Lift
    with E.use_engine(OracleEngine()):
        return Lift(**kw)


def pairs_of(p):
    return [(v, w) for v, w in enumerate(p) if w > v]


def as_dbn(p):
    return D.PairsToDBN(pairs_of(p), len(p))


def partners_of(line):
    p = [-1] * len(line)
    for v, w in D.DBNToPairs(line):
        p[v], p[w] = w, v
    return p


def padded(short, width=None):
    """int64[R, K, width]: per row K partner lists over its residues, -1 padding."""
    K = max(len(mine) for mine in short)
    width = max(max((len(p) for mine in short for p in mine), default=0), 1) if width is None else width
    out = np.full((len(short), K, width), -1, np.int64)
    for r, mine in enumerate(short):
        for k, p in enumerate(mine):
            out[r, k, :len(p)] = p
    return out


@pytest.fixture(scope="module")
def folded():
    from squarna_amd import FoldAlignment
    with E.use_engine(OracleEngine()):
        return FoldAlignment(inputfile=ALI)


def check_types(res, R, L, K):
    import torch
    Lmax = max(int(res.length.max()), 1)
    assert res.source == "host" and res.device.type == "cpu" and (res.R, res.L, res.K, len(res)) == (R, L, K, R)
    for key, shape, dtype in (("length", (R,), torch.int32), ("col_of", (R, Lmax), torch.int32), ("pos_of", (R, L), torch.int32),
                              ("partner", (R, K, Lmax), torch.int32), ("cls", (R, K, L), torch.uint8), ("counts", (R, K, 12), torch.int32),
                              ("status", (R, K), torch.int32)):
        t = getattr(res, key)
        assert tuple(t.shape) == shape and t.dtype == dtype, key


@pytest.mark.parametrize("L", WIDTHS)
def test_the_numpy_path_against_the_naive_reference(L):
    rows = aligned_rows(L, 6, L) + special_rows(L)
    for K in (1, 3):
        shared = [structure_line(10 * L + k, L, knots=k == 1) for k in range(K)]
        per_row = [[class_line(row)] + [structure_line(100 * L + 10 * r + k, L) for k in range(K - 1)] for r, row in enumerate(rows)]
        for canonical_only in (False, True):
            for min_loop in (0, 3, L):
                res = project(sequences=rows, structures=np.array(shared), canonical_only=canonical_only, min_loop=min_loop)
                check_types(res, len(rows), L, K)
                assert res.shared and (res.canonical_only, res.min_loop, res.strict) == (canonical_only, min_loop, True)
                check_equal(project_lists(res), naive(rows, shared, canonical_only, min_loop), (L, K, canonical_only, min_loop))
        res = project(sequences=rows, structures=np.array(per_row), min_loop=2)
        assert not res.shared
        check_equal(project_lists(res), naive(rows, per_row, False, 2), (L, K, "per row"))
        short = short_lines(L + K, rows, K, knots=True)
        got = lift(sequences=rows, structures=padded(short))
        check_equal(lift_lists(got, [K] * len(rows)), naive_lift(rows, short), (L, K, "lift"))


def test_the_defaults_are_unalign_row_by_row():
    from oracle import sqrn_oracle as O
    L = 90
    rows = aligned_rows(5, 9, L, letters="ACGUacgutTN-.~") + special_rows(L)
    lines = [structure_line(1, L), structure_line(2, L, knots=True), class_line(rows[0])]
    res = project(sequences=rows, structures=[as_dbn(p) for p in lines], names=["r%d" % r for r in range(len(rows))])
    assert res.names[3] == "r3" and res.sequences == rows
    for r, seq in enumerate(rows):
        for k, p in enumerate(lines):
            line = as_dbn(p)
            shortseq, shortdbn, pairs = D.UnAlign(seq, line, want_pairs=True)
            if pairs is None:                                            # a row without gaps: the line as it is
                pairs = D.DBNToPairs(shortdbn)
            n = int(res.length[r])
            assert res.sequence(r) == shortseq and n == len(shortseq)
            assert pairs_of(res.partner[r, k, :n].tolist()) == sorted(pairs), (r, k)
            assert D.DBNToPairs(res.dbn(r, k)) == sorted(pairs) and len(res.dbn(r, k)) == n
            oseq, odbn = O.UnAlign(seq, line)
            assert oseq == shortseq and pairs_of(res.partner[r, k, :n].tolist()) == D.DBNToPairs(odbn)
    assert res.records() == (res.names, [res.sequence(r) for r in range(len(rows))]) and res.to_padded() is res.partner


def test_lift_is_realign_and_the_round_trip_holds():
    L = 75
    rows = aligned_rows(8, 7, L) + special_rows(L)
    short = short_lines(3, rows, 2, knots=True)
    as_strings = [[as_dbn(p) for p in mine] for mine in short]
    res = lift(sequences=rows, structures=as_strings)
    assert res.K == 2 and res.nstruct.tolist() == [2] * len(rows) and res.source == "host" and res.to_padded() is res.partner
    for r, seq in enumerate(rows):
        for k, line in enumerate(as_strings[r]):
            assert res.partner[r, k].tolist() == partners_of(D.ReAlign(line, seq)), (r, k)
            assert D.DBNToPairs(res.dbn(r, k)) == pairs_of(res.partner[r, k].tolist()) and len(res.dbn(r, k)) == L
    assert lift(sequences=rows, structures=padded(short)).partner.tolist() == res.partner.tolist()
    back = project(sequences=rows, structures=res.partner)
    assert not back.shared and back.partner.tolist() == padded(short, int(back.partner.shape[2])).tolist()
    assert back.counts[..., 11].tolist() == back.counts[..., 0].tolist() and not back.counts[..., 8:11].any()
    # rows with 0, 1 or 2 lines
    some = [mine[:r % 3] for r, mine in enumerate(as_strings)]
    res = lift(sequences=rows, structures=some)
    check_equal(lift_lists(res, [r % 3 for r in range(len(rows))]), naive_lift(rows, [mine[:r % 3] for r, mine in enumerate(short)]))
    same = lift(sequences=rows, structures=padded(short), nstruct=[r % 3 for r in range(len(rows))])
    assert same.partner.tolist() == res.partner.tolist() and same.nstruct.tolist() == res.nstruct.tolist()


def test_the_counts_identities_and_the_derived_tensors():
    import torch
    rows = aligned_rows(21, 40, 130, gap_share=0.25)
    lines = [class_line(rows[0]), structure_line(4, 130, knots=True)]
    for canonical_only in (False, True):
        for min_loop in (0, 3, 200):
            res = project(sequences=rows, structures=np.array(lines), canonical_only=canonical_only, min_loop=min_loop)
            c = res.counts.long()
            assert (c[..., 0] == c[..., 1:10].sum(-1)).all()
            assert (c[..., 11] == c[..., 1:7].sum(-1) + (0 if canonical_only else 1) * c[..., 7] - c[..., 10]).all()
            assert (c[..., 11] == (res.partner >= 0).sum(-1) // 2).all()
            if min_loop == 200:
                assert not c[..., 11].any() and (res.partner == -1).all()
            kf = res.kept_fraction()
            assert kf.dtype == torch.float64 and tuple(kf.shape) == (40, 2)
            for r in range(40):
                for k in range(2):
                    den = int(c[r, k, 0] - c[r, k, 9])
                    assert kf[r, k].item() == (int(c[r, k, 11]) / den if den else 1.0)
            worst = res.worst_rows(k=1, n=7).tolist()
            assert worst == sorted(range(40), key=lambda r: (kf[r, 1].item(), r))[:7]
    assert (c[0, 0, 1:10] > 0).all() or (c[:, 0, 1:10].sum(0) > 0).all()       # every class occurs
    empty = project(sequences=["--", "AU"], structures="..")
    assert empty.kept_fraction().tolist() == [[1.0], [1.0]] and empty.length.tolist() == [0, 2] and empty.worst_rows(n=5).tolist() == [0, 1]


def test_support_and_contradicting_are_covariations_counts(folded):
    from squarna_amd import Covariation
    for step in (1, 2, 3):
        pairs = folded.pairs(step)
        assert pairs
        res = project(alignment=folded, step=step)
        assert res.K == 1 and res.shared and res.names == folded.names and res.sequences == folded.sequences
        with E.use_engine(OracleEngine()):
            cov = Covariation(alignment=folded, pairs=pairs)
        v = [p[0] for p in pairs]
        assert res.support().dtype.is_floating_point is False and tuple(res.support().shape) == (folded.L,)
        assert res.support()[v].tolist() == cov.bp_rows.tolist() and res.contradicting()[v].tolist() == cov.incompatible.tolist()
        others = sorted(set(range(folded.L)) - set(v))
        assert not res.support()[others].any() and not res.contradicting()[others].any()
    three = project(alignment=folded)
    assert three.K == 3 and three.shared
    for step in (1, 2, 3):
        assert three.support(step - 1).tolist() == project(alignment=folded, step=step).support().tolist()
    file_form = project(inputfile=ALI, structures=folded)
    assert file_form.partner.tolist() == three.partner.tolist() and file_form.names == three.names
    per_row = project(sequences=folded.sequences, structures=three.cpu().pos_of[:, None, :] * 0 - 1, strict=True)
    with pytest.raises(ValueError, match="shared"):
        per_row.support()


def test_every_input_form():
    import torch
    rows = ["GC-AUgc", "G.-A~gc", "ACGUNNN"]
    line = "((...))"
    p = partners_of(line)
    base = project(sequences=rows, structures=line)
    assert base.K == 1 and base.shared and base.dbn(0) == "((..))" and base.dbn(1) == "(..)" and base.dbn(2) == "((...))"
    assert project(sequences=rows, structures=line, canonical_only=True).dbn(2) == "......."
    assert CLASSES == ("none", "AU", "UA", "GC", "CG", "GU", "UG", "noncanonical", "one_gap", "both_gap") and base.CLASSES is CLASSES
    assert base.names == [">record1", ">record2", ">record3"] and base.cls[:, 0, :2].tolist() == [[3, 4], [3, 8], [7, 7]]
    forms = [[line], np.array(p), np.array([p]), torch.tensor(p), torch.tensor([p], dtype=torch.int16), np.array([p], np.int64),
             torch.tensor(p, dtype=torch.int64)]
    for form in forms:
        got = project(sequences=rows, structures=form)
        assert got.shared and got.partner.tolist() == base.partner.tolist() and got.counts.tolist() == base.counts.tolist()
    two = project(sequences=rows, structures=[line, "(.....)"])
    assert two.K == 2 and two.shared and two.partner[:, 0].tolist() == base.partner[:, 0].tolist()
    for form in ([[line, "(.....)"]] * 3, np.array([[p, partners_of("(.....)")]] * 3), torch.tensor([[p, partners_of("(.....)")]] * 3)):
        got = project(sequences=rows, structures=form)
        assert got.K == 2 and not got.shared and got.partner.tolist() == two.partner.tolist() and got.cls.tolist() == two.cls.tolist()
    host = base.cpu()
    assert host.partner.tolist() == base.partner.tolist()


def test_bad_arguments():
    import torch
    rows = ["GC-AUgc", "G.-A~gc"]
    for kw in (dict(), dict(sequences=rows, inputfile=ALI, structures="......."), dict(sequences=rows), dict(sequences=rows, structures="(.)"),
               dict(sequences=rows, structures=["(.....)", "(.)"]), dict(sequences=rows, structures=[["......."]]),
               dict(sequences=rows, structures=[["......."], [".......", "......."]]), dict(sequences=rows, structures=np.zeros((2, 3), np.int64)),
               dict(sequences=rows, structures=np.zeros((3, 1, 7), np.int64)), dict(sequences=rows, structures=np.zeros(7)),
               dict(sequences=rows, structures=np.zeros((0, 7), np.int32)), dict(sequences=rows, structures=".......", step=1),
               dict(sequences=rows, structures=".......", min_loop=-1), dict(sequences=rows, structures=".......", min_loop=1.5),
               dict(sequences=rows, structures=".......", canonical_only=2), dict(sequences=rows, structures=".......", names=["a"]),
               dict(sequences=rows, structures=7)):
        with pytest.raises(ValueError):
            project(**kw)
    for kw in (dict(sequences=rows), dict(sequences=rows, structures=[["(.)"], ["...."]]), dict(sequences=rows, structures=[["......"]]),
               dict(sequences=rows, structures=np.zeros((2, 1, 5), np.int32)), dict(sequences=rows, structures=np.zeros((2, 1, 6))),
               dict(sequences=rows, structures=np.full((2, 1, 6), -1), nstruct=[1, 2]), dict(sequences=rows, structures=[["......"], ["....."]], nstruct=[1, 1]),
               dict(sequences=rows, structures="......")):
        with pytest.raises(ValueError):
            lift(**kw)
    with pytest.raises(AssertionError):
        project(sequences=["GC", "G"], structures="..")


def test_invalid_lines_under_strict_and_not():
    rows = ["GC-AUgc", "G.-A~gc", "-------"]
    good = partners_of("((...))")
    bad = [[1, 0, 7, -1, -1, -1, -1], [0, -1, -1, -1, -1, -1, -1], [2, 2, 0, -1, -1, -1, -1], [-2, -1, -1, -1, -1, -1, -1]]
    for k, line in enumerate(bad):
        with pytest.raises(ValueError, match=r"row 0 \(>record1\), line 1"):
            project(sequences=rows, structures=np.array([good, line]))
    res = project(sequences=rows, structures=np.array([good] + bad), strict=False)
    assert res.status.tolist() == [[0, 1, 1, 1, 1]] * 3 and not res.counts[:, 1:].any() and not res.cls[:, 1:].any()
    assert (res.partner[:, 1:] == -1).all() and res.partner[0, 0].tolist() == [5, 4, -1, -1, 1, 0]
    per_row = project(sequences=rows, structures=np.array([[good], [bad[0]], [good]]), strict=False)
    assert per_row.status.tolist() == [[0], [1], [0]]
    # lifting: validity is in residue coordinates, against the row's length
    short = [[[5, 4, -1, -1, 1, 0]], [[3, -1, -1, 0]], [[]]]
    assert lift(sequences=rows, structures=padded(short)).status.tolist() == [[0], [0], [0]]
    short[1] = [[4, -1, -1, -1]]
    with pytest.raises(ValueError, match=r"row 1 \(>record2\), line 0"):
        lift(sequences=rows, structures=padded(short))
    res = lift(sequences=rows, structures=padded(short), strict=False)
    assert res.status.tolist() == [[0], [1], [0]] and (res.partner[1:] == -1).all() and res.partner[0, 0].tolist() == [6, 5, -1, -1, -1, 1, 0]


def test_score_and_distances_take_the_outputs(folded):
    from squarna_amd import Distances, Score
    res = project(alignment=folded)
    names, seqs = res.records()
    with E.use_engine(OracleEngine()):
        scored = Score(records=seqs, structures=res.to_padded())
        assert len(scored.status) == res.R * res.K and not scored.status.any()
        assert scored.npairs.view(res.R, res.K).tolist() == res.counts[..., 11].tolist()
        lifted = lift(alignment=folded, structures=res.partner)
        assert lifted.K == 3
        dist = Distances(lifted.to_padded(), groups="all")
    assert dist.S == res.R * 3 and not dist.status.any() and dist.npairs.view(res.R, 3).tolist() == res.counts[..., 11].tolist()
    # every lifted line is the step line minus the pairs the row opens
    for k in range(3):
        step = folded.steps[k].tolist()
        for r in range(res.R):
            kept = [(v, w) for v, w in pairs_of(step) if 1 <= int(res.cls[r, k, v]) <= 7]
            assert pairs_of(lifted.partner[r, k].tolist()) == kept
    freq = lifted.pair_frequency(0)
    expect = np.zeros((folded.L, folded.L))
    for r in range(res.R):
        for v, w in pairs_of(lifted.partner[r, 0].tolist()):
            expect[v, w] += 1
            expect[w, v] += 1
    assert freq.dtype.is_floating_point and freq.tolist() == (expect / res.R).tolist()


def test_lift_takes_a_fold_result():
    from squarna_amd import Fold
    rows = ["GGGA-AAUC-CC", "GGGAAAAUCCC-", "-G.GAAA~UCCC"]
    ungapped = ["".join(ch for ch in row if ch not in GAP_CHARS) for row in rows]
    with E.use_engine(OracleEngine()):
        folds = Fold(records=ungapped, configfile="nobpp")
    res = lift(sequences=rows, structures=folds)
    assert res.nstruct.tolist() == (1 + folds.nstruct).tolist() and res.K == int(res.nstruct.max())
    for r, row in enumerate(rows):
        lines = [folds.consensus(r)] + [folds.dbn(r, k) for k in range(int(folds.nstruct[r]))]
        for k, line in enumerate(lines):
            assert res.partner[r, k].tolist() == partners_of(D.ReAlign(line, row)), (r, k)
        assert (res.partner[r, len(lines):] == -1).all()
    with E.use_engine(OracleEngine()):
        other = Fold(records=ungapped[:2] + ["GGGAAAAUCC"], configfile="nobpp")
    with pytest.raises(ValueError, match="lengths"):
        lift(sequences=rows, structures=other)
