"""CPU tests of FoldMutants() / MutantResult (no GPU): the mutational scan's host path under the test-only OracleEngine against
the plain-Python restatement of tests/fold_mutants_checks.py.  All comparisons are exact."""
import random

import pytest

from squarna_amd import engine as E
from tests.fold_mutants_checks import LETTERS, check_equal, check_result, consensus_rows, norm, pair_set, random_seq, substitute
from tests.oracle_engine import OracleEngine

CONF = "greedynobpp"
ODD = "GGGaAGcTNCC-CUUCG&GGCtAAGCCC"                                       # a lower-case letter, a T, an N, a gap, a separator


def mutants(**kw):
    from squarna_amd import FoldMutants
    with E.use_engine(OracleEngine()):
        return FoldMutants(**kw)


def fold(**kw):
    from squarna_amd import Fold
    with E.use_engine(OracleEngine()):
        return Fold(**kw)


def _three_records():
    rng = random.Random(4)
    reacts = [round(rng.random(), 3) for _ in range(30)]
    rests = "__" + "." * 28
    ref = "((((......))))" + "." * 16
    return [("plain", random_seq(21, 40), None, None, None), ("probed", random_seq(22, 30), reacts, rests, ref), ("odd", ODD, None, None, None)]


@pytest.fixture(scope="module")
def scan():
    recs = _three_records()
    res = mutants(records=recs, configfile=CONF)
    return recs, res, check_result(res)


def test_scan_counts_names_and_sequences(scan):
    recs, res, (wanted, _) = scan
    assert res.source == "host" and res.mode == "scan" and res.device.type == "cpu" and len(res) == 3
    assert res.names == ["plain", "probed", "odd"] and res.sequences == [r[1] for r in recs]
    plain = sum(ch in "ACGUacgutT" for ch in ODD)
    assert plain == len(ODD) - 3 and res.var_off.tolist() == [0, 120, 210, 210 + 3 * plain]
    per_pos = [0] * len(ODD)
    for k in range(3 * plain):
        name, ((p, old, new),) = res.variant(2, k)
        per_pos[p] += 1
        assert old == ODD[p] and new in LETTERS and new != norm(old) and name == "odd/%s%d%s" % (old.upper(), p + 1, new)
        assert res.folds.sequences[3 + 210 + k] == ODD[:p] + new + ODD[p + 1:]
    assert per_pos == [3 if ch in "ACGUacgutT" else 0 for ch in ODD]
    assert [res.variant(2, k)[0] for k in (9, 10, 11, 21)] == ["odd/A4C", "odd/A4G", "odd/A4U", "odd/T8A"]
    assert res.variant(0, 0)[0] == "plain/%s1%s" % (recs[0][1][0], [c for c in LETTERS if c != recs[0][1][0]][0])
    # the variants carry the wild type's reactivities and restraints, never its reference
    assert res.folds.metrics[3:].isnan().all() and not res.folds.metrics[1].isnan().all()


def test_scan_variants_are_fold_of_the_variant_records(scan):
    recs, res, (wanted, _) = scan
    for r, k in ((0, 0), (0, 77), (1, 5), (1, 89), (2, 30)):
        seq = substitute(recs[r][1], wanted[r][k])
        name, reacts, rests = recs[r][0], recs[r][2], recs[r][3]
        if reacts is None:
            exp = fold(inputseq=seq, configfile=CONF)
        else:
            exp = fold(records=[(name, seq, reacts, rests, None)], configfile=CONF)
        assert res.dbn(r, k) == exp.consensus(0), (r, k)
    assert res.dbn(1) == fold(records=[recs[1]], configfile=CONF).consensus(0)
    assert all(res.dbn(1, k)[:2] == ".." for k in range(90))              # (the restraint line reaches the variants)


def test_scan_some_variant_changes_the_structure(scan):
    _, res, (_, per_rec) = scan
    assert all(any(d[3] > 0 for d in mine) for mine in per_rec) and any(d[3] == 0 for mine in per_rec for d in mine)
    assert int(res.pos_changed.sum()) == sum(d[3] for mine in per_rec for d in mine)


def test_positions():
    seqs = [random_seq(31, 40), random_seq(32, 40)]
    res = mutants(records=seqs, positions=[0, 5, 5, 39], configfile=CONF)
    check_result(res, positions=[0, 5, 5, 39])
    assert res.site_pos.tolist() == [0] * 3 + [5] * 3 + [39] * 3 + [0] * 3 + [5] * 3 + [39] * 3 and res.var_off.tolist() == [0, 9, 18]
    matrix = res.to_matrix(0).tolist()
    assert all((min(row) == -1 and sorted(row)[1] >= 0) == (p in (0, 5, 39)) and (max(row) == -1) == (p not in (0, 5, 39))
               for p, row in enumerate(matrix))
    assert res.profile(0)[1].isnan().all() and not res.profile(0)[5].isnan().any()
    check_equal(res, mutants(records=seqs, positions=(39, 0, 5), c=CONF))
    for bad in ([40], [0, -1], [1.0], ["1"], [True]):
        with pytest.raises(ValueError):
            mutants(records=seqs, positions=bad, configfile=CONF)
    with pytest.raises(ValueError):                                        # (the shortest record decides)
        mutants(records=seqs + ["ACGUACGU"], positions=[8], configfile=CONF)


def test_explicit_variants():
    seq = random_seq(41, 40)
    wild = fold(inputseq=seq, configfile=CONF)
    npairs = len(pair_set(consensus_rows(wild)[0]))
    assert npairs > 0
    own = seq[7].lower() if seq[7] != "U" else "t"
    variants = [[[(3, "a" if seq[3] != "A" else "c"), (30, "T" if seq[30] != "U" else "G")], [(12, LETTERS[(LETTERS.index(seq[12]) + 1) % 4])], [(7, own)]]]
    res = mutants(records=[("wt", seq, None, None, None)], variants=variants, configfile=CONF)
    check_result(res, variants=variants)
    assert res.mode == "explicit" and res.site_off.tolist() == [0, 2, 3, 4] and res.var_off.tolist() == [0, 3]
    assert res.folds.names[1] == "wt/%s4%s+%s31%s" % (seq[3], norm(variants[0][0][0][1]), seq[30], norm(variants[0][0][1][1]))
    assert res.folds.sequences[3] == seq and res.diff[2].tolist() == [0, 0, npairs, 0, -1, -1]
    assert res.dbn(0, 2) == res.dbn(0) == wild.consensus(0)
    with pytest.raises(ValueError):
        res.to_matrix(0)
    with pytest.raises(ValueError):
        res.profile(0)


@pytest.mark.parametrize("kw", [dict(positions=[1], variants=[[[(1, "A")]]]), dict(records=["ACGU-ACGUACGU"], variants=[[[(4, "A")]]]),
                                dict(records=["ACGUACGU&ACGU"], variants=[[[(8, "A")]]]), dict(variants=[[[(1, "A"), (1, "C")]]]),
                                dict(variants=[[[(16, "A")]]]), dict(variants=[[[(-1, "A")]]]), dict(variants=[[[(1, "N")]]]),
                                dict(variants=[[[]]]), dict(variants=[[[(1, "A")]], [[(1, "A")]]]), dict(variants=[[[(1.5, "A")]]]),
                                dict(bpp=[None]), dict(entropy=True), dict(alignment=True)])
def test_value_errors(kw):
    args = dict(records=["ACGUACGUACGUACGU"], configfile=CONF)
    args.update(kw)
    with pytest.raises(ValueError) as err:
        mutants(**args)
    if "bpp" in kw:
        assert str(err.value) == "FoldMutants does not cover bpp: use Fold"
    if set(kw) & {"entropy", "alignment"}:
        assert "Fold does not cover" in str(err.value)


def test_cpu_round_trip_and_synonyms(scan):
    _, res, _ = scan
    host = res.cpu()
    assert host is not res and host.source == res.source and host.device.type == "cpu" and host.folds.partner.device.type == "cpu"
    check_equal(host, res)
    check_result(host)
    seq = random_seq(51, 24)
    a = mutants(s=seq, c=CONF)
    assert a.names == [">inputseq"] and a.var_off.tolist() == [0, 72]
    check_equal(a, mutants(inputseq=seq, configfile=CONF))


def test_to_matrix_and_profile(scan):
    """Against the helpers in check_result already; here the shape of the odd record: -1 rows where nothing is substituted."""
    _, res, (_, per_rec) = scan
    matrix, prof = res.to_matrix(2).tolist(), res.profile(2).tolist()
    for p, ch in enumerate(ODD):
        if ch in "N-&":
            assert matrix[p] == [-1] * 4 and prof[p][0] != prof[p][0] and prof[p][1] != prof[p][1]
        else:
            assert matrix[p][LETTERS.index(norm(ch))] == -1 and sorted(matrix[p])[1] >= 0
            have = [d for d in matrix[p] if d >= 0]
            assert prof[p] == [sum(have) / 3, float(max(have))]
    assert sum(d >= 0 for row in matrix for d in row) == len(per_rec[2])


def test_most_disruptive_tie_order(scan):
    _, res, (_, per_rec) = scan
    for r, mine in enumerate(per_rec):
        dist = [d[0] + d[1] for d in mine]
        top = res.most_disruptive(r, len(mine)).tolist()
        assert top == sorted(range(len(mine)), key=lambda k: (-dist[k], k))
        ties = [(a, b) for a, b in zip(top, top[1:]) if dist[a] == dist[b]]
        assert ties and all(a < b for a, b in ties)
    assert res.most_disruptive(0).tolist() == res.most_disruptive(0, 120).tolist()[:10]


def test_no_substitutable_position():
    res = mutants(records=["NNNN-NNNN", "ACGUACGUAC"], positions=[0, 1], configfile=CONF)
    check_result(res, positions=[0, 1])
    assert res.var_off.tolist() == [0, 0, 6] and res.pos_changed[:9].tolist() == [0] * 9 and res.distance(0).numel() == 0


def test_prints_nothing(capsys):
    mutants(inputseq=random_seq(3, 20), positions=[2, 3], configfile=CONF)
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""
