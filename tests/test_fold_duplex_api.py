"""CPU tests of FoldDuplex() / DuplexResult (no GPU): the interaction screen's host path under the test-only OracleEngine
against the plain-Python restatement of tests/fold_duplex_checks.py.  All comparisons are exact."""
import os
import random

import pytest

from squarna_amd import engine as E
from tests.fold_duplex_checks import check_equal, check_result, random_seq, revcomp
from tests.oracle_engine import OracleEngine

CONF = "greedynobpp"
T0 = "GGGGCUAAAAGCCCCAAAAAAUCAGGUCAUCG"
TARGETS = [T0, random_seq(71, 64), random_seq(72, 90)]
QUERIES = [revcomp(T0[2:14]), revcomp(TARGETS[1][20:34]), random_seq(73, 20), "A" * 10]
ALL_PAIRS = [(a, b) for a in range(3) for b in range(4)]


def duplex(**kw):
    from squarna_amd import FoldDuplex
    with E.use_engine(OracleEngine()):
        return FoldDuplex(**kw)


def fold(**kw):
    from squarna_amd import Fold
    with E.use_engine(OracleEngine()):
        return Fold(**kw)


@pytest.fixture(scope="module")
def screen():
    res = duplex(targets=TARGETS, queries=QUERIES, configfile=CONF)
    return res, check_result(res, TARGETS, QUERIES, ALL_PAIRS)


def test_screen_numbers(screen):
    from squarna_amd.fold_duplex import COLUMNS
    res, (solo_rows, dup_rows, summary) = screen
    assert COLUMNS == ("inter", "intra_a", "intra_b", "lost_a", "lost_b", "a_first", "a_last", "b_first", "b_last")
    assert res.source == "host" and res.device.type == "cpu" and len(res) == 12 and not res.self_screen
    assert res.target_names == [">record1", ">record2", ">record3"] and res.query_names == [">record%d" % k for k in range(1, 5)]
    assert res.folds.names[5] == ">record2&>record2"
    k = res.index(0, 0)
    assert k == 0 and summary[k][:4] == [12, 0, 0, 6] and res.site(k) == ((2, 13), (0, 11))
    assert res.solo_dbn(0) == "((((((...))))))................." and res.dbn(0) == "..((((((((((((..................&))))))))))))"
    assert int(res.disruption(0)) == summary[0][3] + summary[0][4] > 6
    for a in range(3):                                                      # a poly-A query binds nothing and opens nothing
        assert summary[res.index(a, 3)][0] == 0 and summary[res.index(a, 3)][3] == 0
        assert res.dbn(res.index(a, 3)).split("&") == [res.solo_dbn(a), "." * 10]
    assert summary[res.index(0, 0)][0] > 0 and summary[res.index(1, 1)][0] > 0          # the reverse complements bind
    assert "[" in res.dbn(res.index(1, 2)) and "]" in res.dbn(res.index(1, 2))          # a pseudoknotted duplex
    assert res.bound_of(0).tolist()[2:14] == [1] * 12 and int(res.bound.sum()) == 2 * sum(s[0] for s in summary)
    assert res.best_partners(0, 1).tolist() == [0] and res.to_matrix(0)[0, 0] == 12


def test_duplexes_are_fold_of_the_two_chain_sequences(screen):
    res, _ = screen
    for k, (a, b) in enumerate(ALL_PAIRS):
        assert res.dbn(k) == fold(inputseq=TARGETS[a] + "&" + QUERIES[b], configfile=CONF).consensus(0), k
    for r, seq in enumerate(TARGETS + QUERIES):
        assert res.solo_dbn(r) == fold(inputseq=seq, configfile=CONF).consensus(0)


def test_interchainonly_reaches_the_duplexes_only(screen):
    plain, _ = screen
    res = duplex(targets=TARGETS, queries=QUERIES, configfile=CONF, ico=True)
    _, _, summary = check_result(res, TARGETS, QUERIES, ALL_PAIRS)
    assert all(s[1] == 0 and s[2] == 0 for s in summary) and any(s[0] > 0 for s in summary)
    assert [res.solo_dbn(r) for r in range(7)] == [plain.solo_dbn(r) for r in range(7)] and "(" in res.solo_dbn(0)
    check_equal(res, duplex(targets=TARGETS, queries=QUERIES, c=CONF, interchainonly=True))


def test_targets_against_themselves():
    res = duplex(targets=TARGETS, configfile=CONF)
    check_result(res, TARGETS, None, [(0, 1), (0, 2), (1, 2)])
    assert res.self_screen and res.query_names == [] and res.to_matrix().tolist()[1] == [-1, -1, int(res.summary[2, 0])]
    res = duplex(targets=TARGETS, homodimers=True, configfile=CONF)
    _, _, summary = check_result(res, TARGETS, None, [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)])
    for k in (0, 3, 5):                                                     # both copies of a homodimer see the same
        assert summary[k][1] == summary[k][2] and summary[k][3] == summary[k][4] and summary[k][5:7] == summary[k][7:9]
    assert res.bound_of(1).tolist()[19:60].count(0) < 41
    one = duplex(targets=TARGETS[:1], configfile=CONF)                      # a single target: no pair, no duplex call
    check_result(one, TARGETS[:1], None, [])
    assert one.folds is None and len(one) == 0 and one.to_matrix().tolist() == [[-1]] and one.best_partners(0).tolist() == []
    check_equal(one, one.cpu())


def test_explicit_pairs_with_a_repeat():
    pairs = [(2, 1), (0, 3), (2, 1), (1, 1)]
    res = duplex(targets=TARGETS, queries=QUERIES, pairs=pairs, configfile=CONF)
    _, _, summary = check_result(res, TARGETS, QUERIES, pairs)
    assert res.index(2, 1) == 0 and summary[0] == summary[2] and summary[0][0] > 0 and res.bound_of(2).max() == 2
    with pytest.raises(ValueError):
        res.to_matrix()
    own = duplex(targets=TARGETS, pairs=[(2, 1), (1, 1)], configfile=CONF)  # (both indices into the targets)
    check_result(own, TARGETS, None, [(2, 1), (1, 1)])
    assert own.best_partners(1).tolist() == sorted([1, 2], key=lambda b: (-int(own.summary[own.index(b, 1), 0]), b))


def test_reactivities_and_restraints_on_one_side():
    rng = random.Random(4)
    reacts = [round(rng.random(), 3) for _ in range(len(T0))]
    rests = "______" + "." * (len(T0) - 6)
    probed = ("probed", T0, reacts, rests, "((((((...)))))).................")
    res = duplex(targets=[probed], queries=[("q", QUERIES[0], None, None, None), QUERIES[3]], configfile=CONF)
    from squarna_amd.fold_duplex import _duplex_record
    rec = _duplex_record(probed, ("q", QUERIES[0], None, None, None))
    assert rec == ("probed&q", T0 + "&" + QUERIES[0], reacts + [0.5] * 13, rests + "." * 13, None)
    assert _duplex_record(("q", "ACG", None, None, None), ("p", "GU", [0.1, 0.2], "._", "..")) == ("q&p", "ACG&GU", [0.5] * 4 + [0.1, 0.2], "....._", None)
    assert _duplex_record(("q", "ACG", None, None, None), ("p", "GU", None, None, None))[2:] == (None, None, None)
    assert res.folds.names == ["probed&q", "probed&>record2"] and res.target_names == ["probed"] and res.query_names == ["q", ">record2"]
    assert not res.solos.metrics[0].isnan().all() and res.folds.metrics.isnan().all()
    for k, q in enumerate((QUERIES[0], QUERIES[3])):
        by_hand = ("d", T0 + "&" + q, reacts + [0.5] * (1 + len(q)), rests + "." * (1 + len(q)), None)
        assert res.dbn(k) == fold(records=[by_hand], configfile=CONF).consensus(0)
        assert res.dbn(k)[:6] == "......"                                   # (the restraint line reaches the duplexes)
    assert res.solo_dbn(0)[:6] == "......" and res.summary[0, 0] > 0


def test_files(tmp_path):
    tf, qf = tmp_path / "targets.fas", tmp_path / "queries.fas"
    tf.write_text("".join(">t%d\n%s\n" % (k, s) for k, s in enumerate(TARGETS[:2])))
    qf.write_text("".join(">q%d\n%s\n" % (k, s) for k, s in enumerate(QUERIES[:2])))
    res = duplex(targetfile=str(tf), queryfile=str(qf), inputformat="q", configfile=CONF)
    check_result(res, TARGETS[:2], QUERIES[:2], [(0, 0), (0, 1), (1, 0), (1, 1)])
    assert res.folds.names[1] == ">t0&>q1"
    mixed = duplex(targetfile=str(tf), queries=QUERIES[:2], inputformat="q", configfile=CONF)
    assert mixed.summary.tolist() == res.summary.tolist() and mixed.bound.tolist() == res.bound.tolist()
    with pytest.raises(ValueError, match="targets and targetfile"):
        duplex(targets=TARGETS, targetfile=str(tf), configfile=CONF)
    with pytest.raises(ValueError, match="queries and queryfile"):
        duplex(targets=TARGETS, queries=QUERIES, queryfile=str(qf), configfile=CONF)
    with pytest.raises(AssertionError, match="Input file does not exist"):
        duplex(targetfile=os.path.join(str(tmp_path), "missing.fas"), configfile=CONF)


@pytest.mark.parametrize("kw", [dict(targets=["ACGU-ACGUACGU"]), dict(targets=["ACGUACGU&ACGU"]), dict(queries=["ACGU.ACGU"]),
                                dict(queries=["ACGU;ACGU"]), dict(queries=[("q", "ACGU", "0.1 0.2 0.3 0.4", None, None)]),
                                dict(targets=[("t", "ACGUACGUACGU", "1" * 12, None, None)]),
                                dict(pairs=[(1, 0)]), dict(pairs=[(0, 1)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, 0, 0)]), dict(pairs=[(0.0, 0)]),
                                dict(pairs=[(True, 0)]), dict(pairs=[0]), dict(pairs=7), dict(queries=None, pairs=[(0, 1)]),
                                dict(bpp=[None]), dict(records=["ACGU"]), dict(inputseq="ACGU"), dict(s="ACGU"), dict(inputfile="x.fas"),
                                dict(entropy=True), dict(alignment=True)])
def test_value_errors(kw):
    args = dict(targets=["ACGUACGUACGUACGU"], queries=["ACGUACGU"], configfile=CONF)
    args.update(kw)
    with pytest.raises(ValueError) as err:
        duplex(**args)
    if "bpp" in kw:
        assert str(err.value) == "FoldDuplex does not cover bpp: use Fold"
    if set(kw) & {"entropy", "alignment"}:
        assert "Fold does not cover" in str(err.value)
    if kw.get("targets") and isinstance(kw["targets"][0], str):
        assert ">record1" in str(err.value) and "targets" in str(err.value)     # (the record is named)
    if kw.get("queries") and isinstance(kw["queries"][0], str):
        assert ">record1" in str(err.value) and "queries" in str(err.value)


def test_cpu_round_trip(screen):
    res, _ = screen
    host = res.cpu()
    assert host is not res and host.source == res.source and host.device.type == "cpu" and host.folds.partner.device.type == "cpu"
    check_equal(host, res)
    check_result(host, TARGETS, QUERIES, ALL_PAIRS)


def test_best_partners_tie_order(screen):
    res, (_, _, summary) = screen
    for a in range(3):                                                      # the poly-A query and another without a pair tie at 0
        inter = [summary[res.index(a, b)][0] for b in range(4)]
        assert res.best_partners(a, 4).tolist() == sorted(range(4), key=lambda b: (-inter[b], b))
    assert any(len({summary[res.index(a, b)][0] for b in range(4)}) < 4 for a in range(3))


def test_score_gain_without_a_structure():
    """A duplex or a chain without any structure has no score: NaN, not an index error."""
    res = duplex(targets=["AAAAAAAAAA", T0], queries=["AAAAAAAA", QUERIES[0]], configfile=CONF)
    check_result(res, ["AAAAAAAAAA", T0], ["AAAAAAAA", QUERIES[0]], [(0, 0), (0, 1), (1, 0), (1, 1)])
    gain = res.score_gain()
    have = [int(res.solos.nstruct[r]) > 0 for r in range(4)]
    assert gain.isnan().tolist() == [not (int(res.folds.nstruct[k]) > 0 and have[a] and have[2 + b])
                                     for k, (a, b) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)])]
    assert not gain[3].isnan() and float(gain[3]) > 0


def test_prints_nothing(capsys):
    duplex(targets=[T0], queries=[QUERIES[0]], configfile=CONF)
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""
