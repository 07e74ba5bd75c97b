"""CPU tests of FoldWindows() / WindowResult (no GPU): the windowed mode's host path under the test-only OracleEngine against
the plain-Python restatement of tests/fold_windows_checks.py.  All comparisons are exact."""
import random

import pytest

from squarna_amd import engine as E
from tests.fold_windows_checks import (LIMITS, REAL, by_cell_only, check_equal, check_result, check_views, cover_enum, cover_sorted,
                                       first_fit, random_seq, starts_of)
from tests.oracle_engine import OracleEngine


def windows(**kw):
    from squarna_amd import FoldWindows
    with E.use_engine(OracleEngine()):
        return FoldWindows(**kw)


def fold(**kw):
    from squarna_amd import Fold
    with E.use_engine(OracleEngine()):
        return Fold(**kw)


@pytest.mark.parametrize("shape,expected", [((50, 60, 7), [0]), ((60, 60, 7), [0]), ((61, 60, 7), [0, 1]), ((100, 60, 60), [0, 40]),
                                            ((120, 60, 60), [0, 60]), ((400, 60, 7), list(range(0, 337, 7)) + [340])])
def test_starts_rule(shape, expected):
    from squarna_amd.fold_windows import window_starts
    assert window_starts(*shape) == expected == starts_of(*shape)
    assert len(window_starts(400, 60, 7)) == 50


def test_the_two_coverage_forms_agree():
    rng = random.Random(3)
    for _ in range(200):
        N, window = rng.randint(1, 150), rng.randint(2, 50)
        step = rng.randint(1, window)
        s, wlen = starts_of(N, window, step), min(window, N)
        for _ in range(20):
            i = rng.randrange(N)
            j = rng.randint(i, min(N - 1, i + wlen - 1))
            assert cover_enum(i, j, s, wlen) == cover_sorted(i, j, s, wlen)


@pytest.fixture(scope="module", params=sorted(REAL))
def real(request):
    seq, window, step, conf = REAL[request.param]
    res = windows(inputseq=seq, window=window, step=step, configfile=conf)
    return request.param, res, check_result(res)


def test_real_folds_windows_are_fold_of_the_window_records(real):
    tag, res, _ = real
    seq, window, step, conf = REAL[tag]
    assert res.source == "host" and res.device.type == "cpu" and res.first_fit_rounds == ()
    assert res.names == [">inputseq"] and res.sequences == [seq] and (res.window, res.step, res.freqlimit) == (window, step, 0.35)
    recs = [(">inputseq/%d-%d" % (a + 1, a + window), seq[a:a + window], None, None, None) for a in starts_of(len(seq), window, step)]
    exp = fold(records=recs, configfile=conf)
    import torch
    w = res.windows
    assert w.names == exp.names and w.sequences == exp.sequences and w.paramset_names == exp.paramset_names
    for key in ("partner", "pset_mask", "row_off", "cell_off", "nstruct", "lengths"):
        assert getattr(w, key).tolist() == getattr(exp, key).tolist(), key
    for key in ("scores", "metrics"):
        assert getattr(w, key).view(torch.int64).tolist() == getattr(exp, key).view(torch.int64).tolist(), key


def test_real_folds_table_and_views(real):
    tag, res, tables = real
    table, = tables
    assert len(table) == {"400_greedynobpp": 357, "333_nobpp": 254}[tag]
    assert max(e[2] for e in table) == {"400_greedynobpp": 6, "333_nobpp": 7}[tag] >= 3
    assert any(e[2] >= 3 for e in table)
    check_views(res, tables)


def test_real_folds_the_tie_order_matters(real):
    """Ranking ties by (i, j) alone gives another consensus: the order by count and first holder is what these inputs test."""
    tag, res, (table,) = real
    N = len(res.sequences[0])
    differs = [lim for lim in (0, 0.35, 0.5) if first_fit(table, lim, N) != first_fit(table, lim, N, key=by_cell_only)]
    assert differs == [0, 0.35, 0.5]


def test_three_records_reactivities_and_reference():
    from squarna_amd import align
    rng = random.Random(9)
    seqs = [random_seq(1, 400), random_seq(4, 50), random_seq(5, 61)]
    reacts = [round(rng.random(), 3) for _ in range(400)]
    ref = "((((((......))))))" + "." * 32
    recs = [("long", seqs[0], reacts, None, None), ("short", seqs[1], None, "." * 50, ref), ("edge", seqs[2], None, None, None)]
    res = windows(records=recs, window=60, step=7, configfile="greedynobpp", freqlimit=0.2)
    assert res.win_off.tolist() == [0, 50, 51, 53] and res.pos_off.tolist() == [0, 400, 450, 511]
    assert res.starts.tolist() == starts_of(400, 60, 7) + [0] + [0, 1] and res.freqlimit == 0.2
    tables = check_result(res, [None, ref, None])
    assert len(tables[0]) > 0
    check_views(res, tables, limits=(0.2, 1))
    wrecs = [("long/%d-%d" % (a + 1, a + 60), seqs[0][a:a + 60], reacts[a:a + 60], None, None) for a in starts_of(400, 60, 7)]
    wrecs += [("short/1-50", seqs[1], None, None, None), ("edge/1-60", seqs[2][:60], None, None, None), ("edge/2-61", seqs[2][1:], None, None, None)]
    exp = fold(records=wrecs, configfile="greedynobpp")
    import torch
    assert res.windows.names == exp.names and res.windows.partner.tolist() == exp.partner.tolist()
    assert res.windows.scores.view(torch.int64).tolist() == exp.scores.view(torch.int64).tolist()
    assert (exp.scores[:int(exp.row_off[50]), 2] != 0).any()                 # (the sliced reactivities reach the windows' scores)
    plain = fold(records=[(n, s, None, None, None) for n, s, _, _, _ in wrecs[:50]], configfile="greedynobpp")
    assert plain.scores.tolist() != exp.scores[:int(exp.row_off[50])].tolist()
    # the reference line is used for the metrics only: never handed to a window
    assert res.windows.metrics.isnan().all()
    line = res.dbn(1)
    assert [float(x) for x in align.Metrics(ref, line)] == res.metrics[1].tolist() and res.metrics[0].isnan().all()


def test_one_call_equals_separate_calls():
    """Records are independent: the blocks of a three-record call are the single-record results."""
    seqs = [random_seq(7, 90), random_seq(8, 20), random_seq(9, 75)]
    res = windows(records=seqs, window=40, step=9, configfile="greedynobpp")
    tables = check_result(res)
    for r, seq in enumerate(seqs):
        one = windows(records=[(res.names[r], seq, None, None, None)], window=40, step=9, configfile="greedynobpp")
        assert check_result(one) == [tables[r]]
        lo, hi = res.pos_off.tolist()[r:r + 2]
        assert one.consensus.tolist() == res.consensus.tolist()[lo:hi]
    check_equal(res, windows(records=seqs, window=40, step=9, c="greedynobpp"))


def test_prints_nothing(capsys):
    windows(inputseq=random_seq(3, 50), window=30, configfile="greedynobpp")
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""


def test_default_step_and_synonyms():
    seq = random_seq(11, 47)
    res = windows(s=seq, window=22, c="greedynobpp")
    assert res.step == 4 and res.starts.tolist() == starts_of(47, 22, 4)
    assert windows(inputseq="ACGUACGUAC", window=3, configfile="greedynobpp").step == 1


@pytest.mark.parametrize("kw", [dict(window=1), dict(window=2.5), dict(window="x"), dict(step=0), dict(step=61), dict(step=1.5),
                                dict(freqlimit=-0.1), dict(freqlimit=1.5), dict(freqlimit="x"),
                                dict(records=["ACGU-ACGU"]), dict(records=["ACGUACGU&ACGUACGU"]), dict(records=["ACGU.ACGU"]),
                                dict(records=[("n", "ACGUACGUAC", None, "(........)", None)]),
                                dict(bpp=[None]), dict(entropy=True), dict(alignment=True), dict(rfam=True)])
def test_value_errors(kw):
    args = dict(records=["ACGUACGUACGUACGU"], window=60, configfile="greedynobpp")
    args.update(kw)
    with pytest.raises(ValueError) as err:
        windows(**args)
    if set(kw) & {"entropy", "alignment", "rfam"}:
        assert "Fold does not cover" in str(err.value)


def test_total_length_bound():
    """The positions of all records together stay below 2^31 (checked before anything is cut or folded)."""
    class Long(str):
        def __len__(self):
            return 2 ** 30
    with pytest.raises(ValueError, match="2\\^31"):
        windows(records=[(">a", Long("ACGU"), None, None, None), (">b", Long("ACGU"), None, None, None)], window=60)
