"""Checks shared by the CPU and GPU tests of FoldAlignment(): an AlignmentResult against the Step lines the reference printed
(tests/golden/text/*.txt), against a plain dict count over its rows, and against align.Consensus.  All comparisons are exact."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DATA = os.path.join(os.path.dirname(HERE), "squarna_amd", "data")

with open(os.path.join(GOLDEN, "digests.json")) as f:
    _DIGESTS = json.load(f)
with open(os.path.join(GOLDEN, "align_synth", "cases.json")) as f:
    _SYNTH = json.load(f)

#: golden tag -> (input file, FoldAlignment's keywords): the four alignment texts without verbose / entropy, the three synthetic ones
CASES = {}
for _tag in ("ali_input_a", "ali_input_a_s3i", "ali_input_a_s31", "demo_afa_a"):
    _kw = dict(_DIGESTS[_tag]["args"])
    _path = os.path.join(DATA, _kw.pop("inputfile"))
    assert _kw.pop("alignment") is True
    _kw.pop("reactformat", None)                                       # (only shapes the printed reactivity line)
    CASES[_tag] = (_path, _kw)
for _tag, _case in _SYNTH.items():
    _kw = dict(_case["args"])
    assert _kw.pop("alignment") is True
    CASES["ali_synth_" + _tag] = (os.path.join(GOLDEN, _case["inputfile"]), _kw)

SMALL = ["ali_input_a", "ali_input_a_s3i", "ali_input_a_s31", "demo_afa_a"]


def golden_steps(tag):
    """[(dbn, label, reactivity score text or None, metrics text or None)] of the three Step lines of a golden text."""
    with open(os.path.join(GOLDEN, "text", tag + ".txt")) as f:
        lines = f.read().rstrip("\n").split("\n")[-3:]
    out = []
    for k, line in enumerate(lines):
        fields = line.split("\t")
        assert fields[1].startswith("Step-%d" % (k + 1)), line
        rest = [x for x in fields[2:] if x]
        met = rest.pop() if rest and rest[-1].startswith("TP=") else None
        out.append((fields[0], fields[1], rest[0] if rest else None, met))
    return out


def check_against_golden(res, tag):
    """dbn(1..3), the metrics and the reactivity scores against the reference's Step lines."""
    steps = golden_steps(tag)
    for k, (dbn, label, react, met) in enumerate(steps):
        assert res.dbn(k + 1) == dbn, (tag, label)
        assert len(dbn) == res.L
        exp_pairs = _pairs(dbn)
        assert res.pairs(k + 1) == exp_pairs
        row = res.steps[k].tolist()
        assert [(v, w) for v, w in enumerate(row) if w > v] == exp_pairs and all(row[w] == v for v, w in exp_pairs)
        m = res.metrics[k].tolist()
        if met is not None:
            tp, fp, fn = int(m[0]), int(m[1]), int(m[2])
            assert [float(tp), float(fp), float(fn)] == m[:3]
            # (the reference prints the integer 1 where a ratio has no denominator, a rounded float elsewhere: Metrics :195-208)
            vals = [tp, fp, fn, m[3] if 2 * tp + fp + fn else 1, m[4] if tp + fp else 1, m[5] if tp + fn else 1]
            assert "TP={},FP={},FN={},FS={},PR={},RC={}".format(*vals) == met, (tag, label)
        elif "skipped" not in label:
            assert all(math.isnan(x) for x in m), (tag, label)
        if react is not None:
            assert str(round(float(res.react_scores[k]), 2)) == react, (tag, label)
        elif "skipped" not in label:
            assert float(res.react_scores[k]) == 0.5
    assert ("skipped" in steps[1][1]) == (res.rows is None)


def _pairs(dbn):
    from squarna_amd.dbn import DBNToPairs
    return DBNToPairs(dbn)


def dict_table(res):
    """Consensus' dict over the rows of res (SQRNdbnali.py:281-284), in its order: [(v, w, count, first row)]."""
    bps = {}
    rows = res.rows.cpu()
    for r in range(len(rows)):
        row = rows.partner[int(rows.cell_off[r]):int(rows.cell_off[r]) + len(rows.sequences[r])].tolist()
        for v, w in enumerate(row):
            if w > v:
                c, first = bps.get((v, w), (0, r))
                bps[(v, w)] = (c + 1, first)
    order = sorted(bps, key=lambda bp: bps[bp][0], reverse=True)       # (stable over the insertion order, as the reference's)
    return [(v, w, bps[(v, w)][0], bps[(v, w)][1]) for v, w in order]


def check_table(res):
    """The pair table against a plain dict count over rows; pair_frequency against it."""
    exp = dict_table(res)
    got = [(v, w, c, f) for (v, w), c, f in zip(res.pair_cols.tolist(), res.pair_count.tolist(), res.pair_first.tolist())]
    assert got == exp
    freq = res.pair_frequency()
    assert freq.device == res.steps.device and tuple(freq.shape) == (res.L, res.L)
    dense = np.zeros((res.L, res.L))
    for v, w, c, _ in exp:
        dense[v, w] = dense[w, v] = c / len(res)
    assert freq.cpu().numpy().tobytes() == dense.tobytes()


def check_consensus_at(res):
    """consensus_at(x) against align.Consensus on the rows' consensus lines, its per-pair path and its bulk path."""
    from squarna_amd import align
    structs = [res.rows.consensus(r) for r in range(len(res))]
    for k in range(21):
        x = k / 20
        exp = align.Consensus(structs, x)
        assert res.consensus_at(x) == exp, x
        if len(structs) * len(structs[0]) >= 4096:
            assert align._consensus_bulk(structs, x) == exp
    from squarna_amd.dbn import DBNToPairs, PairsToDBN
    step2 = PairsToDBN(DBNToPairs(align.Consensus(structs, res.freqlimit)), res.L, levellimit=res.levellimit)
    assert res.consensus_at(res.freqlimit, levellimit=res.levellimit) == step2 == res.dbn(2)


def check_equal(a, b):
    """Two AlignmentResults, tensor by tensor (b on the CPU)."""
    assert a.names == b.names and a.sequences == b.sequences and a.L == b.L
    for key in ("steps", "pair_cols", "pair_count", "pair_first"):
        assert getattr(a, key).cpu().tolist() == getattr(b, key).tolist(), key
    for key in ("stem_matrix", "metrics", "react_scores"):
        assert getattr(a, key).cpu().numpy().tobytes() == getattr(b, key).numpy().tobytes(), key
    assert (a.rows is None) == (b.rows is None)
    if a.rows is not None:
        for key in ("lengths", "nstruct", "row_off", "cell_off", "partner", "pset_mask"):
            assert getattr(a.rows, key).cpu().tolist() == getattr(b.rows, key).tolist(), key
        assert a.rows.scores.cpu().numpy().tobytes() == b.rows.scores.numpy().tobytes()
        assert np.array_equal(a.rows.metrics.cpu().numpy(), b.rows.metrics.numpy(), equal_nan=True)
