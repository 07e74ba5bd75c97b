"""Checks shared by the CPU and GPU tests of Score() (tests/test_score_api.py, tests/test_hip_score.py): the golden cases of
tests/golden/score.json in the three forms Score takes structures in, and the exact comparison of a ScoreResult with the
values the reference returned.  Not a test module."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN6 = [float("nan")] * 6
_cases = None

#: (name, sequence, partner row) of every kind of invalid row
INVALID = [
    ("partner_out_of_range", "GGGAAACCC", [9, -1, -1, -1, -1, -1, -1, -1, -1]),
    ("partner_below_minus_one", "GGGAAACCC", [-2, -1, -1, -1, -1, -1, -1, -1, -1]),
    ("not_symmetric", "GGGAAACCC", [8, -1, -1, -1, -1, -1, -1, -1, -1]),
    ("two_claim_one", "GGGAAACCC", [8, 8, -1, -1, -1, -1, -1, -1, 0]),
    ("pairs_with_itself", "GGGAAACCC", [-1, -1, -1, 3, -1, -1, -1, -1, -1]),
    ("pair_on_separator", "GGG&AACCC", [8, -1, -1, 5, -1, 3, -1, -1, 0]),
    ("nothing_to_score", "-&-", [-1, -1, -1]),
]


def cases():
    """The golden cases, read once and left unchanged."""
    global _cases
    if _cases is None:
        with open(os.path.join(GOLDEN, "score.json")) as f:
            _cases = json.load(f)
    return _cases


def records_of(cs):
    return [(">" + c["name"], c["seq"], c["reacts"], None, c["known"]) for c in cs]


def partner_row(dbn, width=None):
    """The partner array of a dot-bracket line (input columns), -1 padded to `width`."""
    from squarna_amd.dbn import DBNToPairs
    row = np.full(len(dbn) if width is None else width, -1, np.int32)
    for v, w in DBNToPairs(dbn):
        row[v], row[w] = w, v
    return row


def strings_form(cs):
    return [[r["dbn"] for r in c["rows"]] for c in cs]


def padded_form(cs, extra=0):
    """(int32[R, K, Lmax] numpy array, nstruct) of the cases' structures; extra: unused columns behind the longest record."""
    K = max(len(c["rows"]) for c in cs)
    Lmax = max(len(c["seq"]) for c in cs) + extra
    out = np.full((len(cs), K, Lmax), -1, np.int32)
    for r, c in enumerate(cs):
        for k, row in enumerate(c["rows"]):
            out[r, k] = partner_row(row["dbn"], Lmax)
    return out, np.array([len(c["rows"]) for c in cs], np.int64)


def fold_result_form(cs, device=None):
    """A FoldResult whose rows are the cases' structures: the first one in the consensus' place, the others behind it."""
    import torch
    from squarna_amd.fold import FoldResult, _offsets
    assert all(c["rows"] for c in cs)
    nstruct = np.array([len(c["rows"]) - 1 for c in cs], np.int64)
    lengths = np.array([len(c["seq"]) for c in cs], np.int64)
    row_off, cell_off = _offsets(nstruct, lengths)
    partner = np.concatenate([partner_row(r["dbn"]) for c in cs for r in c["rows"]])
    tables = dict(partner=torch.from_numpy(partner), scores=torch.zeros((int(row_off[-1]), 3), dtype=torch.float64),
                  pset_mask=torch.zeros(int(row_off[-1]), dtype=torch.int64), metrics=torch.zeros((len(cs), 16), dtype=torch.float64),
                  row_off=torch.from_numpy(row_off), cell_off=torch.from_numpy(cell_off))
    if device is not None:
        tables = {k: t.to(device) for k, t in tables.items()}
    return FoldResult([">" + c["name"] for c in cs], [c["seq"] for c in cs], [[] for _ in cs], tables, nstruct, lengths, "host")


#: the sweep of the metric ratios: the sizes of the known structures, one 200-nt record each; the pairs are (q, 199 - q)
SWEEP_KNOWN = (0, 1, 3, 16, 48, 80)
SWEEP_N = 200
_sweep = None


def sweep_counts():
    """(K, TP, FP) of every row of the sweep, in the order of its rows: per known size K, TP = 0 .. K of the known pairs and
    FP = 0 .. min(96, 100 - K) of the pairs beyond them."""
    return [(K, tp, fp) for K in SWEEP_KNOWN for tp in range(K + 1) for fp in range(min(96, SWEEP_N // 2 - K) + 1)]


def sweep_ratios(K, tp, fp):
    """{column of the metrics: (numerator, denominator)} of the ratios a row forms (SQRNdbnali.py:205-207); none where the
    denominator is empty."""
    fn = K - tp
    out = {3: (2 * tp, 2 * tp + fp + fn), 4: (tp, tp + fp), 5: (tp, tp + fn)}
    return {k: r for k, r in out.items() if r[1]}


def sweep_metrics(K, tp, fp):
    """TP FP FN FS PR RC of a row in plain Python, as the reference's Metrics forms them."""
    ratios = sweep_ratios(K, tp, fp)
    return [tp, fp, K - tp] + [round(ratios[k][0] / ratios[k][1], 3) if k in ratios else 1 for k in (3, 4, 5)]


def round3_floor(x):
    """A wrong round(x, 3): half up on the product."""
    import math
    return math.floor(1000 * x + 0.5) / 1000


def round3_product(x):
    """A wrong round(x, 3): ties to even on the ROUNDED product 1000 x, not on the exact binary value."""
    return round(1000 * x) / 1000


def sweep_telling(wrong):
    """The distinct (numerator, denominator) among the sweep's ratios on which `wrong` differs from round(x, 3)."""
    seen = {r for row in sweep_counts() for r in sweep_ratios(*row).values()}
    return {r for r in seen if wrong(r[0] / r[1]) != round(r[0] / r[1], 3)}


def sweep():
    """(records, int32[6, Kmax, 200] padded partner rows, nstruct, expected float64[rows, 6]) of the sweep, built once and
    left unchanged.  Record r's known structure holds the pairs (q, 199 - q), q < SWEEP_KNOWN[r]; a row holds the first TP of
    them and the FP pairs q = K .. K + FP - 1."""
    global _sweep
    if _sweep is None:
        rng = np.random.default_rng(200)
        n, counts = SWEEP_N, sweep_counts()
        nstruct = np.array([sum(1 for c in counts if c[0] == K) for K in SWEEP_KNOWN], np.int64)
        rows = np.full((len(SWEEP_KNOWN), int(nstruct.max()), n), -1, np.int32)
        recs = []
        for r, K in enumerate(SWEEP_KNOWN):
            tp = np.array([c[1] for c in counts if c[0] == K])
            fp = np.array([c[2] for c in counts if c[0] == K])
            block = rows[r, :len(tp)]
            for q in range(n // 2):
                held = (q < tp) | ((q >= K) & (q < K + fp))
                block[held, q], block[held, n - 1 - q] = n - 1 - q, q
            recs.append((">sweep_%d" % K, ''.join(rng.choice(list("ACGU"), n)), None, None, "(" * K + "." * (n - 2 * K) + ")" * K))
        _sweep = (recs, rows, nstruct, np.array([sweep_metrics(*c) for c in counts], np.float64))
    return _sweep


def same(a, b):
    """Equal as float64 values, NaN equal to NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def input_stems(c, row):
    """The golden stems of a row (gap-free coordinates) in columns of the sequence as given."""
    col = [i for i, ch in enumerate(c["seq"]) if ch not in "-.~"]
    return [(col[i], col[j], ln) for i, j, ln in row["stems"]]


def check_golden(res, cs):
    """res = Score of the cases cs with all their structures, in any form: every value equals the reference's."""
    host = res.cpu()
    assert len(res) == len(cs) and host.row_off.tolist() == np.concatenate([[0], np.cumsum([len(c["rows"]) for c in cs])]).tolist()
    assert host.status.tolist() == [0] * int(host.row_off[-1])
    q = 0
    for r, c in enumerate(cs):
        assert same(host.ref_scores[r].tolist(), c["ref_scores"] if c["known"] else NAN6[:3]), c["name"]
        for row in c["rows"]:
            assert same(host.scores[q].tolist(), row["scores"]), (c["name"], row["dbn"], host.scores[q].tolist(), row["scores"])
            assert same(host.metrics[q].tolist(), row["metrics"] if c["known"] else NAN6), (c["name"], row["dbn"], host.metrics[q].tolist())
            stems = input_stems(c, row)
            assert host.stems_of(q) == stems, (c["name"], row["dbn"])
            assert int(host.nstems[q]) == len(stems) and int(host.npairs[q]) == sum(s[2] for s in stems)
            q += 1
    assert int(host.stem_off[-1]) == len(host.stems)


def equal_results(a, b):
    """Two ScoreResults hold the same values (wherever their tensors live)."""
    a, b = a.cpu(), b.cpu()
    assert a.names == b.names and a.sequences == b.sequences
    for k in ("status", "nstems", "npairs", "stems", "stem_off", "row_off"):
        assert getattr(a, k).tolist() == getattr(b, k).tolist(), k
    for k in ("scores", "metrics", "ref_scores"):
        assert same(getattr(a, k).numpy(), getattr(b, k).numpy()), k
