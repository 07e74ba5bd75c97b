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
