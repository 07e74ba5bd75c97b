"""Shared checks of the FoldMutants() tests (CPU: tests/test_fold_mutants_api.py, tests/test_variants_host.py; GPU:
tests/test_hip_fold_mutants.py): a plain-Python restatement of the mutational scan's semantics -- the variants by string
slicing, lost / gained / kept as set differences of the rows' sets of pairs, changed / first / last by a per-position
comparison, pos_changed as a per-position count -- and check_result(), which forms every tensor and every method's answer of
a MutantResult again from the consensus rows of its folds.  Every comparison is exact: integers and strings."""
import math
import random

LETTERS = "ACGU"
GAPS_AND_SEPS = "-.~;&"


def norm(ch):
    up = ch.upper()
    return "U" if up == "T" else up


def random_seq(seed, n):
    rng = random.Random(seed)
    return ''.join(rng.choice(LETTERS) for _ in range(n))


def scan_variants(seq, positions=None):
    """The variants of a scan of seq: [[(pos, letter)], ...] in the order of the positions, then A, C, G, U."""
    where = range(len(seq)) if positions is None else sorted(set(positions))
    return [[(p, ch)] for p in where if norm(seq[p]) in LETTERS for ch in LETTERS if ch != norm(seq[p])]


def substitute(seq, sites):
    for p, ch in sites:
        seq = seq[:p] + norm(ch) + seq[p + 1:]
    return seq


def label(seq, sites):
    return "+".join("%s%d%s" % (seq[p].upper(), p + 1, norm(ch)) for p, ch in sites)


def pair_set(row):
    return {(t, p) for t, p in enumerate(row) if p > t}


def diff_row(w, v):
    """[lost, gained, kept, changed, first, last] of the partner lists w (wild type) and v (variant)."""
    assert len(w) == len(v)
    a, b = pair_set(w), pair_set(v)
    moved = [t for t in range(len(w)) if w[t] != v[t]]
    return [len(a - b), len(b - a), len(a & b), len(moved), moved[0] if moved else -1, moved[-1] if moved else -1]


def summary(wt_rows, var_rows):
    """(diff rows of all variants, pos_changed of all records' positions) for wt_rows[r] = the wild type's partner list and
    var_rows[r] = its variants' partner lists."""
    diff, pos_changed = [], []
    for w, mine in zip(wt_rows, var_rows):
        diff += [diff_row(w, v) for v in mine]
        pos_changed += [sum(1 for v in mine if v[t] != w[t]) for t in range(len(w))]
    return diff, pos_changed


def consensus_rows(folds):
    """The consensus row of every record of a FoldResult as a list."""
    f = folds.cpu()
    partner, cell_off, lengths = f.partner.tolist(), f.cell_off.tolist(), f.lengths.tolist()
    return [partner[cell_off[r]:cell_off[r] + lengths[r]] for r in range(len(f))]


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def check_result(res, positions=None, variants=None):
    """Every tensor and method of a MutantResult (any device) against the restatement, from the rows of res.folds.
    positions / variants: what the call was given.  Returns (the variants per record, the diff rows per record)."""
    import pytest
    import torch
    for key, dtype in (("pos_off", torch.int64), ("var_off", torch.int64), ("site_off", torch.int64), ("site_pos", torch.int32),
                       ("site_letter", torch.uint8), ("diff", torch.int32), ("pos_changed", torch.int32)):
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == res.device == res.folds.device, key
    assert tuple(res._TENSORS) == ("pos_off", "var_off", "site_off", "site_pos", "site_letter", "diff", "pos_changed")
    R = len(res)
    assert len(res.names) == len(res.sequences) == R and res.mode == ("scan" if variants is None else "explicit")
    wanted = [scan_variants(s, positions) for s in res.sequences] if variants is None else [[list(v) for v in per] for per in variants]
    V = sum(len(per) for per in wanted)
    assert len(res.folds) == R + V and res.folds.names[:R] == res.names and res.folds.sequences[:R] == res.sequences
    pos_off, var_off, site_off, site_pos, site_letter, names, seqs = [0], [0], [0], [], [], [], []
    for name, seq, per in zip(res.names, res.sequences, wanted):
        pos_off.append(pos_off[-1] + len(seq))
        var_off.append(var_off[-1] + len(per))
        for sites in per:
            site_off.append(site_off[-1] + len(sites))
            site_pos += [p for p, _ in sites]
            site_letter += [ord(norm(ch)) for _, ch in sites]
            names.append(name + "/" + label(seq, sites))
            seqs.append(substitute(seq, sites))
    assert res.folds.names[R:] == names and res.folds.sequences[R:] == seqs
    assert res.pos_off.tolist() == pos_off and res.var_off.tolist() == var_off and res.site_off.tolist() == site_off
    assert res.site_pos.tolist() == site_pos and res.site_letter.tolist() == site_letter
    rows = consensus_rows(res.folds)
    assert all(len(rows[R + m]) == len(rows[r]) for r in range(R) for m in range(var_off[r], var_off[r + 1]))
    diff, pos_changed = summary(rows[:R], [rows[R + var_off[r]:R + var_off[r + 1]] for r in range(R)])
    assert tuple(res.diff.shape) == (V, 6) and res.diff.tolist() == diff
    assert res.pos_changed.tolist() == pos_changed
    per_rec = []
    for r, (seq, per) in enumerate(zip(res.sequences, wanted)):
        mine = diff[var_off[r]:var_off[r + 1]]
        per_rec.append(mine)
        dist = [d[0] + d[1] for d in mine]
        got = res.distance(r)
        assert got.dtype == torch.int32 and got.device == res.device and got.tolist() == dist
        assert res.dbn(r) == res.folds.consensus(r)
        for k, sites in enumerate(per):
            assert res.variant(r, k) == (names[var_off[r] + k], [(p, seq[p], norm(ch)) for p, ch in sites])
        for k in sorted({0, len(per) // 2, len(per) - 1} & set(range(len(per)))):
            assert res.dbn(r, k) == res.folds.consensus(R + var_off[r] + k)
        for n in (0, 1, 10, len(per) + 3):
            top = res.most_disruptive(r, n) if n != 10 else res.most_disruptive(r)
            assert top.device == res.device and top.dtype == torch.int64
            assert top.tolist() == sorted(range(len(per)), key=lambda k: (-dist[k], k))[:n]
        if variants is not None:
            with pytest.raises(ValueError):
                res.to_matrix(r)
            with pytest.raises(ValueError):
                res.profile(r)
            continue
        matrix = [[-1] * 4 for _ in seq]
        for k, ((p, ch),) in enumerate(per):
            matrix[p][LETTERS.index(ch)] = dist[k]
        got = res.to_matrix(r)
        assert got.dtype == torch.int32 and got.device == res.device and tuple(got.shape) == (len(seq), 4) and got.tolist() == matrix
        prof = [[sum(have) / len(have), float(max(have))] if have else [math.nan, math.nan]
                for have in ([d for d in line if d >= 0] for line in matrix)]
        got = res.profile(r)
        assert got.dtype == torch.float64 and got.device == res.device and tuple(got.shape) == (len(seq), 2)
        assert all(_same(a, b) for g, e in zip(got.tolist(), prof) for a, b in zip(g, e)), r
    with pytest.raises(IndexError):
        res.distance(R)
    return wanted, per_rec


def check_equal(a, b):
    """Two MutantResults (any devices): the same numbers everywhere but in `source`."""
    import torch
    a, b = a.cpu(), b.cpu()
    assert (a.names, a.sequences, a.mode) == (b.names, b.sequences, b.mode)
    for key in a._TENSORS:
        x, y = getattr(a, key), getattr(b, key)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tolist() == y.tolist(), key
    assert a.folds.names == b.folds.names and a.folds.sequences == b.folds.sequences
    for key in ("partner", "pset_mask", "row_off", "cell_off", "nstruct", "lengths"):
        assert getattr(a.folds, key).tolist() == getattr(b.folds, key).tolist(), key
    assert a.folds.scores.view(torch.int64).tolist() == b.folds.scores.view(torch.int64).tolist()


# ---- synthetic rows for the device entry and the host program (no fold) ---------------------------------------------------
def random_row(rng, n, density=0.6):
    """A random symmetric partner list of n entries."""
    row, free = [-1] * n, list(range(n))
    rng.shuffle(free)
    while len(free) >= 2:
        v, w = free.pop(), free.pop()
        if rng.random() < density:
            row[v], row[w] = w, v
    return row


def nested_row(n):
    row = [-1] * n
    for t in range(n // 2):
        row[t], row[n - 1 - t] = n - 1 - t, t
    return row


def perturbed(rng, row):
    """A variant's row: the wild type's with some pairs dropped and a few new ones among the freed positions."""
    v = list(row)
    for t, p in enumerate(row):
        if p > t and rng.random() < 0.3:
            v[t] = v[p] = -1
    free = [t for t, p in enumerate(v) if p == -1]
    rng.shuffle(free)
    for _ in range(rng.randint(0, 3)):
        if len(free) >= 2:
            a, b = free.pop(), free.pop()
            v[a], v[b] = b, a
    return v


def plant_invalid(rng, row, kind):
    """row with one invalid entry of `kind` ("outside", "below", "self", "asymmetric") at a free position; None if it has none
    (or, for "asymmetric", fewer than 2 entries)."""
    free = [t for t, p in enumerate(row) if p == -1]
    if not free or (kind == "asymmetric" and len(row) < 2):
        return None
    out, t = list(row), rng.choice(free)
    if kind == "asymmetric":
        out[t] = rng.choice([p for p in range(len(row)) if p != t])       # (row[p] is -1 or another position: it does not point back)
    else:
        out[t] = {"outside": len(row) + rng.randint(0, 3), "below": -2 - rng.randint(0, 3), "self": t}[kind]
    return out


def pack_records(rng, wt_rows, var_rows, wt_of, extra=0):
    """Pair tables in Fold's layout: the wild types, `extra` records of other content, then the variants (variant m's wild
    type is wt_of[m]); every record has its row 0 and 0-3 structure rows of other content behind it.
    Returns (partner, cell_off, lengths, rec0, pos_off with rec0 + 1 entries, Ltot)."""
    partner, cell_off, lengths = [], [0], []
    for row in list(wt_rows) + [[-1, 2, 1]] * extra + list(var_rows):
        partner += row
        for _ in range(rng.randint(0, 3)):
            partner += row[1:] + row[:1]                                   # (never read: only row 0 counts)
        cell_off.append(len(partner))
        lengths.append(len(row))
    pos_off = [0]
    for row in wt_rows:
        pos_off.append(pos_off[-1] + len(row))
    Ltot = pos_off[-1]
    return partner, cell_off, lengths, len(wt_rows) + extra, pos_off + [Ltot] * extra, Ltot


def expected_flat(wt_rows, var_rows, wt_of):
    """(diff rows, pos_changed) for variants given in any order of their wild types."""
    diff = [diff_row(wt_rows[w], v) for v, w in zip(var_rows, wt_of)]
    pos_changed = []
    for r, w in enumerate(wt_rows):
        mine = [v for v, q in zip(var_rows, wt_of) if q == r]
        pos_changed += [sum(1 for v in mine if v[t] != w[t]) for t in range(len(w))]
    return diff, pos_changed
