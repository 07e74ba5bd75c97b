"""Shared checks of the FoldDuplex() tests (CPU: tests/test_fold_duplex_api.py, tests/test_duplex_host.py; GPU:
tests/test_hip_fold_duplex.py): a plain-Python restatement of the duplex summary -- inter / intra as subsets of the duplex
row's set of pairs, lost as the solo rows' pairs the duplex lacks, the sites as the smallest and largest ends of the inter
pairs, bound as a per-position count --, a packer into the two-table layout, generators of rows and one planted invalid
entry.  Every comparison is exact: integers and strings."""
from tests.fold_mutants_checks import consensus_rows, nested_row, pair_set, plant_invalid, random_row, random_seq  # noqa: F401

#: the smallest lengths at which the walk of a duplex row can go wrong: nothing, one and two positions, the separator on lane
#: 63 or on lane 0 of the next chunk, chain B starting in the middle of a chunk, several chunks
BOUNDARY_LENGTHS = (0, 1, 2, 62, 63, 64, 65, 127, 128, 129, 300)


def revcomp(seq):
    return ''.join({"A": "U", "C": "G", "G": "C", "U": "A"}[ch] for ch in reversed(seq))


def expected_row(A, B, D):
    """The nine numbers of the duplex row D over the solo rows A and B (partner lists)."""
    nA = len(A)
    assert len(D) == nA + 1 + len(B) and D[nA] == -1
    pairs = pair_set(D)
    inter = {(i, j) for i, j in pairs if i < nA < j}
    intra_a = {(i, j) for i, j in pairs if j < nA}
    intra_b = {(i, j) for i, j in pairs if i > nA}
    assert len(inter) + len(intra_a) + len(intra_b) == len(pairs)
    lost_a = {(i, p) for i, p in pair_set(A) if D[i] != p}
    lost_b = {(u, p) for u, p in pair_set(B) if D[nA + 1 + u] != p + nA + 1}
    ends_a, ends_b = sorted(i for i, _ in inter), sorted(j - nA - 1 for _, j in inter)
    return [len(inter), len(intra_a), len(intra_b), len(lost_a), len(lost_b), ends_a[0] if inter else -1, ends_a[-1] if inter else -1,
            ends_b[0] if inter else -1, ends_b[-1] if inter else -1]


def expected_summary(solo_rows, dup_rows, a_of, b_of):
    """(the nine numbers per duplex, bound of all solo records' positions one after the other) for duplex k = the chains
    solo_rows[a_of[k]] and solo_rows[b_of[k]]."""
    summary = [expected_row(solo_rows[a], solo_rows[b], D) for D, a, b in zip(dup_rows, a_of, b_of)]
    bound = [[0] * len(row) for row in solo_rows]
    for D, a, b in zip(dup_rows, a_of, b_of):
        nA = len(solo_rows[a])
        for i, j in pair_set(D):
            if i < nA < j:
                bound[a][i] += 1
                bound[b][j - nA - 1] += 1
    return summary, [c for per in bound for c in per]


# ---- rows -----------------------------------------------------------------------------------------------------------------
def concat_row(A, B):
    """The duplex in which both chains keep the structures they have alone: no inter pair, nothing lost."""
    nA = len(A)
    return list(A) + [-1] + [p + nA + 1 if p >= 0 else -1 for p in B]


def dropped_row(rng, A, B, p=0.4):
    """concat_row with some pairs opened: lost > 0 without an inter pair."""
    D = concat_row(A, B)
    for t, q in enumerate(list(D)):
        if q > t and rng.random() < p:
            D[t] = D[q] = -1
    return D


def bind_row(rng, A, B, width=None):
    """concat_row with a window of A opened and paired, antiparallel, to an opened window of B."""
    D, nA, nB = concat_row(A, B), len(A), len(B)
    w = min(nA, nB, width or rng.randint(1, 14))
    if not w:
        return D
    i0, j0 = rng.randint(0, nA - w), rng.randint(0, nB - w)
    for t in list(range(i0, i0 + w)) + list(range(nA + 1 + j0, nA + 1 + j0 + w)):
        if D[t] >= 0:
            D[D[t]] = -1
            D[t] = -1
    for i in range(w):
        t, q = i0 + i, nA + j0 + w - i
        D[t], D[q] = q, t
    return D


def inter_only_row(rng, nA, nB, density=0.7):
    """A duplex whose pairs all cross the separator."""
    D = [-1] * (nA + 1 + nB)
    left, right = list(range(nA)), list(range(nA + 1, nA + 1 + nB))
    rng.shuffle(left); rng.shuffle(right)
    for t, q in zip(left, right):
        if rng.random() < density:
            D[t], D[q] = q, t
    return D


def random_duplex_row(rng, nA, nB, density=0.6):
    """A random symmetric duplex row: pairs inside either chain and across, the separator free."""
    D, free = [-1] * (nA + 1 + nB), [t for t in range(nA + 1 + nB) if t != nA]
    rng.shuffle(free)
    while len(free) >= 2:
        v, w = free.pop(), free.pop()
        if rng.random() < density:
            D[v], D[w] = w, v
    return D


ROW_KINDS = ("concat", "dropped", "bind", "inter_only", "random", "empty")


def duplex_row(rng, kind, A, B):
    return {"concat": lambda: concat_row(A, B), "dropped": lambda: dropped_row(rng, A, B), "bind": lambda: bind_row(rng, A, B),
            "inter_only": lambda: inter_only_row(rng, len(A), len(B)), "random": lambda: random_duplex_row(rng, len(A), len(B)),
            "empty": lambda: [-1] * (len(A) + 1 + len(B))}[kind]()


# ---- the two-table layout -------------------------------------------------------------------------------------------------
def _table(rng, rows):
    """(partner, cell_off, lengths) in Fold's layout: every record has its row 0 and 1-3 structure rows of other content
    behind it, so row 0 is never the whole record."""
    partner, cell_off, lengths = [], [0], []
    for row in rows:
        partner += row
        for _ in range(rng.randint(1, 3)):
            partner += row[1:] + row[:1]                                     # (never read: only row 0 counts)
        cell_off.append(len(partner))
        lengths.append(len(row))
    return partner, cell_off, lengths


def pack_tables(rng, solo_rows, dup_rows, one_table=False, unrelated=0):
    """The solo and the duplex rows as pair tables: dict(partner_s, cell_off_s, lengths_s, partner_d, cell_off_d, lengths_d,
    pos_off, Ltot, same).  one_table: both are parts of ONE table -- the solos, `unrelated` records of other content, the
    duplexes --, partner_d is partner_s and cell_off_d / lengths_d are that table's from the first duplex on (same = True);
    else the duplexes have a table of their own, the unrelated records in front of them."""
    other = [[-1, 2, 1]] * unrelated
    ns = len(solo_rows)
    if one_table:
        partner, cell_off, lengths = _table(rng, list(solo_rows) + other + list(dup_rows))
        t = dict(partner_s=partner, cell_off_s=cell_off[:ns + 1], lengths_s=lengths[:ns], partner_d=partner,
                 cell_off_d=cell_off[ns + unrelated:], lengths_d=lengths[ns + unrelated:], same=True)
    else:
        partner, cell_off, lengths = _table(rng, solo_rows)
        pd, cd, ld = _table(rng, other + list(dup_rows))
        t = dict(partner_s=partner, cell_off_s=cell_off, lengths_s=lengths, partner_d=pd, cell_off_d=cd[unrelated:], lengths_d=ld[unrelated:],
                 same=False)
    pos_off = [0]
    for row in solo_rows:
        pos_off.append(pos_off[-1] + len(row))
    t["pos_off"], t["Ltot"] = pos_off, pos_off[-1]
    return t


# ---- a DuplexResult against the restatement -------------------------------------------------------------------------------
def check_result(res, targets, queries, pairs):
    """Every tensor and helper of a DuplexResult (any device) against the restatement, from the rows of res.solos / res.folds.
    targets / queries: the sequences (queries None: the targets against themselves); pairs: the (a, b) list the call should
    have folded.  Returns (solo rows, duplex rows, the nine numbers per duplex)."""
    import math
    import pytest
    import torch
    T, Q = len(targets), len(queries or [])
    b0 = T if queries is not None else 0
    for key, dtype in (("a_rec", torch.int32), ("b_rec", torch.int32), ("pos_off", torch.int64), ("summary", torch.int32),
                       ("bound", torch.int32)):
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == res.device == res.solos.device, key
    assert tuple(res._TENSORS) == ("a_rec", "b_rec", "pos_off", "summary", "bound")
    P = len(pairs)
    assert len(res) == P and res.target_sequences == list(targets) and res.query_sequences == list(queries or [])
    assert len(res.target_names) == T and len(res.query_names) == Q and len(res.solos) == T + Q
    assert res.solos.sequences == list(targets) + list(queries or []) and res.solos.names == res.target_names + res.query_names
    assert res.a_rec.tolist() == [a for a, _ in pairs] and res.b_rec.tolist() == [b + b0 for _, b in pairs]
    seqs = res.solos.sequences
    pos_off = [0]
    for s in seqs:
        pos_off.append(pos_off[-1] + len(s))
    assert res.pos_off.tolist() == pos_off
    solo_rows = consensus_rows(res.solos)
    if not P:
        assert res.folds is None and tuple(res.summary.shape) == (0, 9) and res.bound.tolist() == [0] * pos_off[-1]
        assert res.disruption().numel() == 0 and res.score_gain().numel() == 0
        return solo_rows, [], []
    assert res.folds.device == res.device and len(res.folds) == P
    assert res.folds.sequences == [seqs[a] + "&" + seqs[b + b0] for a, b in pairs]
    assert res.folds.names == [res.solos.names[a] + "&" + res.solos.names[b + b0] for a, b in pairs]
    assert res.folds.metrics.isnan().all()                                   # (references are not carried over)
    dup_rows = consensus_rows(res.folds)
    a_of, b_of = [a for a, _ in pairs], [b + b0 for _, b in pairs]
    assert all(D[len(seqs[a])] == -1 for D, a in zip(dup_rows, a_of))        # (the separator column is never paired)
    summary, bound = expected_summary(solo_rows, dup_rows, a_of, b_of)
    assert tuple(res.summary.shape) == (P, 9) and res.summary.tolist() == summary
    assert res.bound.tolist() == bound
    # ---- the helpers
    dis = res.disruption()
    assert dis.dtype == torch.int32 and dis.device == res.device and dis.tolist() == [s[3] + s[4] for s in summary]
    first = {}
    for k, p in enumerate(pairs):
        first.setdefault(tuple(p), k)
    solo_scores = res.solos.cpu()
    dup_scores = res.folds.cpu()
    gain = res.score_gain()
    assert gain.dtype == torch.float64 and gain.device == res.device and tuple(gain.shape) == (P,)

    def first_total(f, r):
        return float(f.scores[int(f.row_off[r]), 0]) if int(f.nstruct[r]) else math.nan
    for k, (a, b) in enumerate(pairs):
        assert res.index(a, b) == first[(a, b)]
        assert res.dbn(k) == res.folds.consensus(k) and res.dbn(k)[len(seqs[a])] == "&"
        assert res.site(k) == ((summary[k][5], summary[k][6]), (summary[k][7], summary[k][8]))
        assert all(isinstance(x, int) for side in res.site(k) for x in side)
        assert int(res.disruption(k)) == summary[k][3] + summary[k][4]
        nA, nB = len(seqs[a]), len(seqs[b + b0])
        want = [[dup_rows[k][i] == nA + 1 + j for j in range(nB)] for i in range(nA)]
        got = res.contacts(k)
        assert got.dtype == torch.bool and got.device == res.device and tuple(got.shape) == (nA, nB) and got.tolist() == want
        assert int(got.sum()) == summary[k][0]
        exp = first_total(dup_scores, k) - first_total(solo_scores, a) - first_total(solo_scores, b + b0)
        g = float(gain[k])
        assert (math.isnan(g) and math.isnan(exp)) or g == exp, k
    with pytest.raises(KeyError):
        res.index(T, 0)
    with pytest.raises(IndexError):
        res.dbn(P)
    for r in range(T + Q):
        assert res.solo_dbn(r) == res.solos.consensus(r)
        got = res.bound_of(r)
        assert got.dtype == torch.int32 and got.device == res.device and got.tolist() == bound[pos_off[r]:pos_off[r + 1]]
    nb = Q if queries is not None else T
    for col in (0, 3, 6):
        if len(set(map(tuple, pairs))) != P:
            with pytest.raises(ValueError):
                res.to_matrix(col)
            continue
        want = [[-1] * nb for _ in range(T)]
        for k, (a, b) in enumerate(pairs):
            want[a][b] = summary[k][col]
        got = res.to_matrix(col) if col else res.to_matrix()
        assert got.dtype == torch.int32 and got.device == res.device and tuple(got.shape) == (T, nb) and got.tolist() == want
    for a in range(T):
        mine = [(b, summary[k][0]) for k, (x, b) in enumerate(pairs) if x == a]
        if queries is None:
            mine += [(x, summary[k][0]) for k, (x, b) in enumerate(pairs) if b == a and x != a]
        ranked = [b for b, _ in sorted(mine, key=lambda e: (-e[1], e[0]))]
        for n in (0, 1, 10, len(mine) + 2):
            top = res.best_partners(a, n) if n != 10 else res.best_partners(a)
            assert top.dtype == torch.int64 and top.device == res.device and top.tolist() == ranked[:n]
    return solo_rows, dup_rows, summary


def check_equal(x, y):
    """Two DuplexResults (any devices): the same numbers everywhere but in `source`."""
    import torch
    x, y = x.cpu(), y.cpu()
    assert (x.target_names, x.query_names, x.target_sequences, x.query_sequences) == (y.target_names, y.query_names, y.target_sequences, y.query_sequences)
    for key in x._TENSORS:
        p, q = getattr(x, key), getattr(y, key)
        assert p.dtype == q.dtype and p.shape == q.shape and p.tolist() == q.tolist(), key
    for f, g in ((x.solos, y.solos), (x.folds, y.folds)):
        assert (f is None) == (g is None)
        if f is None:
            continue
        assert f.names == g.names and f.sequences == g.sequences
        for key in ("partner", "pset_mask", "row_off", "cell_off", "nstruct", "lengths"):
            assert getattr(f, key).tolist() == getattr(g, key).tolist(), key
        assert f.scores.view(torch.int64).tolist() == g.scores.view(torch.int64).tolist()
