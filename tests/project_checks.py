"""Helpers of the Project / Lift tests (no tests here): seeded generators of aligned rows and of structure lines, and the naive
reference -- plain Python loops over characters, a third form beside the numpy path (cumsum + fancy indexing) and the kernel
(ballot words)."""
import random

LETTERS = "ACGUacgutTN-.~&"
GAP_CHARS = "-.~"
PAIR_TYPES = ["AU", "UA", "GC", "CG", "GU", "UG"]
#: the shapes of the issue: L around the 64-column chunk and the four chunks a block walks at a time
WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 257, 64 * 4 + 1)


def aligned_rows(seed, R, L, gap_share=0.3, letters=LETTERS):
    """R strings of L characters: a gap with probability gap_share, else a non-gap letter of `letters`."""
    rng = random.Random(seed)
    gaps = [ch for ch in letters if ch in GAP_CHARS] or ["-"]
    residues = [ch for ch in letters if ch not in GAP_CHARS]
    return ["".join(rng.choice(gaps) if rng.random() < gap_share else rng.choice(residues) for _ in range(L)) for _ in range(R)]


def special_rows(L):
    """Rows of L columns that are all gaps, have no gap, or have gaps only in the first or in the last 64-column chunk."""
    body = ("GCAUGUNacgu" * (L // 11 + 1))[:L]
    head, tail = min(L, 64), min(L, 64)
    first = "".join("-" if c < head and c % 3 != 1 else body[c] for c in range(L))
    last = "".join("~" if c >= L - tail and c % 2 else body[c] for c in range(L))
    return ["-" * L, body, first, last, "." * L]


def structure_line(seed, L, knots=False, density=0.6):
    """A valid partner list over L columns: nested pairs drawn at random, and with `knots` a second layer of nested pairs over
    the columns left free, which crosses the first."""
    rng = random.Random(seed)
    p = [-1] * L

    def layer(cols, share):
        stack = []
        for c in cols:
            x = rng.random()
            if x < share / 2:
                stack.append(c)
            elif x < share and stack:
                v = stack.pop()
                p[v], p[c] = c, v

    layer(range(L), density)
    if knots:
        layer([c for c in range(L) if p[c] < 0], density)
    return p


def class_line(row):
    """A valid line over the columns of `row` in which consecutive free columns pair up at distance 1, 2, 3, ...: with rows
    from LETTERS every class occurs soon."""
    L, p, c, d = len(row), [-1] * len(row), 0, 1
    while c + d < L:
        if p[c] < 0 and p[c + d] < 0:
            p[c], p[c + d] = c + d, c
            d = d % 4 + 1
        c += 1
    return p


def letter(ch):
    up = ch.upper()
    if up == "T":
        return "U"
    if up in "ACGU":
        return up
    return "-" if ch in GAP_CHARS else "N"


def pair_class(a, b):
    """The class 1..9 of a pair from the characters at its opening and closing column."""
    a, b = letter(a), letter(b)
    if a == "-" and b == "-":
        return 9
    if a == "-" or b == "-":
        return 8
    return PAIR_TYPES.index(a + b) + 1 if a + b in PAIR_TYPES else 7


def line_is_bad(p, width):
    for c in range(width):
        q = p[c]
        if q < -1 or q >= width or q == c:
            return True
        if q >= 0 and p[q] != c:
            return True
    return False


def gap_map(row):
    """(col_of, pos_of) of one row string."""
    col_of, pos_of = [], []
    for c, ch in enumerate(row):
        if ch in GAP_CHARS:
            pos_of.append(-1)
        else:
            pos_of.append(len(col_of))
            col_of.append(c)
    return col_of, pos_of


def naive(rows, lines, canonical_only=False, min_loop=0):
    """The reference of Project: rows = strings of one length L; lines = K partner lists (shared) or, per row, K partner
    lists.  Returns lists per row (and line): length, col_of and partner without padding, pos_of, cls, counts, status."""
    shared = not isinstance(lines[0][0], (list, tuple))
    out = dict(length=[], col_of=[], pos_of=[], partner=[], cls=[], counts=[], status=[])
    for r, row in enumerate(rows):
        L = len(row)
        col_of, pos_of = gap_map(row)
        mine = lines if shared else lines[r]
        partner, cls, counts, status = [], [], [], []
        for p in mine:
            proj, kinds, cnt = [-1] * len(col_of), [0] * L, [0] * 12
            bad = line_is_bad(p, L)
            if not bad:
                for v in range(L):
                    w = p[v]
                    if w <= v:
                        continue
                    k = pair_class(row[v], row[w])
                    kinds[v] = k
                    cnt[0] += 1
                    cnt[k] += 1
                    if k > 7 or (k == 7 and canonical_only):
                        continue
                    inner = 0
                    for c in range(v + 1, w):
                        inner += row[c] not in GAP_CHARS
                    if inner < min_loop:
                        cnt[10] += 1
                        continue
                    cnt[11] += 1
                    proj[pos_of[v]], proj[pos_of[w]] = pos_of[w], pos_of[v]
            partner.append(proj)
            cls.append(kinds)
            counts.append(cnt)
            status.append(int(bad))
        for key, val in (("length", len(col_of)), ("col_of", col_of), ("pos_of", pos_of), ("partner", partner), ("cls", cls),
                         ("counts", counts), ("status", status)):
            out[key].append(val)
    return out


def naive_lift(rows, short):
    """The reference of Lift: short[r] = the lines of row r as partner lists over its residues.  Returns per row: length,
    col_of, pos_of, partner (per line a list over the L columns), status."""
    out = dict(length=[], col_of=[], pos_of=[], partner=[], status=[])
    for row, mine in zip(rows, short):
        col_of, pos_of = gap_map(row)
        partner, status = [], []
        for p in mine:
            bad = line_is_bad(p, len(col_of))
            lifted = [-1] * len(row)
            if not bad:
                for i, q in enumerate(p[:len(col_of)]):
                    if q >= 0:
                        lifted[col_of[i]] = col_of[q]
            partner.append(lifted)
            status.append(int(bad))
        for key, val in (("length", len(col_of)), ("col_of", col_of), ("pos_of", pos_of), ("partner", partner), ("status", status)):
            out[key].append(val)
    return out


def project_lists(res):
    """A ProjectResult in naive()'s form; the padding of col_of and partner must be -1."""
    length = res.length.tolist()
    col_of, partner = res.col_of.tolist(), res.partner.tolist()
    for r, n in enumerate(length):
        assert all(x == -1 for x in col_of[r][n:]), ("col_of padding", r)
        assert all(x == -1 for line in partner[r] for x in line[n:]), ("partner padding", r)
    return dict(length=length, col_of=[row[:n] for row, n in zip(col_of, length)], pos_of=res.pos_of.tolist(),
                partner=[[line[:n] for line in lines] for lines, n in zip(partner, length)], cls=res.cls.tolist(),
                counts=res.counts.tolist(), status=res.status.tolist())


def lift_lists(res, counts):
    """A LiftResult in naive_lift()'s form (counts[r] = the lines of row r); the lines beyond a row's own must be -1 with
    status 0."""
    length = res.length.tolist()
    col_of, partner, status = res.col_of.tolist(), res.partner.tolist(), res.status.tolist()
    assert res.nstruct.tolist() == list(counts)
    for r, n in enumerate(length):
        assert all(x == -1 for x in col_of[r][n:]), ("col_of padding", r)
        assert all(x == -1 for line in partner[r][counts[r]:] for x in line) and not any(status[r][counts[r]:]), ("lines beyond nstruct", r)
    return dict(length=length, col_of=[row[:n] for row, n in zip(col_of, length)], pos_of=res.pos_of.tolist(),
                partner=[lines[:k] for lines, k in zip(partner, counts)], status=[s[:k] for s, k in zip(status, counts)])


def check_equal(got, exp, note=None):
    for key in exp:
        assert got[key] == exp[key], (key, note)


def short_lines(seed, rows, K, knots=False):
    """Per row K valid partner lists over the row's residues."""
    return [[structure_line(seed * 1000 + 10 * r + k, sum(ch not in GAP_CHARS for ch in row), knots) for k in range(K)]
            for r, row in enumerate(rows)]
