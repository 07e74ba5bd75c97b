"""Checks shared by the CPU and GPU tests of Elements() (tests/test_elements_api.py, tests/test_elements_host.py,
tests/test_hip_elements.py): the literal table of the specification, a naive reference that is neither the host path's
stack walk nor the kernels' per-opener walk, a seeded generator of rows, and the exact comparison of results.  Not a test
module."""
import numpy as np

E, S, H, B, I, M, K = range(7)
LETTERS = "ESHBIMK&-"
_T = dict(zip("ESHBIM", range(6)))

#: (sequence, structure, element string, loops as (type, i, j, branches, unpaired, side5))
_TABLE_TEXT = """
A*11        ..((...))..               EESSHHHSSEE               (E,-1,11,1,4,2) (H,3,7,0,3,3)
A*12        ((.((...))))              SSBSSHHHSSSS              (E,-1,12,1,0,0) (B,1,10,1,1,1) (H,4,8,0,3,3)
A*13        ((.((...)).))             SSISSHHHSSISS             (E,-1,13,1,0,0) (I,1,11,1,2,1) (H,4,8,0,3,3)
A*24        ((..((...))..((...))..))  SSMMSSHHHSSMMSSHHHSSMMSS  (E,-1,24,1,0,0) (M,1,22,2,6,2) (H,5,9,0,3,3) (H,14,18,0,3,3)
A*14        ((..[[..))..]]            SSHHKKHHSSEEKK            (E,-1,14,1,4,0) (H,1,8,0,6,6)
A*16        (([[[..))..]]]..          KKSSSHHKKHHSSSEE          (E,-1,16,1,4,2) (H,4,11,0,6,6)
AAAA&AAAA   ((((.))))                 SSSS&SSSS                 (E,-1,9,1,0,0) (E,3,5,0,0,0)
AAAA&AAAA   ((.....))                 SSEE&EESS                 (E,-1,9,1,0,0) (E,1,7,0,4,4)
AA-AAAA-AA  ((.(..).))                SS-SHHS-SS                (E,-1,10,1,0,0) (H,3,6,0,2,2)
AAA         ...                       EEE                       (E,-1,3,0,3,3)
"""


def _parse_table():
    out = []
    for line in _TABLE_TEXT.strip().split("\n"):
        seq, dbn, text, *loops = line.split()
        if "*" in seq:
            seq = seq[0] * int(seq[2:])
        loops = [tuple(_T[x] if x in _T else int(x) for x in lp.strip("()").split(",")) for lp in loops]
        assert len(seq) == len(dbn) == len(text)
        out.append((seq, dbn, text, loops))
    return out


TABLE = _parse_table()


def table_cases():
    """The table as cases in the layout of tests/score_checks.py (strings_form, padded_form, fold_result_form)."""
    return [dict(name="t%d" % k, seq=seq, rows=[dict(dbn=dbn)]) for k, (seq, dbn, _, _) in enumerate(TABLE)]


def check_table(res):
    """res = Elements of the table's records, one row each, in any form."""
    host = res.cpu()
    assert host.status.tolist() == [0] * len(TABLE) and host.row_off.tolist() == list(range(len(TABLE) + 1))
    for q, (seq, dbn, text, loops) in enumerate(TABLE):
        assert host.text(q) == text, (seq, dbn, host.text(q))
        assert host.loops_of(q) == loops, (seq, dbn, host.loops_of(q))
        assert int(host.nloops[q]) == len(loops)
        want = naive(seq, partner_row(dbn))
        assert row_of(host, q) == want, (seq, dbn)
        assert text == ''.join(LETTERS[c] for c in want[1]) and loops == want[4]        # (the reference itself)


def partner_row(dbn, width=None):
    from tests.score_checks import partner_row as pr
    return pr(dbn, width)


def row_of(res, q):
    """Row q of a host ElementsResult in the form naive() returns."""
    a, b = int(res.cell_off[q]), int(res.cell_off[q + 1])
    return (int(res.status[q]), res.element[a:b].tolist(), res.level[a:b].tolist(), res.loop_of[a:b].tolist(), res.loops_of(q),
            int(res.npairs[q]), int(res.nlevels[q]))


def naive(seq, row):
    """(status, element, level, loop_of, loops, npairs, nlevels) of one partner row (input columns) under `seq`: every
    position that is not in a pair of level 1 looks for the narrowest pair of level 1 around it among ALL pairs; the loops
    follow from these assignments.  O(positions x pairs)."""
    from squarna_amd.dbn import PairsToDBN
    lin = len(seq)
    row = [int(x) for x in row[:lin]]
    gap = [ch in "-.~" for ch in seq]
    sep = [ch in ";&" for ch in seq]
    for c, p in enumerate(row):
        if p != -1 and (p < 0 or p >= lin or p == c or row[p] != c or sep[c]):
            return 1, [-1] * lin, [0] * lin, [-1] * lin, [], 0, 0
    cols = [c for c in range(lin) if not gap[c]]
    pos = {c: g for g, c in enumerate(cols)}
    pairs = [(c, p) for c, p in enumerate(row) if p > c and not gap[c] and not gap[p]]
    lev = PairsToDBN([(pos[v], pos[w]) for v, w in pairs], len(cols), returnlevels=True)
    lev = {(v, w): lev[(pos[v], pos[w])] for v, w in pairs}
    nested = [pw for pw in pairs if lev[pw] == 1]
    EXT = (-1, lin)

    def around(c, d):                                                # the narrowest nested pair strictly around columns c..d
        best = EXT
        for v, w in nested:
            if v < c and d < w and w - v < best[1] - best[0]:
                best = (v, w)
        return best
    level, element, inpair = [0] * lin, [None] * lin, {}
    for (v, w), l in lev.items():
        level[v], level[w] = l, -l
        inpair[v] = inpair[w] = l
    home = {c: around(c, c) for c in cols if inpair.get(c) != 1}
    parent = {pw: around(*pw) for pw in nested}
    loops = []
    for X in [EXT] + sorted(nested):
        kids = sorted(pw for pw in nested if parent[pw] == X)
        mine = [c for c in cols if home.get(c) == X]
        free = [c for c in mine if not sep[c]]
        brk = any(sep[c] for c in mine)
        first = kids[0][0] if kids else lin
        side5 = sum(c < first for c in free)
        if X == EXT or brk:
            kind = E
        elif not kids:
            kind = H
        elif len(kids) >= 2:
            kind = M
        elif not free:
            continue                                                 # a stack
        else:
            kind = I if 0 < side5 < len(free) else B
        loops.append((kind, X[0], X[1], len(kids), len(free), side5))
    index = {(lp[1], lp[2]): k for k, lp in enumerate(loops)}
    loop_of = [-1] * lin
    for c in range(lin):
        if gap[c]:
            element[c] = 8
        elif sep[c]:
            element[c] = 7
        elif c in inpair:
            element[c] = S if inpair[c] == 1 else K
        else:
            element[c] = loops[index[home[c]]][0]
        if c in home and not sep[c]:
            loop_of[c] = index[home[c]]
    return 0, element, level, loop_of, loops, len(pairs), max(lev.values(), default=0)


def random_row(seed, width, k=0, gaps=False, sep=False):
    """(sequence, partner row int32[width]) from a seed: nested helices with bulges, internal loops and multiloops, then up to
    `k` crossing helices on what is still free, gap columns (some on paired columns: those pairs are dropped, others stack
    across the gap) and one separator on an unpaired column."""
    rng = np.random.default_rng(seed)
    row = np.full(width, -1, np.int32)

    def fill(lo, hi, depth):                                         # nested helices inside columns lo .. hi - 1
        at = lo + int(rng.integers(0, 3))
        while hi - at >= 5 and depth < 6:
            ln = int(rng.integers(1, 5))
            span = int(rng.integers(2 * ln + 3, max(2 * ln + 4, min(hi - at, 60) + 1)))
            if at + span > hi:
                break
            a, b = at, at + span - 1
            for t in range(ln):
                row[a + t], row[b - t] = b - t, a + t
            a, b = a + ln, b - ln
            # the helix goes on behind a bulge or an internal loop, or closes a hairpin / a multiloop
            if b - a >= 8 and rng.random() < 0.5:
                a += int(rng.integers(0, 3)); b -= int(rng.integers(0, 3))
                if rng.random() < 0.5:
                    row[a], row[b] = b, a
                    a, b = a + 1, b - 1
            if b - a >= 3:
                fill(a + 1, b, depth + 1)
            at += span + int(rng.integers(0, 4))
    fill(0, width, 0)
    for _ in range(k):                                               # crossing helices (tools/score_probe.py's form)
        if width < 4:
            break
        a, b, ln = int(rng.integers(0, width - 1)), int(rng.integers(1, width)), int(rng.integers(1, 5))
        for t in range(ln):
            v, w = a + t, b - t
            if v < w and row[v] < 0 and row[w] < 0:
                row[v], row[w] = w, v
    seq = list(rng.choice(list("ACGU"), width)) if width else []
    if gaps:
        for c in np.flatnonzero(rng.random(width) < 0.08).tolist():
            seq[c] = "-.~"[int(rng.integers(0, 3))]
    free = [c for c in range(width) if row[c] < 0 and seq[c] not in "-.~"]
    if sep and free:
        seq[free[int(rng.integers(0, len(free)))]] = "&"
    return ''.join(seq), row


def row_dbn(row):
    """The dot-bracket string of a valid partner row (input columns, every pair kept)."""
    from squarna_amd.dbn import PairsToDBN
    return PairsToDBN([(c, int(p)) for c, p in enumerate(row) if p > c], len(row))


def mixed_records(widths=(0, 1, 63, 64, 65, 129, 263)):
    """(records, structures as partner rows per record): the widths around the wave with gaps, a separator and K = 0 .. 6
    rows of 0 .. 6 crossing helices."""
    recs, rows = [], []
    for r, w in enumerate(widths):
        K_ = r % 7
        made = [random_row(1000 * r + k, w, k=k, gaps=r % 2 == 1, sep=r % 3 == 2) for k in range(K_)]
        seq = made[0][0] if made else random_row(1000 * r, w, gaps=r % 2 == 1, sep=r % 3 == 2)[0]
        # (the rows of a record share its sequence: the generator's gaps and separator depend on the row, so rows whose pairs
        # fall on the first row's separator lose those pairs)
        keep = []
        for _, row in made:
            row = row.copy()
            for c in range(w):
                if seq[c] in ";&" and row[c] >= 0:
                    row[row[c]] = -1; row[c] = -1
            keep.append(row)
        recs.append((">m%d" % r, seq, None, None, None))
        rows.append(keep)
    return recs, rows


def padded(rows_per_record, extra=0):
    """(int32[R, K, Lmax], nstruct) of partner rows per record."""
    K_ = max((len(rows) for rows in rows_per_record), default=0)
    Lmax = max((len(row) for rows in rows_per_record for row in rows), default=0) + extra
    out = np.full((len(rows_per_record), max(K_, 1), max(Lmax, 1)), -1, np.int32)
    for r, rows in enumerate(rows_per_record):
        for k, row in enumerate(rows):
            out[r, k, :len(row)] = row
    return out, np.array([len(rows) for rows in rows_per_record], np.int64)


def check_naive(res, recs, rows_per_record):
    """Every row of res equals the naive reference."""
    host = res.cpu()
    q = 0
    for rec, rows in zip(recs, rows_per_record):
        seq = rec if isinstance(rec, str) else rec[1]
        for row in rows:
            assert row_of(host, q) == naive(seq, row), (seq, list(row))
            q += 1
    assert q == len(host.status) and int(host.loop_off[-1]) == len(host.loops) and int(host.cell_off[-1]) == len(host.element)


def equal_results(a, b):
    """Two ElementsResults hold the same values (wherever their tensors live)."""
    a, b = a.cpu(), b.cpu()
    assert a.names == b.names and a.sequences == b.sequences
    for k in a._TENSORS:
        assert getattr(a, k).dtype == getattr(b, k).dtype and getattr(a, k).tolist() == getattr(b, k).tolist(), k
