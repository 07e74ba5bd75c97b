"""Shared checks of the FoldWindows() tests (CPU: tests/test_fold_windows_api.py, tests/test_windows_host.py; GPU:
tests/test_hip_fold_windows.py): a plain-Python restatement of the windowed mode's semantics -- the starts, a dict count, the
coverage by enumeration, freq, the rank order as a sorted() key, a sequential first fit -- and check_result(), which forms
every tensor of a WindowResult again from its windows' consensus rows.  Every comparison is exact: integers, and doubles bit
for bit."""
import bisect
import random

from squarna_amd.dbn import PairsToDBN
from tests.fold_checks import same_doubles

LIMITS = (0, 0.2, 0.35, 0.5, 1)


def starts_of(N, window, step):
    if N <= window:
        return [0]
    out, a = [], 0
    while a + window <= N:
        out.append(a)
        a += step
    if (N - window) % step != 0:
        out.append(N - window)
    return out


def dict_count(rows, starts):
    """{(i, j): (count, first)} over the windows of ONE record: rows[k] = the partner list of window k (its own coordinates),
    starts[k] = its start.  Only entries that are pairs inside the window count (j > i, row[j] == i)."""
    table = {}
    for k, (row, a) in enumerate(zip(rows, starts)):
        for t, p in enumerate(row):
            if t < p < len(row) and row[p] == t:
                c, f = table.get((a + t, a + p), (0, k))
                table[(a + t, a + p)] = (c + 1, f)
    return table


def cover_enum(i, j, starts, wlen):
    return sum(1 for a in starts if a <= i and j < a + wlen)


def cover_sorted(i, j, starts, wlen):
    """The same number for ascending starts without the walk over all windows (the large synthetic cases)."""
    return bisect.bisect_right(starts, i) - bisect.bisect_right(starts, j - wlen)


def ranked_table(rows, starts, wlen, cover=cover_enum):
    """[(i, j, count, cover, first)] of one record in rank order: freq descending, count descending, first, i, j ascending."""
    table = dict_count(rows, starts)
    full = [(i, j, c, cover(i, j, starts, wlen), f) for (i, j), (c, f) in table.items()]
    return sorted(full, key=lambda e: (-(e[2] / e[3]), -e[2], e[4], e[0], e[1]))


def first_fit(ranked, limit, N, key=None):
    """The partner list of the sequential pass over the prefix freq >= limit of a ranked table."""
    partner = [-1] * N
    for i, j, c, cov, f in (ranked if key is None else sorted(ranked, key=key)):
        if c / cov >= limit and partner[i] < 0 and partner[j] < 0:
            partner[i], partner[j] = j, i
    return partner


def by_cell_only(e):
    """The order that ignores count and first among equal frequencies: what the rank order must differ from somewhere."""
    return (-(e[2] / e[3]), e[0], e[1])


def window_rows(res):
    """Per record the partner lists of its windows' consensus rows, from res.windows."""
    w = res.windows.cpu()
    partner, cell_off, lengths = w.partner.tolist(), w.cell_off.tolist(), w.lengths.tolist()
    win_off = res.win_off.tolist()
    rows = [partner[cell_off[k]:cell_off[k] + lengths[k]] for k in range(len(w))]
    return [rows[win_off[r]:win_off[r + 1]] for r in range(len(res))]


def check_result(res, references=None):
    """Every tensor of a WindowResult (any device) against the restatement, from the rows of res.windows.
    references: per record the reference line or None (default: none has one).  Returns the ranked tables."""
    import torch
    from squarna_amd import align
    for key, dtype in (("pos_off", torch.int64), ("win_off", torch.int64), ("starts", torch.int64), ("pair_off", torch.int64),
                       ("pair_pos", torch.int32), ("pair_count", torch.int32), ("pair_cover", torch.int32), ("pair_first", torch.int32),
                       ("consensus", torch.int32), ("metrics", torch.float64)):
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == res.device, key
    R = len(res)
    assert len(res.names) == len(res.sequences) == R
    lens = [len(s) for s in res.sequences]
    pos_off, win_off, pair_off = [0], [0], [0]
    starts, tables = [], []
    rows = window_rows(res)
    for r, N in enumerate(lens):
        s = starts_of(N, res.window, res.step)
        starts += s
        pos_off.append(pos_off[-1] + N)
        win_off.append(win_off[-1] + len(s))
        wlen = min(res.window, N)
        assert all(len(row) == wlen for row in rows[r]) and len(rows[r]) == len(s)
        names = res.windows.names[win_off[r]:win_off[r + 1]]
        assert names == ["%s/%d-%d" % (res.names[r], a + 1, a + wlen) for a in s]
        assert res.windows.sequences[win_off[r]:win_off[r + 1]] == [res.sequences[r][a:a + wlen] for a in s]
        tables.append(ranked_table(rows[r], s, wlen))
        pair_off.append(pair_off[-1] + len(tables[-1]))
    assert res.pos_off.tolist() == pos_off and res.win_off.tolist() == win_off and res.starts.tolist() == starts
    assert res.pair_off.tolist() == pair_off
    flat = [e for t in tables for e in t]
    assert res.pair_pos.tolist() == [[e[0], e[1]] for e in flat]
    assert res.pair_count.tolist() == [e[2] for e in flat]
    assert res.pair_cover.tolist() == [e[3] for e in flat]
    assert res.pair_first.tolist() == [e[4] for e in flat]
    assert tuple(res.pair_pos.shape) == (len(flat), 2)
    cons = [p for r, N in enumerate(lens) for p in first_fit(tables[r], res.freqlimit, N)]
    assert res.consensus.tolist() == cons
    assert tuple(res.metrics.shape) == (R, 6)
    for r, N in enumerate(lens):
        ref = references[r] if references else None
        row = cons[pos_off[r]:pos_off[r + 1]]
        line = PairsToDBN([(i, j) for i, j in enumerate(row) if j > i], N)
        assert same_doubles(res.metrics[r].tolist(), [float(x) for x in align.Metrics(ref, line)]), r
    return tables


def check_views(res, tables, limits=LIMITS):
    """consensus_at, pairs, dbn, pair_frequency and cpu() against the restatement."""
    import torch
    lens = [len(s) for s in res.sequences]
    pos_off = res.pos_off.tolist()
    for lim in limits:
        exp = [first_fit(tables[r], lim, N) for r, N in enumerate(lens)]
        got = res.consensus_at(lim)
        assert got.dtype == torch.int32 and got.device == res.device
        assert got.tolist() == [p for row in exp for p in row], lim
        for r, N in enumerate(lens):
            prs = [(i, j) for i, j in enumerate(exp[r]) if j > i]
            assert res.pairs(r, lim) == prs
            assert res.dbn(r, lim) == PairsToDBN(prs, N)
            assert res.dbn(r, lim, levellimit=1) == PairsToDBN(prs, N, levellimit=1)
    for r, N in enumerate(lens):
        own = res.consensus.tolist()[pos_off[r]:pos_off[r + 1]]
        assert res.pairs(r) == [(i, j) for i, j in enumerate(own) if j > i]
        assert res.dbn(r) == PairsToDBN(res.pairs(r), N)
        band = res.pair_frequency(r)
        width = min(res.window, N)
        assert band.dtype == torch.float64 and band.device == res.device and tuple(band.shape) == (N, width)
        exp = [[0.0] * width for _ in range(N)]
        for i, j, c, cov, f in tables[r]:
            exp[i][j - i] = c / cov
        assert all(same_doubles(g, e) for g, e in zip(band.tolist(), exp)), r
    host = res.cpu()
    assert host.device.type == "cpu" and host.windows.partner.device.type == "cpu" and host.source == res.source
    for key in res._TENSORS:
        a, b = getattr(host, key), getattr(res, key).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and a.view(torch.int64 if a.dtype == torch.float64 else a.dtype).tolist() == \
            b.view(torch.int64 if b.dtype == torch.float64 else b.dtype).tolist(), key
    assert host.consensus_at(0.2).tolist() == res.consensus_at(0.2).tolist()


def check_equal(a, b):
    """Two WindowResults (any devices): the same numbers everywhere but in `source` and the rounds."""
    import torch
    a, b = a.cpu(), b.cpu()
    assert (a.names, a.sequences, a.window, a.step, a.freqlimit) == (b.names, b.sequences, b.window, b.step, b.freqlimit)
    for key in a._TENSORS:
        x, y = getattr(a, key), getattr(b, key)
        assert x.dtype == y.dtype and x.shape == y.shape, key
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert x.tolist() == y.tolist(), key
    assert a.windows.partner.tolist() == b.windows.partner.tolist() and a.windows.names == b.windows.names
    assert a.windows.scores.view(torch.int64).tolist() == b.windows.scores.view(torch.int64).tolist()


def random_seq(seed, n):
    rng = random.Random(seed)                                            # (ONE generator per sequence: a new one per character repeats one letter)
    return ''.join(rng.choice('ACGU') for _ in range(n))


# the real-fold inputs: (sequence, window, step, configfile)
REAL = {"400_greedynobpp": (random_seq(1, 400), 60, 7, "greedynobpp"), "333_nobpp": (random_seq(2, 333), 70, 10, "nobpp")}


# ---- synthetic tables for the count alone (no fold) ----------------------------------------------------------------------
def synthetic_windows(rng, Ns, window, step, keep=0.7, extras=3, nested=False):
    """Windows of records of Ns nt with made-up consensus rows: per record a base structure of which every window keeps each
    pair it contains with probability `keep`, plus a few random pairs of its own; nested=True: every window holds the same
    nested pairs (0, wlen - 1), (1, wlen - 2), ...  Returns (gstart, lens, rows, per record (starts, wlen, its rows))."""
    gstart, lens, rows, per_rec, off = [], [], [], [], 0
    for N in Ns:
        wlen = min(window, N)
        base, free = {}, list(range(N))
        rng.shuffle(free)
        while len(free) >= 2:
            v, w = sorted((free.pop(), free.pop()))
            if w - v < wlen and rng.random() < 0.6:
                base[v] = w
        s = starts_of(N, window, step)
        mine = []
        for a in s:
            row = [-1] * wlen
            if nested:
                for t in range(wlen // 2):
                    row[t], row[wlen - 1 - t] = wlen - 1 - t, t
            else:
                for v, w in base.items():
                    if a <= v and w < a + wlen and rng.random() < keep:
                        row[v - a], row[w - a] = w - a, v - a
                for _ in range(rng.randint(0, extras)):
                    if wlen >= 2:
                        v, w = sorted(rng.sample(range(wlen), 2))
                        if row[v] == -1 and row[w] == -1:
                            row[v], row[w] = w, v
            gstart.append(off + a)
            lens.append(wlen)
            rows.append(row)
            mine.append(row)
        per_rec.append((s, wlen, mine))
        off += N
    return gstart, lens, rows, per_rec


def pack_tables(rows, rng, rec0=0):
    """The rows as pair tables in sq_result_pairs_dev's layout: `rec0` records of other content first, and a few structure
    rows of other content behind every consensus row.  Returns (partner list, cell_off list)."""
    partner, cell_off = [], [0]
    for _ in range(rec0):
        partner += [-1, 2, 1]
        cell_off.append(len(partner))
    for row in rows:
        partner += row
        for _ in range(rng.randint(0, 2)):
            partner += row[1:] + row[:1]                                  # (never read: only row 0 counts)
        cell_off.append(len(partner))
    return partner, cell_off


def expected_global(per_rec, Ns, cover=cover_enum):
    """{(gi, gj): (count, cover, first)} on the axis on which the records follow one another, first counting the windows of
    all records."""
    out, off, k0 = {}, 0, 0
    for (s, wlen, mine), N in zip(per_rec, Ns):
        for (i, j), (c, f) in dict_count(mine, s).items():
            out[(off + i, off + j)] = (c, cover(i, j, s, wlen), k0 + f)
        off += N
        k0 += len(s)
    return out
