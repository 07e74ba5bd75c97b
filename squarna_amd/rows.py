"""Host helpers on partner rows (entry i: the 0-based partner of position i, -1 unpaired) and on the offsets of records that
follow one another on one axis.  numpy only; the result classes and the entries' host paths share them.
"""
import numpy as np


def offsets(counts):
    """int64[n + 1]: where each of n consecutive blocks of `counts` entries starts, and the total."""
    out = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=out[1:])
    return out


def position_axis(seqs):
    """(pos_off int64[R + 1], Ltot): the records' offsets on the axis on which their positions follow one another."""
    pos_off = offsets([len(s) for s in seqs])
    Ltot = int(pos_off[-1])
    if Ltot >= 2 ** 31:
        raise ValueError("{} positions in all records: fewer than 2^31 are needed".format(Ltot))
    return pos_off, Ltot


def partner_row(pairs, n):
    """The int32[n] partner row of (v, w) pairs."""
    row = np.full(n, -1, np.int32)
    for v, w in pairs:
        row[v], row[w] = w, v
    return row


def row_pairs(row):
    """Sorted (v, w) pairs, v < w, of a host partner row."""
    v = np.flatnonzero(row > np.arange(len(row)))
    return list(zip(v.tolist(), row[v].tolist()))


def first_fit(candidates):
    """The sequential greedy pass over ranked (v, w) candidates: one joins iff both of its positions are still free.
    [(v, w)] in the order taken."""
    seen, taken = set(), []
    for v, w in candidates:
        if v not in seen and w not in seen:
            seen.add(v)
            seen.add(w)
            taken.append((v, w))
    return taken


def checked_fit(info, rounds):
    """The four result words of a device first fit (status, rounds, pairs, live), read once: RuntimeError unless the pass
    ended clean; its rounds are appended to `rounds` (None: not wanted)."""
    status, nrounds, npairs, live = info.tolist()
    if status or live:
        raise RuntimeError("sq_first_fit_dev: %d candidates still live after %d rounds" % (live, nrounds))
    if rounds is not None:
        rounds.append(nrounds)


def pair_table(partner, cell_off, lengths, width, base=None):
    """The distinct pairs that the consensus rows of a host pair table hold (record r: lengths[r] entries from cell_off[r]
    on): (flat, count, first) int64 -- flat = (base[r] + v) * width + base[r] + w of a pair keyed at its 5' end v, ascending;
    the records that hold it; the first of them.  base None: 0 for every record."""
    keys, recs = [], []
    for r in range(len(lengths)):
        row = partner[cell_off[r]:cell_off[r] + lengths[r]]
        v = np.flatnonzero(row > np.arange(len(row)))
        b = 0 if base is None else base[r]
        keys.append((b + v.astype(np.int64)) * width + b + row[v])
        recs.append(np.full(len(v), r, np.int64))
    keys, recs = np.concatenate(keys), np.concatenate(recs)
    flat, at, count = np.unique(keys, return_index=True, return_counts=True)
    return flat, count, recs[at] if len(at) else np.zeros(0, np.int64)   # (the records come in order: the first occurrence is the first holder)
