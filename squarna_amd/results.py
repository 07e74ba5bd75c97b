"""Decoding of the library's packed result records (sq_result_pack layout, include/squarna_hip.h) and the containers of
Predict's output blocks."""
import copy
import struct

import numpy as np

from .dbn import BRACKETS
from .rows import offsets


_HDR = struct.Struct("<4q")
_MET = struct.Struct("<16d")
_MASK_IDS = [[q for q in range(4) if (m >> q) & 1] for m in range(16)]

#: code points of the bracket characters by signed level (+L opening, -L closing, 0 dot; levels beyond the
#: alphabet print as dots, SQRNdbnseq.py:142-143), indexed by level + _NBR + 1
_NBR = len(BRACKETS)
_LEVEL_CP = np.full(2 * _NBR + 3, ord('.'), np.uint32)
for _l in range(1, _NBR + 1):
    _LEVEL_CP[_NBR + 1 + _l] = ord(BRACKETS[_l - 1][0])
    _LEVEL_CP[_NBR + 1 - _l] = ord(BRACKETS[_l - 1][1])


class TensorResult:
    """What the result classes of the tensor entries share.  ``_TENSORS`` names a class's tensor attributes, ``_NESTED`` its
    attributes that are results themselves (or None)."""
    _TENSORS = ()
    _NESTED = ()

    @property
    def device(self):
        return getattr(self, self._TENSORS[0]).device

    def cpu(self):
        """The same result with every tensor in host memory."""
        new = copy.copy(self)                                        # (host attributes and host caches: carried over as they are)
        for k in self._TENSORS + self._NESTED:
            if getattr(self, k) is not None:
                setattr(new, k, getattr(self, k).cpu())
        return new


class _BlockRun:
    """fold_records(..., _blocks=...) result of one batch whose blocks the library wrote completely."""
    __slots__ = ("blocks",)

    def __init__(self, blocks):
        self.blocks = blocks

    def __len__(self):
        return len(self.blocks)

    def __iter__(self):
        return (("text", t) for t in self.blocks)


class _Blocks:
    """Output blocks of all records of a batch as ONE string + offsets (a list of per-record slices on demand): a caller
    that prints them in order writes the string once."""
    __slots__ = ("text", "off")

    def __init__(self, text, off):
        self.text, self.off = text, off

    def __len__(self):
        return len(self.off) - 1

    def __iter__(self):
        o, t = self.off.tolist(), self.text
        return (t[o[k]:o[k + 1]] for k in range(len(o) - 1))


def unpack_result(p, buf, base=0):
    """(SQRNdbnseq return tuple, reference scores or None) of ONE packed result record (sq_result_pack layout, see
    include/squarna_hip.h) of the prepared record `p`: any rank can decode a record another rank folded."""
    ns, n, has_ref, evals = _HDR.unpack_from(buf, base)
    met = _MET.unpack_from(buf, base + 32)
    o = base + 160
    scores = struct.unpack_from("<%dd" % (3 * ns), buf, o); o += 24 * ns
    masks = struct.unpack_from("<%dQ" % ns, buf, o); o += 8 * ns
    seq = p.seq
    if True:
        lev = np.frombuffer(buf, np.int16, (ns + 1) * n, o).reshape(ns + 1, n)
        # levels -> bracket characters for all rows at once (code-point table), gap columns and separators
        # re-inserted with array assignments (SQRNdbnseq.py:1239-1246)
        cp = _LEVEL_CP[np.clip(lev, -_NBR - 1, _NBR + 1) + (_NBR + 1)]                     # (ns+1, n) uint32
        if p.gapidx or p.sepidx:
            full = np.full((ns + 1, len(seq)), ord('.'), np.uint32)
            keep = np.ones(len(seq), bool)
            keep[p.gapidx] = False
            full[:, keep] = cp
            for i in p.sepidx:
                full[:, i] = ord(seq[i])
            cp = full
        width = cp.shape[1]
        text = cp.tobytes().decode('utf-32-le')
    cons = text[:width]
    preds = []
    for t in range(ns):
        m = masks[t]
        preds.append((text[(t + 1) * width:(t + 2) * width], scores[3 * t:3 * t + 3],
                      list(_MASK_IDS[m]) if m < 16 else [q for q in range(64) if (m >> q) & 1]))
    if has_ref:
        consres = _metrics(met[:6])
        res = _metrics(met[6:12]) + [int(met[12])]
        return (cons, preds, consres, res), tuple(met[13:16])
    return (cons, preds, [np.nan] * 6, [np.nan] * 7), None


def _metrics(m):
    """[TP, FP, FN, FS, PR, RC] with the reference's int/float types: a ratio whose
    denominator is empty is the int 1, everything else a rounded float
    (SQRNdbnseq.py:1256-1258,1273-1275)."""
    tp, fp, fn = int(m[0]), int(m[1]), int(m[2])
    fs = float(m[3]) if 2 * tp + fp + fn else 1
    pr = float(m[4]) if tp + fp else 1
    rc = float(m[5]) if tp + fn else 1
    return [tp, fp, fn, fs, pr, rc]


def _level_partners(lev):
    """Partner arrays of bracket-level rows (int16[rows, n]: +L opens, -L closes a pair of level L) as int32[rows, n],
    -1 unpaired.  The brackets of one level nest, so an opener and its closer are neighbours once the brackets of a row
    are ordered by (depth, position): array code, no per-position loop."""
    out = np.full(lev.shape, -1, np.int32)
    for L in range(1, int(np.abs(lev).max(initial=0)) + 1):
        s = (lev == L).astype(np.int32) - (lev == -L).astype(np.int32)
        rr, pp = np.nonzero(s)
        if not len(rr):
            continue
        depth = np.cumsum(s, axis=1)[rr, pp] + (s[rr, pp] < 0)       # an opener and its closer: the same number
        order = np.lexsort((pp, depth, rr))
        a, b = order[0::2], order[1::2]
        out[rr[a], pp[a]] = pp[b]
        out[rr[b], pp[b]] = pp[a]
    return out


def packed_pair_tables(buf, off):
    """The packed records of a batch (Batch.pack_all) in the layout of sq_result_pairs_dev (include/squarna_hip.h), as
    numpy arrays: what a batch whose ranking tail ran on the host hands to HipEngine.fold_tensors.  A Python loop over the
    records (array code per record and bracket level): the fallback's cost grows with the number of records, unlike the
    device path's."""
    nseq = len(off) - 1
    raw = bytes(buf)
    nstruct, lengths = np.zeros(nseq, np.int64), np.zeros(nseq, np.int64)
    partner, scores, masks = [], [], []
    metrics = np.zeros((nseq, 16), np.float64)
    for k in range(nseq):
        base = int(off[k])
        ns, n, _, _ = _HDR.unpack_from(raw, base)
        nstruct[k], lengths[k] = ns, n
        metrics[k] = _MET.unpack_from(raw, base + 32)
        scores.append(np.frombuffer(raw, '<f8', 3 * ns, base + 160))
        masks.append(np.frombuffer(raw, '<i8', ns, base + 160 + 24 * ns))
        partner.append(_level_partners(np.frombuffer(raw, '<i2', (ns + 1) * n, base + 160 + 32 * ns).reshape(ns + 1, n)).reshape(-1))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros(0, dt)
    return dict(partner=cat(partner, np.int32), scores=cat(scores, np.float64).reshape(-1, 3), pset_mask=cat(masks, np.int64),
                metrics=metrics, row_off=offsets(nstruct), cell_off=offsets((1 + nstruct) * lengths)), nstruct, lengths
