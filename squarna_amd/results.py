"""Decoding of the library's packed result records (sq_result_pack layout, include/squarna_hip.h) and the containers of
Predict's output blocks."""
import struct

import numpy as np

from .dbn import BRACKETS


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
