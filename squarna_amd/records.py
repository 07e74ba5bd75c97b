"""Host pre-processing of the input records (SQRNdbnseq.py:1001-1037): one record at a time (Prepared) or all rows of an
alignment at once as array code (PackedRows).  numpy and dbn.py only."""
import numpy as np

from .dbn import gap_mask, SEPS, ReactDict, ProcessReacts, DBNToPairs, UnAlign, ParseRestraints


class Prepared:
    """One input record after the host pre-processing of SQRNdbnseq.py:1001-1037."""
    __slots__ = ("seq", "shortseq", "shortrest", "shortreacts", "shortdbn", "rbps", "rxs",
                 "rlefts", "rrights", "gapidx", "sepidx", "plain_reacts", "refpairs")

    _NONE = ([], frozenset())

    def __init__(self, seq, reacts=None, restraints=None, dbn=None):
        seq = seq.upper().replace("T", "U")                          # :1004
        if not reacts and not restraints and not dbn and seq.isalpha():
            # a plain record (letters only: no gap column, no separator; nothing but the sequence given): every field is
            # what the general path below would compute, without its per-record string work -- most records of a big
            # input are like this
            self.seq = self.shortseq = seq
            self.shortrest = None
            self.shortreacts = None                                  # (all 0.5: plain_reacts says so)
            self.plain_reacts = True
            self.gapidx = self.sepidx = self.rbps = self._NONE[0]
            self.rxs = self.rlefts = self.rrights = self._NONE[1]
            self.shortdbn = self.refpairs = None
            return
        if dbn and not reacts and not restraints and seq.isalpha():
            # the same record with a known structure beside it (a benchmark set): what the general path below computes
            # for it, without its string passes (no gap column: UnAlign returns its arguments; no restraint: four empties)
            assert len(seq) == len(dbn)
            n = len(seq)
            self.seq = self.shortseq = seq
            self.shortrest = '.' * n
            self.shortreacts = [0.5] * n
            self.plain_reacts = True
            self.gapidx, self.sepidx, self.rbps = [], [], []
            self.rxs, self.rlefts, self.rrights = set(), set(), set()
            self.shortdbn = dbn
            self.refpairs = None
            return
        if not restraints:
            restraints = '.' * len(seq)                              # :1007-1008
        assert len(seq) == len(restraints), "Invalid restraints given"
        self.plain_reacts = not reacts                               # all 0.5: the batch fills them in one go
        if not reacts:
            reacts = [0.5] * len(seq)                                # :1013-1014
        assert len(reacts) == len(seq), "Invalid reactivities given"
        if type(reacts) == str:                                      # :1019-1020 (default B = 1.6)
            reacts = ProcessReacts([ReactDict[ch] for ch in reacts])
        self.seq = seq
        self.shortseq, self.shortrest, rbps = UnAlign(seq, restraints, want_pairs=True)     # :1023
        if '-' in seq or '.' in seq or '~' in seq:
            gaps = gap_mask(seq)
            self.gapidx = np.flatnonzero(gaps).tolist()
        else:
            gaps, self.gapidx = None, []
        self.sepidx = [i for i, ch in enumerate(seq) if ch in SEPS] if (';' in seq or '&' in seq) else []
        if self.plain_reacts:
            self.shortreacts = [0.5] * len(self.shortseq)
        elif not self.gapidx:
            self.shortreacts = list(reacts)
        else:
            self.shortreacts = np.asarray(reacts, dtype=np.float64)[~gaps].tolist()
        self.shortdbn = None
        self.refpairs = None                                         # pairs of the known structure (Batch._fold_args), formed once
        if dbn:
            assert len(seq) == len(dbn)
            self.shortseq, self.shortdbn = UnAlign(seq, dbn)         # :1026-1028
        self.rbps, self.rxs, self.rlefts, self.rrights = ParseRestraints(self.shortrest, rbps)   # :1037


class PackedRows:
    """The rows of ONE alignment after the host pre-processing of SQRNdbnseq.py:1001-1037 / SQRNdbnali.py:60-86, for all rows at
    once as array code: the alignment is one uint8[rows, columns] array, and letter codes, gap maps, restraint flags and the
    restraint pairs that survive each row's gaps (UnAlign, SQRNdbnseq.py:236-255) come out of it with a handful of numpy
    calls -- what a list of per-row Prepared records holds, in the layout Batch uploads (config 5: 2 x 512 rows of 5,000
    columns were 1.3 s of per-row string work, most of it a character loop over a restraint line whose bracket letters
    leave latin-1 beyond 30 pseudoknot levels).  Rows without reactivities, one restraint line shared by all rows (or none).
    cols: the alignment column of every position, row after row (ReAlignDict, SQRNdbnali.py:20-37)."""
    __slots__ = ("nseq", "seq_off", "codes", "flags", "reacts", "rbp_off", "rbps", "cols", "lengths")

    def __init__(self, seqs, restraint_line=None):
        from .dbn import _CODE_LUT, encode_seq
        R, Lc = len(seqs), len(seqs[0])
        if _CODE_LUT is None:
            encode_seq("A")                                          # (builds the table)
        from .dbn import _CODE_LUT as LUT
        A = np.frombuffer("".join(seqs).encode("latin-1", "replace"), np.uint8).reshape(R, Lc)
        gap_mask("-")                                                # (builds the gap table)
        from .dbn import _GAP_LUT
        keep = ~_GAP_LUT[A]
        self.nseq = R
        self.lengths = keep.sum(axis=1)
        self.seq_off = np.zeros(R + 1, np.int32)
        np.cumsum(self.lengths, out=self.seq_off[1:])
        ltot = int(self.seq_off[-1])
        self.codes = LUT[A[keep]] if ltot else np.zeros(1, np.uint8)
        self.cols = np.ascontiguousarray(np.nonzero(keep)[1], np.int32) if ltot else np.zeros(1, np.int32)
        self.reacts = None
        self.flags = np.zeros(max(ltot, 1), np.uint8)
        self.rbp_off = np.zeros(R + 1, np.int32)
        self.rbps = np.zeros(2, np.int32)
        if restraint_line and restraint_line.count(".") != len(restraint_line):
            assert len(restraint_line) == Lc, "Invalid restraints given"
            cp = np.frombuffer(restraint_line.encode("utf-32-le"), np.uint32)        # code points: any bracket alphabet
            fl = np.zeros(Lc, np.uint8)
            fl[(cp == ord("_")) | (cp == ord("+"))] |= 1             # SQRNdbnseq.py:370-376: unpaired
            fl[cp == ord("/")] |= 2                                  # no pair to the left
            fl[cp == ord("\\")] |= 4                                 # no pair to the right
            if fl.any() and ltot:
                self.flags = np.ascontiguousarray(np.broadcast_to(fl, (R, Lc))[keep])
            pairs = DBNToPairs(restraint_line)                       # once: every row shares the line
            if pairs:
                v = np.fromiter((p[0] for p in pairs), np.int64, len(pairs))
                w = np.fromiter((p[1] for p in pairs), np.int64, len(pairs))
                ok = keep[:, v] & keep[:, w]                         # a pair that touches a gap of the row is dropped (:243-249)
                rank = np.cumsum(keep, axis=1, dtype=np.int32) - 1   # column -> position of the row
                rr, pp = np.nonzero(ok)                              # row-major: every row's pairs in the line's (sorted) order
                rb = np.empty((len(rr), 2), np.int32)
                rb[:, 0] = rank[rr, v[pp]]
                rb[:, 1] = rank[rr, w[pp]]
                np.cumsum(ok.sum(axis=1), out=self.rbp_off[1:])
                if len(rr):
                    self.rbps = rb.reshape(-1)
