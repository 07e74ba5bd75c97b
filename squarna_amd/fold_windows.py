"""``FoldWindows``: a long sequence folded in overlapping windows, with the windows' consensus formed where the folds are.

Long RNAs are scanned for local structure by folding every window of ~150 nt.  ``FoldWindows`` cuts the windows, sends ALL
windows of ALL input records through ONE ``Fold(records=...)`` call, and turns the windows' consensus rows into a table
of every distinct pair (i, j) of sequence positions: ``count`` -- the windows that predict it --, ``cover`` -- the windows
that contain both positions --, ``first`` -- the first window that predicts it --, ranked by ``freq = count / cover``.  The
consensus at a frequency limit is alignment mode's ``Consensus`` (SQRNdbnali.py:285-295) over that table, with the
frequency relative to the coverage: a first fit down the ranked pairs with ``freq >= limit``.

With the GPU engine no window's row leaves the device: ``sq_window_pair_count`` forms the table from the pair tables
``Fold`` left there, a device sort ranks it, and ONE ``sq_first_fit_dev`` call assembles the consensus of every record on the
axis on which the records follow one another.  An engine without these device methods (the tests' CPU engine) gets the
same object built with numpy.  ``FoldWindows`` prints nothing.
"""
import numpy as np

from . import align as _align
from . import engine as _engine
from . import fold as _fold
from .dbn import GAPS, SEPS, PairsToDBN
from .options import as_freqlimit, derived_inputs
from .results import TensorResult
from .rows import checked_fit, first_fit, offsets, pair_table, partner_row, position_axis, row_pairs

_DEVICE_METHODS = ("fold_tensors", "window_pair_count", "first_fit")


def window_starts(N, window, step):
    """The starts of the windows of a record of N nt: 0, step, 2 step, ... while the window fits, and N - window when the
    last of them does not end at the 3' end; one window at 0 when N <= window."""
    if N <= window:
        return [0]
    starts = list(range(0, N - window + 1, step))
    if (N - window) % step:
        starts.append(N - window)
    return starts


def _rank_order(xp, rec, freq, count, first, flat, nwin):
    """The permutation that puts a table in rank order, record after record: freq descending, count descending, first
    ascending, then i, j ascending (flat ascending).  xp: torch (stable sorts on the tensors' device) or numpy."""
    if xp is np:
        return np.lexsort((flat, first, -count.astype(np.int64), -freq, rec))
    key = (int(nwin) - count.long()) * (int(nwin) + 1) + first.long()        # (count <= nwin, first < nwin: one key for both)
    order = xp.argsort(flat)
    for k, desc in ((key, False), (freq, True), (rec, False)):
        order = order[xp.sort(k[order], descending=desc, stable=True)[1]]
    return order


def _first_fit_host(flat, Ltot):
    """The sequential pass over ranked candidates gi * Ltot + gj on the host: the partner row of the whole axis."""
    v, w = np.divmod(flat, Ltot)
    return partner_row(first_fit(zip(v.tolist(), w.tolist())), Ltot)


class WindowResult(TensorResult):
    """What ``FoldWindows`` computes for R records cut into T windows.

    Host attributes: ``names``, ``sequences``, ``window``, ``step``, ``freqlimit``, ``source`` ("device" or "host": where the
    pair table was formed) and ``first_fit_rounds`` (device path: the rounds of the call's greedy pass).  Torch tensors on
    ``device``: ``pos_off`` int64[R + 1] -- the records' offsets on the axis on which they follow one another --, ``win_off``
    int64[R + 1] -- the offsets of the records' windows --, ``starts`` int64[T] -- every window's start within its record --,
    ``pair_off`` int64[R + 1], ``pair_pos`` int32[P, 2] -- positions i < j within the record --, ``pair_count``,
    ``pair_cover``, ``pair_first`` int32[P] -- the windows of the record whose consensus row pairs i and j, those that
    contain both, and the first holder's index within the record --: record after record, each block in rank order (freq =
    count / cover descending, count descending, first, i, j ascending).  ``consensus`` int32[sum N]: the partner within the
    record, -1 if unpaired, at the call's ``freqlimit``; record r starts at pos_off[r].  ``metrics`` float64[R, 6]: TP FP FN
    FS PR RC of that consensus against the record's reference line, NaN without one.  ``windows``: the :class:`FoldResult`
    of the T windows, named ``name/first-last`` (1-based)."""

    def __init__(self, names, sequences, window, step, freqlimit, source, first_fit_rounds, windows, pos_off, win_off, starts,
                 pair_off, pair_pos, pair_count, pair_cover, pair_first, consensus, metrics):
        self.names, self.sequences, self.window, self.step, self.freqlimit = names, sequences, window, step, freqlimit
        self.source, self.first_fit_rounds, self.windows = source, tuple(first_fit_rounds), windows
        self.pos_off, self.win_off, self.starts, self.pair_off = pos_off, win_off, starts, pair_off
        self.pair_pos, self.pair_count, self.pair_cover, self.pair_first = pair_pos, pair_count, pair_cover, pair_first
        self.consensus, self.metrics = consensus, metrics
        # the host's copy of the sizes: the helpers below index with it
        self._pos_off = offsets([len(s) for s in sequences])
        self._pair_off = None

    _TENSORS = ("pos_off", "win_off", "starts", "pair_off", "pair_pos", "pair_count", "pair_cover", "pair_first", "consensus", "metrics")
    _NESTED = ("windows",)

    def __len__(self):
        return len(self.names)

    def _block(self, r):
        if not 0 <= r < len(self.names):
            raise IndexError("there are %d records" % len(self.names))
        if self._pair_off is None:
            self._pair_off = self.pair_off.cpu().numpy()
        return int(self._pair_off[r]), int(self._pair_off[r + 1])

    def _freq(self, lo=None, hi=None):
        # (divided tensor by tensor: by a Python number the device form multiplies with the reciprocal, which is not
        # count / cover in the last bit -- AlignmentResult.pair_frequency)
        return self.pair_count[lo:hi].double() / self.pair_cover[lo:hi].double()

    def consensus_at(self, freqlimit):
        """The consensus of every record for another frequency limit, from the stored table (no fold): a new tensor in
        ``consensus``'s layout."""
        import torch
        Ltot = int(self._pos_off[-1])
        rec = torch.repeat_interleave(torch.arange(len(self.names), device=self.device), self.pair_off[1:] - self.pair_off[:-1],
                                      output_size=int(self.pair_count.numel()))
        take = self._freq() >= float(freqlimit)
        base = self.pos_off[rec[take]]
        pos = self.pair_pos[take].long()
        flat = (pos[:, 0] + base) * Ltot + pos[:, 1] + base
        eng = _engine.get_engine()
        if flat.is_cuda and hasattr(eng, "first_fit"):
            partner, info = eng.first_fit(flat, Ltot, 0)
            checked_fit(info, None)
        else:
            partner = torch.from_numpy(_first_fit_host(flat.cpu().numpy(), Ltot)).to(self.device)
        return _within_records(torch, partner, self.pos_off)

    def pairs(self, r, freqlimit=None):
        """Sorted (i, j) pairs, i < j, of record r's consensus at the call's limit or at another one."""
        self._block(r)
        row = self.consensus if freqlimit is None else self.consensus_at(freqlimit)
        return row_pairs(row[int(self._pos_off[r]):int(self._pos_off[r + 1])].cpu().numpy())

    def dbn(self, r, freqlimit=None, levellimit=None):
        """Dot-bracket line of record r's consensus (PairsToDBN; levellimit: cut to that many bracket levels)."""
        n = len(self.sequences[r])
        if levellimit is None:
            return PairsToDBN(self.pairs(r, freqlimit), n)
        return PairsToDBN(self.pairs(r, freqlimit), n, levellimit=levellimit)

    def pair_frequency(self, r):
        """float64[N, min(window, N)] band on the tensors' device: band[i, d] is the freq of the pair (i, i + d) of
        record r, 0 elsewhere."""
        import torch
        lo, hi = self._block(r)
        n = len(self.sequences[r])
        band = torch.zeros((n, min(self.window, n)), dtype=torch.float64, device=self.device)
        if hi > lo:
            pos = self.pair_pos[lo:hi].long()
            band[pos[:, 0], pos[:, 1] - pos[:, 0]] = self._freq(lo, hi)
        return band


def _within_records(torch, partner, pos_off):
    """A partner row of the whole axis in the records' own coordinates."""
    lens = pos_off[1:] - pos_off[:-1]
    base = torch.repeat_interleave(pos_off[:-1], lens, output_size=int(partner.numel()))
    return torch.where(partner >= 0, partner.long() - base, torch.full_like(base, -1)).to(torch.int32)


def _host_table(rows, gstart, wlens, wrec, rec_starts, pos_off, win_off, Ltot):
    """(flat, count, cover, first, rec) as numpy arrays from the consensus rows of a host FoldResult, unordered; first
    counts the windows of the whole call, as the kernel does."""
    flat, count, first = pair_table(rows.partner.numpy(), rows._cell_off, wlens, Ltot, gstart)
    rec = wrec[first] if len(first) else np.zeros(0, np.int64)
    cover = np.zeros(len(flat), np.int64)
    for r in np.unique(rec):                                         # the windows with start <= i and j < start + wlen: the starts ascend
        m = rec == r
        i, j = flat[m] // Ltot - pos_off[r], flat[m] % Ltot - pos_off[r]
        s, wl = rec_starts[r], wlens[win_off[r]]
        cover[m] = np.searchsorted(s, i, side="right") - np.searchsorted(s, j - wl, side="right")
    return flat, count, cover, first, rec


def FoldWindows(inputfile=None, inputseq=None, records=None, window=150, step=None, freqlimit=0.35, inputformat="qtrf",
                fileformat="unknown", ignorewarn=False, M=1.8, B=-0.6, **fold_keywords):
    """Fold every input record in overlapping windows and return a :class:`WindowResult`.

    The inputs are ``Fold``'s (``inputfile`` / ``inputseq`` / ``records``, parsed as there).  A record of N nt has one
    window when N <= ``window``; else windows of ``window`` nt start at 0, ``step``, 2 ``step``, ... (default step:
    window // 5, at least 1) and one more ends at the 3' end when the last of them does not.  Every window is the record
    ``(name/first-last, sequence slice, reactivity slice, None, None)``; all windows of all records go through one ``Fold``
    call, to which every other keyword is forwarded unchanged (``configfile``, ``algorithms``, ``rankby``, ``toplim``,
    ``outplim``, ``conslim``, ``poollim``, ``levellimit``, ``priority``, ``maxstemnum``, ``hardrest``, ...; validation and
    messages are ``Fold``'s).  A window's structure is its consensus row.  ``freqlimit``: the limit of the stored
    ``consensus``; ``WindowResult.consensus_at`` forms others without folding.

    Windows across chain breaks or restraint pairs are not defined: a sequence with a gap or separator character and a
    restraint line that is not all '.' raise ValueError, as does ``bpp``.  A reference line is used for the metrics only."""
    import torch
    try:
        ok = int(window) == window and int(window) >= 2
    except Exception:
        ok = False
    if not ok:
        raise ValueError("Inappropriate window value (integer >= 2): {}".format(window))
    window = int(window)
    if step is None:
        step = max(1, window // 5)
    try:
        ok = int(step) == step and 1 <= int(step) <= window
    except Exception:
        ok = False
    if not ok:
        raise ValueError("Inappropriate step value (integer between 1 and window): {}".format(step))
    step = int(step)
    freqlimit = as_freqlimit(freqlimit)
    inputs, kw = derived_inputs("FoldWindows", records, inputfile, inputseq, inputformat, fileformat, ignorewarn, M, B, fold_keywords)

    # ---- the windows
    names, seqs = [rec[0] for rec in inputs], [rec[1] for rec in inputs]
    R = len(inputs)
    (pos_off, Ltot), win_off = position_axis(seqs), np.zeros(R + 1, np.int64)
    wrecs, rec_starts = [], []
    for r, (name, seq, reacts, rests, _) in enumerate(inputs):
        if not seq or any(ch in GAPS or ch in SEPS for ch in seq):
            raise ValueError("FoldWindows: record {} is empty or has a gap or separator character; windows across chain "
                             "breaks are not defined".format(name))
        if rests and set(rests) != {"."}:
            raise ValueError("FoldWindows: record {} has restraints; windows across restraint pairs are not defined".format(name))
        if reacts is not None and len(reacts) and len(reacts) != len(seq):
            raise ValueError("FoldWindows: record {} has {} reactivities for {} positions".format(name, len(reacts), len(seq)))
        wlen = min(window, len(seq))
        s = window_starts(len(seq), window, step)
        rec_starts.append(np.array(s, np.int64))
        win_off[r + 1] = win_off[r] + len(s)
        for a in s:
            wrecs.append((name + "/" + "%d-%d" % (a + 1, a + wlen), seq[a:a + wlen],
                          (list(reacts[a:a + wlen]) or None) if reacts is not None else None, None, None))
    T = int(win_off[-1])
    starts = np.concatenate(rec_starts)
    wrec = np.repeat(np.arange(R), np.diff(win_off))
    gstart = starts + pos_off[wrec]
    wlens = np.minimum(window, np.diff(pos_off))[wrec]

    windows = _fold.Fold(records=wrecs, **kw)
    assert windows._lengths.tolist() == wlens.tolist(), "a window's table does not have its length"

    eng = _engine.get_engine()
    on_device = all(hasattr(eng, m) for m in _DEVICE_METHODS) and windows.partner.is_cuda
    dev = windows.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pos_off, d_win_off = up(pos_off), up(win_off)
    rounds = []
    if on_device:
        flat, count, cover, first = eng.window_pair_count(windows.partner, windows.cell_off, 0, up(gstart), up(wlens.astype(np.int32)), Ltot)
        rec = up(wrec)[first.long()]
        freq = count.double() / cover.double()
        order = _rank_order(torch, rec, freq, count, first, flat, T)
        flat, count, cover, first, rec, freq = (x[order] for x in (flat, count, cover, first, rec, freq))
        partner, info = eng.first_fit(flat[freq >= freqlimit], Ltot, 0)
        checked_fit(info, rounds)
    else:
        flat, count, cover, first, rec = _host_table(windows, gstart, wlens, wrec, rec_starts, pos_off, win_off, Ltot)
        freq = count.astype(np.float64) / cover.astype(np.float64)
        order = _rank_order(np, rec, freq, count, first, flat, T)
        flat, count, cover, first, rec, freq = (x[order] for x in (flat, count, cover, first, rec, freq))
        partner = torch.from_numpy(_first_fit_host(flat[freq >= freqlimit], Ltot))
        flat, count, cover, first, rec = (torch.from_numpy(x) for x in (flat, count, cover, first, rec))
    base = d_pos_off[rec]
    pair_pos = torch.stack((flat // Ltot - base, flat % Ltot - base), 1).to(torch.int32)
    pair_first = (first.long() - d_win_off[rec]).to(torch.int32)
    pair_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    pair_off[1:] = torch.cumsum(torch.bincount(rec, minlength=R), 0)
    consensus = _within_records(torch, partner.to(dev), d_pos_off)

    metrics = np.full((R, 6), np.nan)
    if any(rec[4] for rec in inputs):                                # (O(N) on the host, for the records with a reference line)
        host = consensus.cpu().numpy()
        for r, rec5 in enumerate(inputs):
            if rec5[4]:
                line = PairsToDBN(row_pairs(host[pos_off[r]:pos_off[r + 1]]), len(seqs[r]))
                metrics[r] = [float(x) for x in _align.Metrics(rec5[4], line)]
    return WindowResult(names, seqs, window, step, freqlimit, "device" if on_device else "host", rounds, windows, d_pos_off, d_win_off,
                        up(starts), pair_off, pair_pos, count.to(torch.int32), cover.to(torch.int32), pair_first, consensus, up(metrics))
