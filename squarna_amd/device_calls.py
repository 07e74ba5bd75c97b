"""The batch-free device entries of libsquarna_hip.so: calls that take the caller's device tensors, enqueue on the current
stream and own no sq_batch -- the select / count / first-fit steps of alignment mode and of sliding windows, and the scoring
of given structures.  HipEngine (engine.py) inherits them; engine.py itself keeps batching and the fold / retry machinery.
"""
import ctypes as C

import numpy as np

from . import _lib
from .rows import offsets

#: the most blocks sq_variant_diff launches, four variants each at a time (SQ_VARIANT_MAX_BLOCKS, csrc/sq_variants.h)
VARIANT_DIFF_MAX_BLOCKS = 2048
#: the most blocks sq_duplex_summary launches, four duplexes each at a time (SQ_DUPLEX_MAX_BLOCKS, csrc/sq_duplex.h)
DUPLEX_SUMMARY_MAX_BLOCKS = 2048
#: sq_covariation_scan's tile of columns, the 64-row words it keeps in LDS at a time and the most blocks it launches
#: (SQ_COV_TILE, SQ_COV_WORD_CHUNK, SQ_COV_MAX_BLOCKS, csrc/sq_covar.h)
COVAR_TILE = 32
COVAR_WORD_CHUNK = 4
COVAR_MAX_BLOCKS = 2048
#: sq_covariation_stat_scan's tile of columns, the 64-row words it keeps in LDS at a time and the most blocks it launches
#: (SQ_COVSTAT_TILE, SQ_COVSTAT_WORD_CHUNK, SQ_COVSTAT_MAX_BLOCKS, csrc/sq_covar_stat.h)
COVAR_STAT_TILE = 32
COVAR_STAT_WORD_CHUNK = 4
COVAR_STAT_MAX_BLOCKS = 2048
#: the statistics and the corrections of sq_covariation_stat_scan / _pairs by name (SQ_COVSTAT_*, csrc/sq_covar_stat.h)
COVAR_STATISTICS = ("mi", "gt", "chi")
COVAR_CORRECTIONS = (None, "apc", "asc")
#: the fixed point of the row weights of sq_covariation_wstat_scan / _pairs, the largest weight and the most rows they take
#: (SQ_COVWSTAT_ONE, SQ_COVWSTAT_MAX_WEIGHT, SQ_COVWSTAT_MAX_ROWS, csrc/sq_covar_wstat.h)
COVAR_WSTAT_ONE = 1 << 20
COVAR_WSTAT_MAX_WEIGHT = 2048.0
COVAR_WSTAT_MAX_ROWS = 1 << 22
#: the most rows sq_covariation_null shuffles on the device and the bins its scan keeps in LDS (SQ_COVNULL_MAX_ROWS,
#: SQ_COVNULL_LDS_BINS, csrc/sq_covar_null.h)
COVAR_NULL_MAX_ROWS = 4096
COVAR_NULL_LDS_BINS = 4096
#: the bytes of shuffled planes covariation_null keeps at a time unless told a batch, and the most samples of a batch
COVAR_NULL_BATCH_BYTES = 256 << 20
COVAR_NULL_BATCH = 64
#: the thresholds and bins sq_covariation_stat_null's scan keeps in LDS (SQ_COVSTATNULL_LDS_BINS, csrc/sq_covar_stat_null.h)
COVAR_STAT_NULL_LDS_BINS = 2048
#: the thresholds and bins sq_covariation_wstat_null's scan keeps in LDS (SQ_COVWSTATNULL_LDS_BINS, csrc/sq_covar_wstat.h)
COVAR_WSTAT_NULL_LDS_BINS = 896
#: sq_row_identity's tile of rows, the 64-column words it keeps in LDS at a time, the most blocks it launches, the most rows
#: and columns it takes and the words of neighbour bits a lane of its filter kernel holds ahead (SQ_ID_TILE, SQ_ID_WORD_CHUNK, SQ_ID_MAX_BLOCKS,
#: SQ_ID_MAX_ROWS, SQ_ID_MAX_COLS, SQ_ID_FILTER_WORDS, csrc/sq_identity.h)
IDENTITY_TILE = 64
IDENTITY_WORD_CHUNK = 4
IDENTITY_MAX_BLOCKS = 2048
IDENTITY_MAX_ROWS = 65535
IDENTITY_MAX_COLS = 1 << 21
IDENTITY_FILTER_WORDS = 64
#: the denominators of sq_row_identity by name (SQ_ID_DEN_*, csrc/sq_identity.h)
IDENTITY_DENOMINATORS = ("shorter", "aligned", "columns")
#: sq_structure_distances' tile of rows, the 64-column words it keeps in LDS at a time, the most blocks it launches, the most
#: rows, columns and planes it takes and the words of neighbour bits a lane of its filter kernel holds ahead (SQ_DIST_TILE,
#: SQ_DIST_WORD_CHUNK, SQ_DIST_MAX_BLOCKS, SQ_DIST_MAX_ROWS, SQ_DIST_MAX_COLS, SQ_DIST_MAX_PLANES, SQ_DIST_FILTER_WORDS,
#: csrc/sq_distances.h)
DISTANCES_TILE = 64
DISTANCES_WORD_CHUNK = 2
DISTANCES_MAX_BLOCKS = 2048
DISTANCES_MAX_ROWS = 65535
DISTANCES_MAX_COLS = 32768
DISTANCES_MAX_PLANES = 16
DISTANCES_FILTER_WORDS = 64
#: the neighbour tests of sq_structure_distances by name (SQ_DIST_RADIUS, SQ_DIST_RELATIVE, csrc/sq_distances.h)
DISTANCES_MODES = ("radius", "relative")
#: sq_project_rows / sq_lift_rows: the threads of a block (one block per alignment row at a time), the most blocks launched,
#: the most columns and rows, the 64-column words of the longest row and the counters of a line (SQ_PROJ_THREADS,
#: SQ_PROJ_MAX_BLOCKS, SQ_PROJ_MAX_COLS, SQ_PROJ_MAX_ROWS, SQ_PROJ_MAX_WORDS, SQ_PROJ_COUNTS, csrc/sq_project.h)
PROJECT_THREADS = 256
PROJECT_MAX_BLOCKS = 2048
PROJECT_MAX_COLS = 32768
PROJECT_MAX_ROWS = 1 << 20
PROJECT_MAX_WORDS = 512
PROJECT_COUNTS = 12
#: the rows (waves) of a block of sq_elements_rows' loops kernel (SQ_ELEM_WAVES, csrc/sq_elements.h)
ELEMENTS_WAVES = 4
#: the stems and the pseudoknot levels of a row beyond which sq_elements_rows leaves it to the host (SQ_CHAIN_TMAX,
#: csrc/sq_device.h; SQ_MAXLEVELS, csrc/sq_internal.h)
ELEMENTS_MAX_STEMS = 11264
ELEMENTS_MAX_LEVELS = 64


def _ptr(t):
    """The address of a device tensor as the C ABI takes it (None: a null pointer)."""
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _stream(device):
    """torch's current stream on `device`, as the C ABI takes it."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _upload_once(arrays, device):
    """The numpy arrays as torch tensors on `device`, through ONE host-to-device copy (every array starts 8-byte aligned)."""
    import torch
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 7) & ~7
    host = np.zeros(max(total, 8), np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    dev = torch.from_numpy(host).to(device)
    return [dev[o:o + a.nbytes].view(getattr(torch, a.dtype.name)).reshape(a.shape) for a, o in zip(arrays, offs)]


def _result_words(out, status_error):
    """The two int64 words an entry leaves in `out`, read once: (records, status).  RuntimeError(status_error) on a status;
    else the records' number."""
    n, status = out.tolist()
    if status:
        raise RuntimeError(status_error)
    return n


def _call_until_fits(device, cap, dtypes, call, status_error):
    """The protocol of the entries that emit a number of records nobody knows beforehand (sq_colmatrix_select,
    sq_window_pair_count): result tensors of `cap` entries, one per dtype (a pair (dtype, n): `cap` rows of n), are allocated
    on `device`; call(tensors, cap, out)
    enqueues the entry, which leaves (records, status) in the two int64 words of `out` -- it counts every record, also those
    beyond cap; the two words are read once.  RuntimeError(status_error) on a status; the call is repeated once, with cap =
    the true number, when that was larger.  Returns the tensors cut to the records' number: only that number comes to the
    host."""
    import torch
    while True:                                                    # result buffers are torch tensors (caller-owned)
        tensors = [torch.empty((cap, dt[1]), dtype=dt[0], device=device) if isinstance(dt, tuple) else torch.empty(cap, dtype=dt, device=device)
                   for dt in dtypes]
        out = torch.zeros(2, dtype=torch.int64, device=device)
        call(tensors, cap, out)
        n = _result_words(out, status_error)
        if n <= cap:
            return tuple(t[:n] for t in tensors)
        cap = n


class DeviceCalls:
    """The engine's batch-free device methods (mixed into HipEngine)."""
    #: score_tensors' table of (k / 2) ** 1.7, kept for the longest record seen (_pow17_table)
    _pow17 = None

    def matrix_select(self, matrix, threshold, minspan=4):
        """Device tensors (flat indices int64, values float64) of the upper cells >= threshold with span >= minspan of a
        device matrix, unordered (sq_colmatrix_select); only the cells' number comes to the host."""
        import torch
        Lcols, dev = int(matrix.shape[0]), matrix.device

        def call(res, cap, out):                                   # (the entry has no status: out[1] stays 0)
            _lib.check(_lib.load().sq_colmatrix_select(_ptr(matrix), Lcols, float(threshold), int(minspan), _ptr(res[0]), _ptr(res[1]),
                                                       cap, _ptr(out), _stream(dev)))

        return _call_until_fits(dev, 1 << 16, (torch.int64, torch.float64), call, None)

    def matrix_cells(self, matrix, threshold, minspan=4, sort=True):
        """(flat indices, values) of the upper cells >= threshold with span >= minspan of a device matrix,
        sorted by flat index unless sort=False (MatrixToDBNs' candidates, SQRNdbnali.py:127-148)."""
        idx, val = self.matrix_select(matrix, threshold, minspan)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        if not sort:
            return idx, val
        order = np.argsort(idx, kind="stable")
        return idx[order], val[order]

    def first_fit(self, flat, Lcols, minspan=0):
        """The greedy pass over ranked candidates on the device (sq_first_fit_dev): flat = int64 device tensor of cells
        v * Lcols + w in rank order; a candidate of span >= minspan joins iff both of its columns are still free
        (MatrixToDBNs' first structure SQRNdbnali.py:127-192 with minspan 4, Consensus :285-295 with none).  Returns
        (partner int32[Lcols] on the device, -1 where free; info int32[4] on the device: status, rounds, pairs, live).
        Enqueued on the current stream; nothing is waited for."""
        import torch
        flat = flat.contiguous()
        assert flat.dtype == torch.int64 and flat.is_cuda and flat.dim() == 1
        L = _lib.load()
        n, dev = int(flat.numel()), flat.device
        with torch.cuda.device(dev):
            nbytes = int(L.sq_first_fit_scratch(n, int(Lcols)))
            scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
            partner = torch.empty(int(Lcols), dtype=torch.int32, device=dev)
            info = torch.empty(4, dtype=torch.int32, device=dev)
            _lib.check(L.sq_first_fit_dev(_ptr(flat if n else None), n, int(Lcols), int(minspan), _ptr(partner), _ptr(scratch), nbytes,
                                          _ptr(info), _stream(dev)))
        return partner, info

    def align_pair_count(self, partner, cell_off, gap_maps, Lcols, threshold=1):
        """Consensus' dict on the device (sq_align_pair_count): partner / cell_off = the pair tables of fold_tensors (gap-free
        coordinates), gap_maps = per record the int32 array of its positions' alignment columns.  Returns the device
        tensors (flat int64 = v * Lcols + w, count int32, first int32) of the distinct column pairs that at least
        `threshold` records' consensus rows hold, unordered; only their number comes to the host."""
        import torch
        L = _lib.load()
        dev, nrec = partner.device, len(gap_maps)
        col_off = np.zeros(nrec + 1, np.int32)
        np.cumsum([len(g) for g in gap_maps], out=col_off[1:])
        cols = np.concatenate(gap_maps).astype(np.int32) if nrec else np.zeros(0, np.int32)
        assert int(cell_off.numel()) == nrec + 1
        cap = max(int(col_off[-1]) // 2, 1)                          # (a record of n positions holds at most n / 2 pairs)
        with torch.cuda.device(dev):
            if not partner.numel():                                  # (every row all gaps: no table, no pair)
                return tuple(torch.empty(0, dtype=dt, device=dev) for dt in (torch.int64, torch.int32, torch.int32))
            d_off, d_cols = _upload_once([col_off, cols if len(cols) else np.zeros(1, np.int32)], dev)
            nbytes = int(L.sq_align_pair_count_scratch(int(Lcols)))
            scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
            flat = torch.empty(cap, dtype=torch.int64, device=dev)
            count = torch.empty(cap, dtype=torch.int32, device=dev)
            first = torch.empty(cap, dtype=torch.int32, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_align_pair_count(_ptr(partner), _ptr(cell_off), _ptr(d_off), _ptr(d_cols), nrec, int(Lcols), int(threshold),
                                             _ptr(scratch), nbytes, _ptr(flat), _ptr(count), _ptr(first), cap, _ptr(out), _stream(dev)))
            n = _result_words(out, "sq_align_pair_count: a pair table entry lies outside its record or the %d columns" % Lcols)
        assert n <= cap
        return flat[:n], count[:n], first[:n]

    def window_pair_count(self, partner, cell_off, rec0, starts, lens, Ltot, cap=None):
        """The pair table of sliding windows on the device (sq_window_pair_count): partner / cell_off = pair tables in
        fold_tensors' layout, window k = record rec0 + k (its consensus row, in the window's own coordinates); starts int64
        (non-decreasing, on the axis of Ltot positions on which the records follow one another) and lens int32: device
        tensors.  Returns the device tensors (flat int64 = gi * Ltot + gj, count, cover, first int32) of the distinct
        pairs, unordered.  `cap` (default 1 << 16) sizes the result buffers; the call is repeated with the true number when
        it was too small (matrix_select's protocol).  Only that number comes to the host."""
        import torch
        L = _lib.load()
        dev, nwin = partner.device, int(starts.numel())
        assert starts.dtype == torch.int64 and lens.dtype == torch.int32 and int(lens.numel()) == nwin
        assert partner.dtype == torch.int32 and cell_off.dtype == torch.int64 and int(cell_off.numel()) >= int(rec0) + nwin + 1
        starts, lens = starts.contiguous(), lens.contiguous()
        cap = 1 << 16 if cap is None else int(cap)

        def call(res, cap, out):
            _lib.check(L.sq_window_pair_count(_ptr(partner), _ptr(cell_off), int(rec0), nwin, _ptr(starts), _ptr(lens), int(Ltot),
                                              _ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(res[3]), cap, _ptr(out), _stream(dev)))

        with torch.cuda.device(dev):
            return _call_until_fits(dev, cap, (torch.int64, torch.int32, torch.int32, torch.int32), call,
                                    "sq_window_pair_count: a pair table entry is not a pair inside its window, or a window "
                                    "lies outside the %d positions or its table" % Ltot)

    def variant_diff(self, partner, cell_off, lengths, rec0, wt_rec, pos_off, Ltot):
        """What substitution variants change against their wild types, on the device (sq_variant_diff): partner / cell_off /
        lengths = pair tables in fold_tensors' layout, variant m = record rec0 + m, its wild type = record wt_rec[m] < rec0 of
        the same length (both at their consensus rows); wt_rec int32 and pos_off int64 (where a record's positions start on
        the axis of Ltot positions, at least rec0 entries): device tensors.  Returns the device tensors (diff int32[V, 6] =
        lost, gained, kept, changed, first, last per variant; pos_changed int32[Ltot] = per wild-type position the variants
        that changed its partner).  Only the two result words come to the host."""
        import torch
        dev, nvar = partner.device, int(wt_rec.numel())
        assert partner.dtype == torch.int32 and cell_off.dtype == torch.int64 and lengths.dtype == torch.int64
        assert wt_rec.dtype == torch.int32 and pos_off.dtype == torch.int64 and int(pos_off.numel()) >= int(rec0)
        assert int(cell_off.numel()) >= int(rec0) + nvar + 1 and int(lengths.numel()) >= int(rec0) + nvar
        lengths, wt_rec, pos_off = lengths.contiguous(), wt_rec.contiguous(), pos_off.contiguous()
        with torch.cuda.device(dev):
            diff = torch.empty((nvar, 6), dtype=torch.int32, device=dev)
            pos_changed = torch.empty(int(Ltot), dtype=torch.int32, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(_lib.load().sq_variant_diff(_ptr(partner), _ptr(cell_off), _ptr(lengths), int(rec0), nvar, _ptr(wt_rec), _ptr(pos_off),
                                                   int(Ltot), _ptr(diff), _ptr(pos_changed), _ptr(out), _stream(dev)))
            _result_words(out, "sq_variant_diff: a variant and its wild type differ in length or lie outside their tables or the %d "
                               "positions, or a pair table entry is not a pair inside its row" % Ltot)
        return diff, pos_changed

    def duplex_summary(self, partner_s, cell_off_s, lengths_s, partner_d, cell_off_d, lengths_d, a_rec, b_rec, pos_off, Ltot):
        """What two chains do to one another, on the device (sq_duplex_summary): partner_s / cell_off_s / lengths_s = the pair
        tables of the records folded alone, partner_d / cell_off_d / lengths_d = those of the duplex records, both in
        fold_tensors' layout and possibly views of one allocation; duplex k = the chain of solo record a_rec[k], a separator
        column and the chain of solo record b_rec[k] (all three at their consensus rows); a_rec / b_rec int32 and pos_off
        int64 (where a solo record's positions start on the axis of Ltot positions, one entry more than there are solo
        records): device tensors.  The duplex tables may be None when there is no duplex.  Returns the device tensors
        (summary int32[P, 9] = inter, intra_a, intra_b, lost_a, lost_b, a_first, a_last, b_first, b_last per duplex; bound
        int32[Ltot] = per solo position the duplexes in which it pairs across the separator).  Only the two result words come
        to the host."""
        import torch
        dev, nsolo, ndup = partner_s.device, int(lengths_s.numel()), int(a_rec.numel())
        assert partner_s.dtype == torch.int32 and cell_off_s.dtype == torch.int64 and lengths_s.dtype == torch.int64
        assert a_rec.dtype == torch.int32 and b_rec.dtype == torch.int32 and int(b_rec.numel()) == ndup
        assert pos_off.dtype == torch.int64 and int(pos_off.numel()) >= nsolo + 1 and int(cell_off_s.numel()) >= nsolo + 1
        if ndup:
            assert partner_d.dtype == torch.int32 and cell_off_d.dtype == torch.int64 and lengths_d.dtype == torch.int64
            assert int(cell_off_d.numel()) >= ndup + 1 and int(lengths_d.numel()) >= ndup
            cell_off_d, lengths_d = cell_off_d.contiguous(), lengths_d.contiguous()
        cell_off_s, lengths_s, a_rec, b_rec, pos_off = (t.contiguous() for t in (cell_off_s, lengths_s, a_rec, b_rec, pos_off))
        with torch.cuda.device(dev):
            summary = torch.empty((ndup, 9), dtype=torch.int32, device=dev)
            bound = torch.empty(int(Ltot), dtype=torch.int32, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(_lib.load().sq_duplex_summary(_ptr(partner_s), _ptr(cell_off_s), _ptr(lengths_s), nsolo,
                                                     _ptr(partner_d if ndup else None), _ptr(cell_off_d if ndup else None),
                                                     _ptr(lengths_d if ndup else None), ndup, _ptr(a_rec), _ptr(b_rec), _ptr(pos_off),
                                                     int(Ltot), _ptr(summary), _ptr(bound), _ptr(out), _stream(dev)))
            _result_words(out, "sq_duplex_summary: a duplex does not consist of its two chains and a separator column, a row lies "
                               "outside its table or the %d positions, or a pair table entry is not a pair inside its row" % Ltot)
        return summary, bound

    def covariation_scan(self, rows, minspan=4, min_rows=1, min_cov=1, cap=None):
        """Covariation evidence for every pair of columns of an alignment, on the device (sq_covariation_scan): rows = uint8
        device tensor [R, L] of the rows' ASCII bytes.  Returns the device tensors (flat int64 = v * L + w, counts int32[P, 7] =
        the rows of the pair types AU UA GC CG GU UG and the rows with a gap in both columns, cov int64[P]) of the cells
        with w - v >= minspan, at least min_rows rows that hold a canonical pair and cov >= min_cov, unordered.  `cap`
        (default 1 << 16) sizes the result buffers; the call is repeated with the true number when it was too small
        (matrix_select's protocol).  Only that number comes to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        dev, R, Lcols = rows.device, int(rows.shape[0]), int(rows.shape[1])
        cap = 1 << 16 if cap is None else int(cap)

        def call(res, cap, out):                                   # (the entry has no status: out[1] stays 0)
            _lib.check(L.sq_covariation_scan(_ptr(rows), R, Lcols, int(minspan), int(min_rows), int(min_cov), _ptr(scratch), nbytes,
                                             _ptr(res[0]), _ptr(res[1]), _ptr(res[2]), cap, _ptr(out), _stream(dev)))

        with torch.cuda.device(dev):
            nbytes = int(L.sq_covariation_scratch(R, Lcols))
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            return _call_until_fits(dev, cap, (torch.int64, (torch.int32, 7), torch.int64), call, None)

    def covariation_pairs(self, rows, pairs):
        """The same numbers for given column pairs (sq_covariation_pairs): pairs = int32 device tensor [P, 2] of (v, w),
        0 <= v < w < L.  Returns the device tensors (counts int32[P, 7], cov int64[P]) in the pairs' order; RuntimeError when
        a pair is not such a pair.  Only the two result words come to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        assert pairs.dtype == torch.int32 and pairs.dim() == 2 and int(pairs.shape[1]) == 2 and pairs.device == rows.device
        dev, R, Lcols, P = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(pairs.shape[0])
        pairs = pairs.contiguous()
        with torch.cuda.device(dev):
            nbytes = int(L.sq_covariation_scratch(R, Lcols))
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            counts = torch.empty((P, 7), dtype=torch.int32, device=dev)
            cov = torch.empty(P, dtype=torch.int64, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_covariation_pairs(_ptr(rows), R, Lcols, _ptr(pairs if P else None), P, _ptr(scratch), nbytes,
                                              _ptr(counts if P else None), _ptr(cov if P else None), _ptr(out), _stream(dev)))
            _result_words(out, "sq_covariation_pairs: a pair is not 0 <= v < w < %d columns" % Lcols)
        return counts, cov

    def _covariation_stat_buffers(self, rows, statistic, correction):
        """What covariation_stat_scan and covariation_stat_pairs share: (stat, corr, scratch, its bytes, mean or None)."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        stat, corr = COVAR_STATISTICS.index(statistic), COVAR_CORRECTIONS.index(correction)
        R, Lcols = int(rows.shape[0]), int(rows.shape[1])
        nbytes = int(L.sq_covariation_stat_scratch(R, Lcols))
        scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=rows.device)
        mean = torch.empty(Lcols + 1, dtype=torch.float64, device=rows.device) if corr else None
        return stat, corr, scratch, nbytes, mean

    def covariation_stat_scan(self, rows, statistic="gt", correction="apc", minspan=4, min_rows=1, min_stat=None, cap=None):
        """Covariation statistics of every pair of columns of an alignment, on the device (sq_covariation_stat_scan): rows = uint8
        device tensor [R, L] of the rows' ASCII bytes, statistic one of COVAR_STATISTICS, correction one of COVAR_CORRECTIONS.
        Returns the device tensors (flat int64 = v * L + w, joint int32[P, 16] = the rows with residue a at v and b at w at
        [a * 4 + b], a and b in A C G U, raw float64[P] = S, value float64[P] = the corrected C, mean float64[L + 1] = the
        column means of S and, last, the mean of all cells; None without a correction) of the cells with w - v >= minspan, at
        least min_rows rows in the table and C >= min_stat (None: every C), unordered.  `cap` (default 1 << 16) sizes the result
        buffers; the call is repeated with the true number when it was too small (matrix_select's protocol).  Only that
        number comes to the host."""
        import torch
        L = _lib.load()
        dev, R, Lcols = rows.device, int(rows.shape[0]), int(rows.shape[1])
        cap = 1 << 16 if cap is None else int(cap)
        floor = float("-inf") if min_stat is None else float(min_stat)

        def call(res, cap, out):                                   # (the entry has no status: out[1] stays 0)
            _lib.check(L.sq_covariation_stat_scan(_ptr(rows), R, Lcols, stat, corr, int(minspan), int(min_rows), floor, _ptr(scratch), nbytes,
                                                  _ptr(mean), _ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(res[3]), cap, _ptr(out),
                                                  _stream(dev)))

        with torch.cuda.device(dev):
            stat, corr, scratch, nbytes, mean = self._covariation_stat_buffers(rows, statistic, correction)
            return _call_until_fits(dev, cap, (torch.int64, (torch.int32, 16), torch.float64, torch.float64), call, None) + (mean,)

    def covariation_stat_pairs(self, rows, pairs, statistic="gt", correction="apc"):
        """The same numbers for given column pairs (sq_covariation_stat_pairs): pairs = int32 device tensor [P, 2] of (v, w),
        0 <= v < w < L.  Returns the device tensors (joint int32[P, 16], raw float64[P], value float64[P], mean float64[L + 1] or
        None) in the pairs' order; RuntimeError when a pair is not such a pair.  Only the two result words come to the host."""
        import torch
        L = _lib.load()
        assert pairs.dtype == torch.int32 and pairs.dim() == 2 and int(pairs.shape[1]) == 2 and pairs.device == rows.device
        dev, R, Lcols, P = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(pairs.shape[0])
        pairs = pairs.contiguous()
        with torch.cuda.device(dev):
            stat, corr, scratch, nbytes, mean = self._covariation_stat_buffers(rows, statistic, correction)
            joint = torch.empty((P, 16), dtype=torch.int32, device=dev)
            raw, value = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_covariation_stat_pairs(_ptr(rows), R, Lcols, stat, corr, _ptr(pairs if P else None), P, _ptr(scratch), nbytes,
                                                   _ptr(mean), _ptr(joint if P else None), _ptr(raw if P else None),
                                                   _ptr(value if P else None), _ptr(out), _stream(dev)))
            _result_words(out, "sq_covariation_stat_pairs: a pair is not 0 <= v < w < %d columns" % Lcols)
        return joint, raw, value, mean

    def _covariation_wstat_buffers(self, rows, weights, statistic, correction):
        """What covariation_wstat_scan and covariation_wstat_pairs share: (stat, corr, scratch, its bytes, mean or None)."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        R, Lcols = int(rows.shape[0]), int(rows.shape[1])
        assert weights.dtype == torch.float64 and weights.device == rows.device and tuple(weights.shape) == (R,) and weights.is_contiguous()
        stat, corr = COVAR_STATISTICS.index(statistic), COVAR_CORRECTIONS.index(correction)
        nbytes = int(L.sq_covariation_wstat_scratch(R, Lcols))
        scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=rows.device)
        mean = torch.empty(Lcols + 1, dtype=torch.float64, device=rows.device) if corr else None
        return stat, corr, scratch, nbytes, mean

    def covariation_wstat_scan(self, rows, weights, statistic="gt", correction="apc", minspan=4, min_rows=1.0, min_stat=None, cap=None):
        """covariation_stat_scan with a weight per row (sq_covariation_wstat_scan): weights = float64 device tensor [R], each
        finite and in 0 .. 2048 (RuntimeError otherwise), quantised to multiples of 1 / COVAR_WSTAT_ONE.  Returns the device
        tensors (flat int64, joint int64[P, 16] = Q, the sums of the quantised weights of the rows of each cell: the weighted
        counts times COVAR_WSTAT_ONE, raw, value, mean) as covariation_stat_scan does; min_rows is a float and compared with the
        weighted rows of a cell, the sum of Q / COVAR_WSTAT_ONE."""
        import torch
        L = _lib.load()
        dev, R, Lcols = rows.device, int(rows.shape[0]), int(rows.shape[1])
        cap = 1 << 16 if cap is None else int(cap)
        floor = float("-inf") if min_stat is None else float(min_stat)

        def call(res, cap, out):
            _lib.check(L.sq_covariation_wstat_scan(_ptr(rows), R, Lcols, _ptr(weights), stat, corr, int(minspan), float(min_rows), floor,
                                                   _ptr(scratch), nbytes, _ptr(mean), _ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(res[3]), cap,
                                                   _ptr(out), _stream(dev)))

        with torch.cuda.device(dev):
            stat, corr, scratch, nbytes, mean = self._covariation_wstat_buffers(rows, weights, statistic, correction)
            return _call_until_fits(dev, cap, (torch.int64, (torch.int64, 16), torch.float64, torch.float64), call,
                                    "sq_covariation_wstat_scan: a weight is not a finite number in 0 .. 2048") + (mean,)

    def covariation_wstat_pairs(self, rows, weights, pairs, statistic="gt", correction="apc"):
        """covariation_stat_pairs with a weight per row (sq_covariation_wstat_pairs; the weights and Q as covariation_wstat_scan
        has them).  Returns the device tensors (joint int64[P, 16] = Q, raw float64[P], value float64[P], mean float64[L + 1] or
        None) in the pairs' order; RuntimeError for a bad weight or a bad pair.  Only the two result words come to the host."""
        import torch
        L = _lib.load()
        assert pairs.dtype == torch.int32 and pairs.dim() == 2 and int(pairs.shape[1]) == 2 and pairs.device == rows.device
        dev, R, Lcols, P = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(pairs.shape[0])
        pairs = pairs.contiguous()
        with torch.cuda.device(dev):
            stat, corr, scratch, nbytes, mean = self._covariation_wstat_buffers(rows, weights, statistic, correction)
            joint = torch.empty((P, 16), dtype=torch.int64, device=dev)
            raw, value = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.float64, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_covariation_wstat_pairs(_ptr(rows), R, Lcols, _ptr(weights), stat, corr, _ptr(pairs if P else None), P,
                                                    _ptr(scratch), nbytes, _ptr(mean), _ptr(joint if P else None), _ptr(raw if P else None),
                                                    _ptr(value if P else None), _ptr(out), _stream(dev)))
            status = out.tolist()[1]
            if status == 3:
                raise RuntimeError("sq_covariation_wstat_pairs: a weight is not a finite number in 0 .. 2048")
            if status:
                raise RuntimeError("sq_covariation_wstat_pairs: a pair is not 0 <= v < w < %d columns" % Lcols)
        return joint, raw, value, mean

    def covariation_null_planes(self, rows, k, seed, count=None):
        """The bit planes of sample k of the shuffled-column null of an alignment (sq_covariation_null_planes): rows = uint8
        device tensor [R, L]; returns the int64 device tensor [5, ceil(R / 64), L rounded up to 64] of the planes A, C, G, U, gap
        (csrc/sq_covar.h has the layout, csrc/sq_covar_null.h the shuffle).  With `count`: the samples k .. k + count - 1 from one
        launch, as [count, 5, ceil(R / 64), L rounded up to 64]."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        dev, R, Lcols, many = rows.device, int(rows.shape[0]), int(rows.shape[1]), 1 if count is None else int(count)
        words, lpad = (R + 63) // 64, (Lcols + 63) // 64 * 64
        with torch.cuda.device(dev):
            nbytes = int(L.sq_covariation_null_scratch(R, Lcols, many))
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            _lib.check(L.sq_covariation_null_planes(_ptr(rows), R, Lcols, int(k), many, int(seed), _ptr(scratch), nbytes, _stream(dev)))
        planes = scratch[:many * 5 * words * lpad].view(many, 5, words, lpad)
        return planes[0] if count is None else planes

    def covariation_null(self, rows, pairs, cov, minspan=4, samples=100, seed=0, batch=None):
        """The shuffled-column null of cov for observed pairs (sq_covariation_null): rows = uint8 device tensor [R, L], pairs =
        int32 device tensor [P, 2], cov = int64 device tensor [P] (their observed values).  Returns the device tensors
        (null_ge int64[P] = the null cells of all samples with cov >= cov[p], own_ge int32[P] = the samples in which the same
        cell reaches cov[p], null_max int64[samples]).  `batch` samples are formed at a time (default: as many as
        COVAR_NULL_BATCH_BYTES of planes hold, at most COVAR_NULL_BATCH); the results do not depend on it.  RuntimeError when a
        pair is not 0 <= v < w < L.  Only the two result words come to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        assert pairs.dtype == torch.int32 and pairs.dim() == 2 and int(pairs.shape[1]) == 2 and pairs.device == rows.device
        assert cov.dtype == torch.int64 and cov.dim() == 1 and cov.device == rows.device and int(cov.numel()) == int(pairs.shape[0])
        dev, R, Lcols, P, K = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(pairs.shape[0]), int(samples)
        pairs, cov = pairs.contiguous(), cov.contiguous()
        if batch is None:
            per = 5 * ((R + 63) // 64) * ((Lcols + 63) // 64 * 64) * 8
            batch = max(1, min(K, COVAR_NULL_BATCH, COVAR_NULL_BATCH_BYTES // per))
        batch = int(batch)
        with torch.cuda.device(dev):
            thresholds = torch.unique(cov)                           # (sorted)
            U = int(thresholds.numel())
            nbytes = int(L.sq_covariation_null_scratch(R, Lcols, batch))
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            hist = torch.empty(U + 1, dtype=torch.int64, device=dev)
            own_ge = torch.empty(P, dtype=torch.int32, device=dev)
            null_max = torch.empty(K, dtype=torch.int64, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_covariation_null(_ptr(rows), R, Lcols, int(minspan), _ptr(pairs if P else None), _ptr(cov if P else None), P,
                                             _ptr(thresholds if U else None), U, K, int(seed), batch, _ptr(scratch), nbytes, _ptr(hist),
                                             _ptr(own_ge if P else None), _ptr(null_max), _ptr(out), _stream(dev)))
            _result_words(out, "sq_covariation_null: a pair is not 0 <= v < w < %d columns" % Lcols)
            # hist[b] = the null cells with exactly b thresholds <= their cov: cov[p], the t-th threshold, is reached by the bins
            # from t + 1 on
            from_bin = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
            null_ge = from_bin[torch.searchsorted(thresholds, cov) + 1] if P else torch.empty(0, dtype=torch.int64, device=dev)
        return null_ge, own_ge, null_max

    def covariation_stat_null(self, rows, pairs, value, statistic="gt", correction="apc", minspan=4, samples=100, seed=0, batch=None):
        """The shuffled-column null of a covariation statistic for observed pairs (sq_covariation_stat_null): rows = uint8 device
        tensor [R, L], pairs = int32 device tensor [P, 2], value = float64 device tensor [P] (their observed C, no NaN),
        statistic one of COVAR_STATISTICS, correction one of COVAR_CORRECTIONS.  Returns the device tensors (null_ge int64[P] =
        the null cells of all samples with C >= value[p], own_ge int32[P] = the samples in which the same cell reaches value[p],
        null_max float64[samples], -inf for a sample without a cell in scope).  `batch` samples are formed at a time (default: as
        many as COVAR_NULL_BATCH_BYTES of planes and partial column sums hold, at most COVAR_NULL_BATCH); the results do not
        depend on it.  RuntimeError when a pair is not 0 <= v < w < L.  Only the two result words come to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        assert pairs.dtype == torch.int32 and pairs.dim() == 2 and int(pairs.shape[1]) == 2 and pairs.device == rows.device
        assert value.dtype == torch.float64 and value.dim() == 1 and value.device == rows.device and int(value.numel()) == int(pairs.shape[0])
        stat, corr = COVAR_STATISTICS.index(statistic), COVAR_CORRECTIONS.index(correction)
        dev, R, Lcols, P, K = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(pairs.shape[0]), int(samples)
        pairs, value = pairs.contiguous(), value.contiguous()
        if batch is None:
            per = int(L.sq_covariation_stat_null_scratch(R, Lcols, 2)) - int(L.sq_covariation_stat_null_scratch(R, Lcols, 1))
            batch = max(1, min(K, COVAR_NULL_BATCH, COVAR_NULL_BATCH_BYTES // max(per, 1)))
        batch = int(batch)
        with torch.cuda.device(dev):
            thresholds = torch.unique(value)                         # (sorted; -0.0 and 0.0 are one value)
            U = int(thresholds.numel())
            nbytes = int(L.sq_covariation_stat_null_scratch(R, Lcols, batch))
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            hist = torch.empty(U + 1, dtype=torch.int64, device=dev)
            own_ge = torch.empty(P, dtype=torch.int32, device=dev)
            null_max = torch.empty(K, dtype=torch.float64, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_covariation_stat_null(_ptr(rows), R, Lcols, stat, corr, int(minspan), _ptr(pairs if P else None),
                                                  _ptr(value if P else None), P, _ptr(thresholds if U else None), U, K, int(seed), batch,
                                                  _ptr(scratch), nbytes, _ptr(hist), _ptr(own_ge if P else None), _ptr(null_max), _ptr(out),
                                                  _stream(dev)))
            _result_words(out, "sq_covariation_stat_null: a pair is not 0 <= v < w < %d columns" % Lcols)
            # hist[b] = the null cells with exactly b thresholds <= their C: value[p], the t-th threshold, is reached by the bins
            # from t + 1 on
            from_bin = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
            null_ge = from_bin[torch.searchsorted(thresholds, value) + 1] if P else torch.empty(0, dtype=torch.int64, device=dev)
        return null_ge, own_ge, null_max

    def covariation_wstat_null(self, rows, weights, pairs, value, statistic="gt", correction="apc", minspan=4, samples=100, seed=0,
                               batch=None):
        """covariation_stat_null with a weight per row (sq_covariation_wstat_null): weights = float64 device tensor [R] as
        covariation_wstat_scan takes them, value = the observed C of the weighted statistics.  Row r of every shuffled sample
        keeps weights[r]: a null cell's value is what covariation_wstat_scan gives for the shuffled rows and the same weights.
        Returns the device tensors (null_ge int64[P], own_ge int32[P], null_max float64[samples]) as covariation_stat_null does;
        `batch` is chosen as there and the results do not depend on it.  RuntimeError for a bad weight or a bad pair.  Only the
        two result words come to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        assert pairs.dtype == torch.int32 and pairs.dim() == 2 and int(pairs.shape[1]) == 2 and pairs.device == rows.device
        assert value.dtype == torch.float64 and value.dim() == 1 and value.device == rows.device and int(value.numel()) == int(pairs.shape[0])
        stat, corr = COVAR_STATISTICS.index(statistic), COVAR_CORRECTIONS.index(correction)
        dev, R, Lcols, P, K = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(pairs.shape[0]), int(samples)
        assert weights.dtype == torch.float64 and weights.device == dev and tuple(weights.shape) == (R,) and weights.is_contiguous()
        pairs, value = pairs.contiguous(), value.contiguous()
        if batch is None:
            per = int(L.sq_covariation_wstat_null_scratch(R, Lcols, 2)) - int(L.sq_covariation_wstat_null_scratch(R, Lcols, 1))
            batch = max(1, min(K, COVAR_NULL_BATCH, COVAR_NULL_BATCH_BYTES // max(per, 1)))
        batch = int(batch)
        with torch.cuda.device(dev):
            thresholds = torch.unique(value)                         # (sorted; -0.0 and 0.0 are one value)
            U = int(thresholds.numel())
            nbytes = int(L.sq_covariation_wstat_null_scratch(R, Lcols, batch))
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
            hist = torch.empty(U + 1, dtype=torch.int64, device=dev)
            own_ge = torch.empty(P, dtype=torch.int32, device=dev)
            null_max = torch.empty(K, dtype=torch.float64, device=dev)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_covariation_wstat_null(_ptr(rows), R, Lcols, stat, corr, int(minspan), _ptr(pairs if P else None),
                                                   _ptr(value if P else None), P, _ptr(thresholds if U else None), U, K, int(seed), batch,
                                                   _ptr(scratch), nbytes, _ptr(hist), _ptr(own_ge if P else None), _ptr(null_max), _ptr(out),
                                                   _stream(dev), _ptr(weights)))
            status = out.tolist()[1]
            if status == 3:
                raise RuntimeError("sq_covariation_wstat_null: a weight is not a finite number in 0 .. 2048")
            if status:
                raise RuntimeError("sq_covariation_wstat_null: a pair is not 0 <= v < w < %d columns" % Lcols)
            # (hist and null_ge: as covariation_stat_null)
            from_bin = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
            null_ge = from_bin[torch.searchsorted(thresholds, value) + 1] if P else torch.empty(0, dtype=torch.int64, device=dev)
        return null_ge, own_ge, null_max

    def row_identity(self, rows, denominator=0, threshold_bp=8000, matrix=True):
        """Row identities, neighbour counts and the greedy redundancy filter of an alignment, on the device (sq_row_identity):
        rows = uint8 device tensor [R, L] of the rows' ASCII bytes, denominator = 0 / 1 / 2 (IDENTITY_DENOMINATORS: the
        shorter row's residues, the columns where both hold a residue, L), threshold_bp = the neighbour threshold in basis
        points.  Returns a dict of device tensors: len, bases, neighbours int32[R], keep bool[R] and, with `matrix`, same and
        both int32[R, R] (else None: then nothing of size R x R is written).  Only the two result words come to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        dev, R, Lcols = rows.device, int(rows.shape[0]), int(rows.shape[1])
        with torch.cuda.device(dev):
            nbytes = int(L.sq_row_identity_scratch(R, Lcols))
            scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            res = dict(len=new(R, torch.int32), bases=new(R, torch.int32), neighbours=new(R, torch.int32), keep=new(R, torch.uint8),
                       same=new((R, R), torch.int32) if matrix else None, both=new((R, R), torch.int32) if matrix else None)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_row_identity(_ptr(rows), R, Lcols, int(denominator), int(threshold_bp), _ptr(scratch), nbytes, _ptr(res["len"]),
                                         _ptr(res["bases"]), _ptr(res["same"]), _ptr(res["both"]), _ptr(res["neighbours"]),
                                         _ptr(res["keep"]), _ptr(out), _stream(dev)))
            _result_words(out, "sq_row_identity: status")            # (the entry has no status: out[1] stays 0)
        res["keep"] = res["keep"].bool()
        return res

    def structure_distances(self, partner, row_start, row_width, group_off, tiles, mode=0, threshold=0, matrix=True):
        """Base-pair distances, neighbour counts and the greedy filter of structure rows, on the device
        (sq_structure_distances): partner = a flat int32 CUDA tensor of partner rows, read where it is; the small tables are
        host arrays and go up in one copy: row_start / row_width = per row where it starts in partner and its columns,
        group_off [G + 1] = the groups' first rows (from 0 to S), tiles [T, 2] = the planned tiles (distances.plan_tiles).
        mode = 0 / 1 (DISTANCES_MODES: a radius in pairs, basis points of the relative distance) and its threshold.  Returns a
        dict of device tensors: status, npairs, neighbours, leader int32[S], keep bool[S] and common (with `matrix`: the
        block-diagonal int32 matrix of the groups, flat, group g's cells from sum of n^2 of the groups before it on; else
        None: then nothing of that size is written).  Only the two result words come to the host."""
        import torch
        L = _lib.load()
        dev = partner.device
        assert partner.is_cuda and partner.dtype == torch.int32 and partner.dim() == 1 and partner.is_contiguous()
        row_start, row_width = np.asarray(row_start, np.int64), np.asarray(row_width, np.int32)
        group_off, tiles = np.asarray(group_off, np.int32), np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
        S, G, T = len(row_start), len(group_off) - 1, len(tiles)
        n = np.diff(group_off.astype(np.int64))
        assert len(row_width) == S and G >= 1 and group_off[0] == 0 and group_off[-1] == S and (n >= 0).all()
        mat_off = offsets(n * n)
        cells, Wmax = int(mat_off[-1]) if matrix else 0, int(row_width.max())
        with torch.cuda.device(dev):
            d_start, d_width, d_group, d_goff, d_moff, d_tiles = _upload_once(
                [row_start, row_width, np.repeat(np.arange(G, dtype=np.int32), n), group_off, mat_off, tiles], dev)
            nbytes = int(L.sq_structure_distances_scratch(S, Wmax, T))
            scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            res = dict(status=new(S, torch.int32), npairs=new(S, torch.int32), neighbours=new(S, torch.int32), leader=new(S, torch.int32),
                       keep=new(S, torch.uint8), common=new(cells, torch.int32) if matrix else None)
            out = torch.empty(2, dtype=torch.int64, device=dev)
            _lib.check(L.sq_structure_distances(_ptr(partner), int(partner.numel()), _ptr(d_start), _ptr(d_width), _ptr(d_group), S, Wmax,
                                                _ptr(d_goff), _ptr(d_moff), G, int(n.max()), _ptr(d_tiles), T, int(mode), int(threshold),
                                                _ptr(scratch), nbytes, _ptr(res["status"]), _ptr(res["npairs"]), _ptr(res["common"]), cells,
                                                _ptr(res["neighbours"]), _ptr(res["leader"]), _ptr(res["keep"]), _ptr(out), _stream(dev)))
            _result_words(out, "sq_structure_distances: a tile or a group outside the rows")
        res["keep"] = res["keep"].bool()
        return res

    def project_rows(self, rows, structs, shared, Lmax, canonical_only=False, min_loop=0):
        """Structure lines over the columns of an alignment projected onto the residues of its rows, on the device
        (sq_project_rows): rows = uint8 device tensor [R, L] of the rows' ASCII bytes; structs = int32 device tensor of
        partners, [K, L] when `shared` (read by every row where it is) else [R, K, L]; Lmax >= the residues of every row.
        Returns a dict of device tensors: length int32[R], col_of int32[R, Lmax], pos_of int32[R, L], partner int32[R, K, Lmax],
        cls uint8[R, K, L], counts int32[R, K, 12], status int32[R, K].  Nothing comes to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        dev, R, Lcols = rows.device, int(rows.shape[0]), int(rows.shape[1])
        assert structs.dtype == torch.int32 and structs.device == dev and structs.is_contiguous()
        assert tuple(structs.shape[-1:]) == (Lcols,) and structs.dim() == (2 if shared else 3) and (shared or int(structs.shape[0]) == R)
        K, Lmax = int(structs.shape[-2]), int(Lmax)
        with torch.cuda.device(dev):
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            res = dict(length=new(R, torch.int32), col_of=new((R, Lmax), torch.int32), pos_of=new((R, Lcols), torch.int32),
                       partner=new((R, K, Lmax), torch.int32), cls=new((R, K, Lcols), torch.uint8),
                       counts=new((R, K, PROJECT_COUNTS), torch.int32), status=new((R, K), torch.int32))
            _lib.check(L.sq_project_rows(_ptr(rows), R, Lcols, _ptr(structs), 0 if shared else K * Lcols, K, Lmax, int(bool(canonical_only)),
                                         int(min_loop), _ptr(res["length"]), _ptr(res["col_of"]), _ptr(res["pos_of"]), _ptr(res["partner"]),
                                         _ptr(res["cls"]), _ptr(res["counts"]), _ptr(res["status"]), _stream(dev)))
        return res

    def lift_rows(self, rows, short, start, stride, nstruct, K, Lmax):
        """Structure lines over the residues of the rows of an alignment lifted onto its columns, on the device
        (sq_lift_rows): rows = uint8 device tensor [R, L]; short = a flat int32 device tensor of partners in residue
        coordinates, read where it is; the small tables are host arrays and go up in one copy: line k < nstruct[r] of row r
        starts at short[start[r] + k * stride[r]].  Returns a dict of device tensors: length int32[R], col_of int32[R, Lmax],
        pos_of int32[R, L], partner int32[R, K, L], status int32[R, K], nstruct int32[R].  Nothing comes to the host."""
        import torch
        L = _lib.load()
        assert rows.dtype == torch.uint8 and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        dev, R, Lcols, K, Lmax = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(K), int(Lmax)
        assert short.dtype == torch.int32 and short.device == dev and short.dim() == 1 and short.is_contiguous()
        start, stride, nstruct = np.asarray(start, np.int64), np.asarray(stride, np.int32), np.asarray(nstruct, np.int32)
        assert start.shape == stride.shape == nstruct.shape == (R,)
        with torch.cuda.device(dev):
            d_start, d_stride, d_nstruct = _upload_once([start, stride, nstruct], dev)
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            res = dict(length=new(R, torch.int32), col_of=new((R, Lmax), torch.int32), pos_of=new((R, Lcols), torch.int32),
                       partner=new((R, K, Lcols), torch.int32), status=new((R, K), torch.int32), nstruct=d_nstruct)
            _lib.check(L.sq_lift_rows(_ptr(rows), R, Lcols, _ptr(short), int(short.numel()), _ptr(d_start), _ptr(d_stride), _ptr(d_nstruct), K,
                                      Lmax, _ptr(res["length"]), _ptr(res["col_of"]), _ptr(res["pos_of"]), _ptr(res["partner"]),
                                      _ptr(res["status"]), _stream(dev)))
        return res

    def score_tensors(self, recs, partner, row_start, row_rec):
        """ScoreStruct, stems and metrics of given structures on the device (sq_score_structs_dev; SQRNdbnseq.py:958-970,
        1249-1258).  recs: the records (score.ScoreRecord: prepared on the host once per record, however many rows it has);
        partner: a flat int32 CUDA tensor of partner rows in input columns; row_start / row_rec: per row (host arrays) where
        it starts in partner and its record.  Returns device tensors: scores float64[rows, 3], metrics float64[rows, 6],
        status / npairs / nstems int32[rows], stems int32[S, 3], stem_off int64[rows + 1], ref_scores float64[records, 3],
        ref_status int32[records].  No sq_batch.  Enqueued on the current stream; the one wait is for the number of stems,
        which sizes their tensor."""
        import torch
        assert partner.is_cuda and partner.dtype == torch.int32 and partner.dim() == 1 and partner.is_contiguous()
        L = _lib.load()
        dev, R, rows = partner.device, len(recs), len(row_rec)
        lens = np.array([rec.n for rec in recs], np.int64)
        pos_off = offsets(lens)
        cat = lambda parts, dt: np.concatenate([np.asarray(p, dt).reshape(-1) for p in parts] + [np.zeros(0, dt)])
        has_reacts = np.array([rec.reacts is not None for rec in recs], np.uint8)
        react_len = int(max((rec.n for rec in recs if rec.reacts is not None), default=0))
        arrays = [pos_off, cat([rec.codes for rec in recs], np.uint8), has_reacts, np.array([rec.nsep for rec in recs], np.int32),
                  cat([rec.known_partner for rec in recs], np.int32),
                  np.array([len(rec.known) if rec.known is not None else -1 for rec in recs], np.int32),
                  self._pow17_table(int(lens.max(initial=0))), np.asarray(row_start, np.int64).reshape(-1), np.asarray(row_rec, np.int32).reshape(-1)]
        if react_len:
            arrays.append(cat([np.asarray(rec.reacts, np.float64) if rec.reacts is not None else np.zeros(rec.n) for rec in recs], np.float64))
        if rows:                                                     # (every row lies inside the tensor: the kernels trust it)
            width = np.array([len(rec.seq) for rec in recs], np.int64)[arrays[8]]
            assert int(arrays[7].min()) >= 0 and int((arrays[7] + width).max()) <= partner.numel(), "a row outside the partner tensor"
        gaps = any(rec.has_gap for rec in recs)
        if gaps:                                                     # (the maps between input columns and gap-free positions)
            col_off = offsets([len(rec.colmap) for rec in recs])
            arrays += [col_off, cat([rec.colmap for rec in recs], np.int32), cat([rec.gfcol for rec in recs], np.int32)]
        with torch.cuda.device(dev):
            up = _upload_once([a if len(a) else np.zeros(1, a.dtype) for a in arrays], dev)
            d = _lib.ScoreDesc(nrec=R, max_react_len=react_len, d_pos_off=_ptr(up[0]), d_codes=_ptr(up[1]), d_has_reacts=_ptr(up[2]),
                               d_nsep=_ptr(up[3]), d_known=_ptr(up[4]), d_known_n=_ptr(up[5]), d_pow=_ptr(up[6]), pow_len=len(arrays[6]),
                               d_reacts=_ptr(up[9]) if react_len else None)
            if gaps:
                d.d_col_off, d.d_colmap, d.d_gfcol = (_ptr(t) for t in up[-3:])
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            out = dict(scores=new((rows, 3), torch.float64), metrics=new((rows, 6), torch.float64), status=new(rows, torch.int32),
                       npairs=new(rows, torch.int32), nstems=new(rows, torch.int32), ref_scores=new((R, 3), torch.float64),
                       ref_status=new(R, torch.int32))
            nbytes = int(L.sq_score_scratch(R))
            scratch = new(nbytes // 4, torch.int32)
            stem_off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
            o = _lib.ScoreRows(nrows=rows, d_partner=_ptr(partner), d_row_start=_ptr(up[7]), d_row_rec=_ptr(up[8]), d_status=_ptr(out["status"]),
                               d_npairs=_ptr(out["npairs"]), d_nstems=_ptr(out["nstems"]), d_stem_off=_ptr(stem_off), d_stems=None, stem_cap=0,
                               d_scores=_ptr(out["scores"]), d_metrics=_ptr(out["metrics"]), d_ref_scores=_ptr(out["ref_scores"]),
                               d_ref_status=_ptr(out["ref_status"]))
            stream = _stream(dev)
            _lib.check(L.sq_score_structs_dev(C.byref(d), C.byref(o), 0, _ptr(scratch), nbytes, stream))
            stem_off[1:] = torch.cumsum(out["nstems"], 0, dtype=torch.int64)
            nstems = int(stem_off[-1].item())
            out["stems"] = new((nstems, 3), torch.int32)
            o.d_stems, o.stem_cap = (_ptr(out["stems"]) if nstems else None), nstems
            _lib.check(L.sq_score_structs_dev(C.byref(d), C.byref(o), 1, _ptr(scratch), nbytes, stream))
        out["stem_off"] = stem_off
        return out

    def elements_tensors(self, recs, partner, row_start, row_rec):
        """The loop and pseudoknot annotation of given structures on the device (sq_elements_rows).  recs, partner, row_start,
        row_rec as for score_tensors.  Returns device tensors: element int8 / level int16 / loop_of int32 [cells] (row q's
        columns from cell_off[q] on), cell_off int64[rows + 1], status / npairs / nlevels / nloops int32[rows], loop_off
        int64[rows + 1], loops int32[S, 6].  A row of status 2 (more stems than the kernel's LDS holds, more than 64 levels) is
        the caller's to annotate.  No sq_batch.  Enqueued on the current stream; the one wait is for the number of loops,
        which sizes their tensor."""
        import torch
        assert partner.is_cuda and partner.dtype == torch.int32 and partner.dim() == 1 and partner.is_contiguous()
        L = _lib.load()
        dev, R, rows = partner.device, len(recs), len(row_rec)
        pos_off = offsets([rec.n for rec in recs])
        cat = lambda parts, dt: np.concatenate([np.asarray(p, dt).reshape(-1) for p in parts] + [np.zeros(0, dt)])
        row_start, row_rec = np.asarray(row_start, np.int64).reshape(-1), np.asarray(row_rec, np.int32).reshape(-1)
        width = np.array([len(rec.seq) for rec in recs], np.int64)[row_rec]
        cell_off = offsets(width)
        cells = int(cell_off[-1])
        if rows:                                                     # (every row lies inside the tensor: the kernels trust it)
            assert int(row_start.min()) >= 0 and int((row_start + width).max()) <= partner.numel(), "a row outside the partner tensor"
        arrays = [pos_off, cell_off, row_start, row_rec, cat([rec.codes for rec in recs], np.uint8)]
        gaps = any(rec.has_gap for rec in recs)
        if gaps:                                                     # (the maps between input columns and gap-free positions)
            arrays += [offsets([len(rec.colmap) for rec in recs]), cat([rec.colmap for rec in recs], np.int32),
                       cat([rec.gfcol for rec in recs], np.int32)]
        with torch.cuda.device(dev):
            up = _upload_once([a if len(a) else np.zeros(1, a.dtype) for a in arrays], dev)
            d = _lib.ElementsDesc(nrec=R, max_len=int(max((rec.n for rec in recs), default=0)), d_pos_off=_ptr(up[0]), d_codes=_ptr(up[4]))
            if gaps:
                d.d_col_off, d.d_colmap, d.d_gfcol = (_ptr(t) for t in up[5:8])
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            out = dict(element=new(cells, torch.int8), level=new(cells, torch.int16), loop_of=new(cells, torch.int32),
                       status=new(rows, torch.int32), npairs=new(rows, torch.int32), nlevels=new(rows, torch.int32),
                       nloops=new(rows, torch.int32))
            nbytes = int(L.sq_elements_scratch(cells))
            scratch = new(nbytes // 4, torch.int32)
            loop_off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
            o = _lib.ElementsRows(nrows=rows, cells=cells, d_partner=_ptr(partner), d_row_start=_ptr(up[2]), d_row_rec=_ptr(up[3]),
                                  d_cell_off=_ptr(up[1]), d_element=_ptr(out["element"]), d_level=_ptr(out["level"]),
                                  d_loop_of=_ptr(out["loop_of"]), d_status=_ptr(out["status"]), d_npairs=_ptr(out["npairs"]),
                                  d_nlevels=_ptr(out["nlevels"]), d_nloops=_ptr(out["nloops"]), d_loop_off=_ptr(loop_off), d_loops=None,
                                  loop_cap=0)
            stream = _stream(dev)
            _lib.check(L.sq_elements_rows(C.byref(d), C.byref(o), 0, _ptr(scratch), nbytes, stream))
            loop_off[1:] = torch.cumsum(out["nloops"], 0, dtype=torch.int64)
            nloops = int(loop_off[-1].item())
            out["loops"] = new((nloops, 6), torch.int32)
            o.d_loops, o.loop_cap = (_ptr(out["loops"]) if nloops else None), nloops
            _lib.check(L.sq_elements_rows(C.byref(d), C.byref(o), 1, _ptr(scratch), nbytes, stream))
        out["loop_off"], out["cell_off"] = loop_off, up[1]
        return out

    def _pow17_table(self, nmax):
        """(k / 2) ** 1.7 for k <= 4 nmax with the host's pow, as ScoreStruct's `bpsum ** power` computes it (:884): a stem of
        an n-nt record sums at most 4 x n / 2.  Kept for the longest record seen.  Python's float power IS the libm call the
        reference makes; numpy's vectorised power may not be.  One pass of 4 n entries: ~20 ms once for a 32,768-nt record."""
        have = self._pow17
        if have is None or len(have) < 4 * nmax + 1:
            have = self._pow17 = np.array([(0.5 * k) ** 1.7 for k in range(4 * max(nmax, 64) + 1)], np.float64)
        return have[:4 * nmax + 1]
