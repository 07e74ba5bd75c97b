"""HIP engine: batches sequences, owns the device workspace (a torch uint8 tensor) and
drives libsquarna_hip.so through its C ABI.  PyTorch is plumbing here (device memory,
stream, torch.distributed); all arithmetic runs in the hand-written gfx950 kernels.

This module is batching and the fold / retry machinery (sub-batches, the capacity retry, alignment step 1 and entropy
mode through Batch).  The batch-free device entries -- matrix_select, matrix_cells, first_fit, align_pair_count,
window_pair_count, score_tensors -- live in device_calls.DeviceCalls, which HipEngine inherits.

There is NO CPU fallback: without the built library or without a GPU the engine raises.
Tests may install another engine with :func:`use_engine` (tests/ only use that to check
the host-side text layer on CPU against the oracle).
"""
import contextlib
import threading
import weakref

import numpy as np

from . import _lib, switches
from .dbn import gap_mask
# every name callers outside this module take from `engine` (bench.py, tests/, tools/, api.py, align.py, core.py, parallel.py)
from .records import Prepared, PackedRows  # noqa: F401
from .batch import Batch, fold_concurrently
from .device_calls import DeviceCalls, _upload_once
from .results import unpack_result, packed_pair_tables, _Blocks, _BlockRun  # noqa: F401
from .rows import offsets
from .bpp import vienna_bpp, set_bpp_provider, bpp_terms, check_bpp_matrix  # noqa: F401
from .plan import (pool_slots_wanted, pool_slots_wanted_many, pool_slot_cap, slot_bytes, default_structs,  # noqa: F401
                   MIN_CAND_PER_NT, SubBatchPlan, _kept_bytes_per_slot, _free_device_bytes, _shared_weights)


def _cut_in_two_lanes(groups, hints, tensors=False):
    """SQ_ENGINE_LANES=2 and one big group: (groups, hints, back) with the group cut into two concurrent batches, back = the
    records' places (for one-shot calls the second batch's set-up costs more than the overlap saves, so that is opt-in);
    else the arguments and None.  tensors: the results are whole-batch tables (fold_tensors), which are not cut."""
    if len(groups) == 1 and switches.engine_lanes() >= 2 and len(groups[0]) >= 256 and hints[0] is None and not tensors:
        recs = groups[0]
        cost = [float(len(r[0])) ** 2 * len(r[4]) for r in recs]
        if sum(cost) >= 1e8 and not any(len(r) > 5 and r[5] is not None and hasattr(r[5], "is_cuda") for r in recs) \
                and not any(_bpp_of(r) is not None for r in recs):
            from .parallel import lpt_partition
            back = [p for p in lpt_partition(cost, 2) if p]
            return [[recs[k] for k in idx] for idx in back], [None] * len(back), back
    return groups, hints, None


def _undo_two_lane_cut(back, outs, refs):
    """The results of _cut_in_two_lanes' batches as those of the one group, in its order."""
    n = sum(len(idx) for idx in back)
    o, rf = [None] * n, [None] * n
    for idx, oo, rr in zip(back, outs, refs):
        for k, x, y in zip(idx, oo, rr):
            o[k], rf[k] = x, y
    return [o], [rf]


def _packed_results(batches):
    """fold_records(_packed=True): per batch [(packed record, None)]."""
    res = []
    for b in batches:
        views = b.detach_packed() if not switches.no_detach() else None
        if views is not None:                            # (no copy: the records stay where the device wrote them)
            res.append([(v, None) for v in views])
            continue
        buf, off = b.pack_all()
        res.append([(buf[off[k]:off[k + 1]].tobytes(), None) for k in range(b.nseq)])
    return res


def _block_results(batches, groups, cfg):
    """fold_records(_blocks=cfg), Predict's printing path: the library writes the blocks; a record it leaves out (or a batch
    whose tail ran on the host) comes back as its result tuple and the caller formats it.  Records carry their block fields
    behind the fold's: (..., name, encoded reactivity line, index of their paramset-name list)."""
    res = []
    for b, recs in zip(batches, groups):
        texts = b.write_blocks([r[6] for r in recs], [r[0] for r in recs], [r[7] for r in recs],
                               [r[2] for r in recs], [r[3] for r in recs], [r[8] for r in recs],
                               cfg["psnames"], cfg["conslim"], cfg["outplim"])
        if isinstance(texts, _Blocks):
            res.append(_BlockRun(texts))
        elif texts is None or any(t is None for t in texts):
            full = b.results_all()
            res.append([(("text", texts[k]) if texts and texts[k] is not None else ("pred", full[k]), None) for k in range(b.nseq)])
        else:
            res.append([(("text", t), None) for t in texts])
    return res


_TABLES = ("partner", "scores", "pset_mask", "metrics", "row_off", "cell_off")

#: where a record carries its device matrix of base-pair probabilities (0..5: the fold's fields, 6..8: Predict's block fields)
_BPP_AT = 9


def _with_bpp(records, bpp):
    """The records with their matrices of base-pair probabilities behind them (index _BPP_AT), so that whatever slices,
    reorders or repeats the records -- sub-batches, lanes, the capacity retry -- carries each matrix with its record.
    bpp: per record a CUDA float64 tensor of the record's gap-free length (separators counted) squared, or None."""
    if len(bpp) != len(records):
        raise ValueError("bpp: %d matrices for %d records" % (len(bpp), len(records)))
    out = []
    for k, (r, m) in enumerate(zip(records, bpp)):
        if m is not None:
            check_bpp_matrix(m, int(np.count_nonzero(~gap_mask(r[0]))), "bpp matrix of record %d" % k)
        out.append(tuple(r[:_BPP_AT]) + (None,) * (_BPP_AT - len(r)) + (m,))
    return out


def _bpp_of(r):
    return r[_BPP_AT] if len(r) > _BPP_AT else None


class _TensorRun:
    """fold_records(_tensors=True) result of one batch: its pair tables as torch tensors on the batch's device (the layout
    of sq_result_pairs_dev, gap-free coordinates), the host's copy of the sizes, and where the tables were formed."""
    __slots__ = ("tables", "nstruct", "lengths", "source")

    def __init__(self, tables, nstruct, lengths, source):
        self.tables, self.nstruct, self.lengths, self.source = tables, nstruct, lengths, source


def _tensor_results(batches):
    """fold_records(_tensors=True), fold_tensors' path: per batch [((its _TensorRun, record), None)].  The device tail's
    results leave as tensors formed on the device (Batch.result_tensors); a batch whose tail ran on the host is converted
    from its packed records (the same content; a Python loop over the records and their bracket levels on the host,
    results.packed_pair_tables: the cost of such a batch's results, tens of microseconds per record) and uploaded once."""
    res = []
    for b in batches:
        tables = b.result_tensors()
        if tables is not None:
            nstruct, lengths = b.result_counts()
            run = _TensorRun(tables, nstruct, lengths, "device")
        else:
            host, nstruct, lengths = packed_pair_tables(*b.pack_all())
            run = _TensorRun(dict(zip(_TABLES, _upload_once([host[k] for k in _TABLES], b.device))), nstruct, lengths, "host")
        res.append([((run, k), None) for k in range(b.nseq)])
    return res


def _join_runs(runs):
    """The tables of consecutive batches as one set: concatenated, the offsets rebased."""
    import torch
    if len(runs) == 1:
        out = dict(runs[0].tables)
    else:
        out = {k: torch.cat([r.tables[k] for r in runs]) for k in ("partner", "scores", "pset_mask", "metrics")}
        for key in ("row_off", "cell_off"):
            parts, base = [], 0
            for q, r in enumerate(runs):
                t = r.tables[key]
                parts.append((t if q == len(runs) - 1 else t[:-1]) + base)
                base += int(r.nstruct.sum()) if key == "row_off" else int(((1 + r.nstruct) * r.lengths).sum())
            out[key] = torch.cat(parts)
    out["nstruct"] = np.concatenate([r.nstruct for r in runs])
    out["lengths"] = np.concatenate([r.lengths for r in runs])
    sources = {r.source for r in runs}
    out["source"] = sources.pop() if len(sources) == 1 else "mixed"
    return out


def _tuple_results(batches):
    """fold_records: per batch [(SQRNdbnseq tuple, reference scores or None)]."""
    return [b.results_all() for b in batches]


class HipEngine(DeviceCalls):
    """Default engine: everything on the GPU through libsquarna_hip.so."""
    name = "hip"
    writes_blocks = True          # fold_records(..., _blocks=cfg): the library forms Predict's output blocks

    def __init__(self, max_structs=0, cand_per_nt=0):
        self.max_structs = max_structs
        self.cand_per_nt = cand_per_nt
        #: per record of the last fold_records call: ScoreStruct of its known structure (C tail) or None
        self.last_ref_scores = None
        #: driver (Batch.fold_driver) and peak structures (of the first batch) of the last fold
        self.last_fold_driver, self.last_fold_peak = 0, 0
        #: folds repeated with a larger batch after a CapacityError
        self.capacity_retries = 0
        # (the scale the pools of an earlier call reached under the same paramsets, pool limit and lengths: the estimate is for the
        # widest pools a configuration can have -- 500nobpp at 500 nt reaches an eighth of it -- and a first sub-batch sized by it
        # was a quarter of the records, with the full wait for its Edmonds graphs)
        self._pool_scale = {}
        # (a lane keeps its stream for the engine's lifetime: torch's caching allocator hands a freed workspace only to the
        # stream it was allocated on -- a new stream per call allocated tens of GB anew every time)
        self._lane_streams = {}
        # max |M| of a shared stem matrix, remembered through a WEAK reference: the engine is process-wide and must not keep an
        # L x L device matrix (200 MB at L = 5000) alive after the alignment that owns it has ended
        self._sm_maxabs = (None, None)

    def fold_records(self, records, bpp=None, **opts):
        """records: list of (seq, reacts, restraints, dbn, paramsets, stemmatrix);
        returns the list of SQRNdbnseq return tuples, in order.
        bpp: per record a CUDA float64 N x N tensor of base-pair probabilities (N = the gap-free length, separators counted:
        what the reference hands to ViennaRNA), or None -- it takes the provider's place for that record, and the terms of its
        bpp != 0 paramsets are formed on the device (|bpp| 0.5 or 1; a record with another exponent has its matrix copied
        to the host once and takes the host terms of bpp.bpp_terms).  ValueError on a wrong size, dtype, device or a strided
        column.  The tensors are read, never written; a repeated fold (capacity retry) reads them again."""
        if bpp is not None:
            records = _with_bpp(records, bpp)
        # Building tens of thousands of small containers (Prepared records, result tuples) with the cyclic collector on
        # costs ~10 us per record in generation scans of objects that hold no cycles: 220 of 340 ms for 10,000 records.
        import gc
        was = gc.isenabled()
        gc.disable()
        try:
            return self._fold_records(records, **opts)
        finally:
            if was:
                gc.enable()

    def fold_records_packed(self, records, bpp=None, **opts):
        """Like fold_records, but every record's result stays in the library's packed form (bytes, sq_result_pack layout):
        the payload ranks exchange (parallel.py).  `unpack_result(Prepared(...), blob)` decodes one on any rank."""
        return self.fold_records(records, bpp=bpp, _packed=True, **opts)

    def fold_tensors(self, records, bpp=None, **opts):
        """Like fold_records, but the results stay on the device as data: dict of torch tensors partner int32[cells],
        scores float64[rows, 3], pset_mask int64[rows], metrics float64[records, 16], row_off / cell_off int64[records + 1]
        in the layout of sq_result_pairs_dev (include/squarna_hip.h; gap-free coordinates), the host arrays nstruct and
        lengths (int64 per record), and source: "device" when the ranking tail of every batch ran on the device, "host"
        when none did (rankbydiff, forced hardrest pairs, conslim > 1, > 4,096 final structures: converted from the packed
        records), "mixed" otherwise.  `keep` and `bpp` as for fold_records."""
        import torch
        if not records:
            raise ValueError("fold_tensors needs at least one record")
        kept = self.last_ref_scores                                  # (the known structures' scores are in the metrics table)
        out = self.fold_records(records, bpp=bpp, _tensors=True, **opts)
        self.last_ref_scores = kept
        # every record carries (the tables of its batch, its place in them): the batches must cover the records in order,
        # each whole -- what the sub-batch planner hands out; anything else would join the tables in another order
        runs, at = [], 0
        for run, k in out:
            if not runs or runs[-1] is not run:
                assert not runs or at == len(runs[-1].nstruct), "a batch's records are not consecutive"
                runs.append(run)
                at = 0
            assert k == at, "a batch's records are not in order"
            at += 1
        assert at == len(runs[-1].nstruct), "a batch's records are not consecutive"
        with torch.cuda.device(runs[0].tables["partner"].device):
            return _join_runs(runs)

    def _fold_records(self, records, **opts):
        """`keep`: only the first `keep` structures of every record are fetched (Predict prints outplim of them)."""
        poollim = opts.get("poollim", 1000)
        if not self.max_structs and poollim > 1 and len(records) > 1:
            # wide pools: as many records per batch as the device pools have slots for (a fold that outgrows them is
            # repeated by the library's host loop -- correct, but several times slower)
            lens = [len(r[0]) for r in records]
            per_rec = pool_slots_wanted_many(lens, [r[4] for r in records], poollim, rarely_branch=_shared_weights(records))
            cap = pool_slot_cap(max(lens), want=int(per_rec.sum()))
            if int(per_rec.sum()) > cap:
                return self._fold_in_sub_batches(records, per_rec.tolist(), cap, opts)
        out, refs = self._fold_groups([records], [None], opts)
        self.last_ref_scores = refs[0]
        return out[0]

    def _fold_in_sub_batches(self, records, per_rec, cap, opts):
        """Consecutive sub-batches sized to the device-pool slots (plan.SubBatchPlan).
        (Measured: folding the sub-batches two at a time on streams of their own gains nothing -- 512 x 5000-column
        alignment 10.5 s either way, 3000 x 300 nt with pools of a thousand 2.1 s: these folds are bound by the scoring
        kernel, not by gaps between rounds -- and costs the second batch's memory.)"""
        # dense per-job matrices (alignment step 2: N x N fp64 + fp32 per job) bound a sub-batch as well: 32 GB of them
        # (allocating and touching 100 GB per batch costs more than the larger rounds save)
        # (not the rows of an alignment weighted by ONE device matrix: the kernels read it through the gap map, no slice exists --
        # unless SQ_MUL_GATHER=1 asks for the round-3 form)
        direct = _shared_weights(records) and not switches.mul_gather()
        dense = [12.0 * len(r[0]) ** 2 * len(r[4]) if len(r) > 5 and r[5] is not None and not direct else 0.0 for r in records]
        # SQ_ENGINE_SUBLANES=2: two sub-batches at a time, each from a thread of its own (a batch's fold releases the GIL).
        # Measured again in round 6 (1,000 records of 500 nt, pools of a thousand on kept lists): 566 ms against 398 one after
        # the other -- each lane's batches get half of the slots, so there are twice as many, and every one of them waits ~100 ms
        # for the 500-vertex Edmonds graphs of its records however few they are.  Off by default.
        # Not the rows weighted by ONE device matrix: they share that tensor on the caller's stream.
        lanes = switches.engine_sublanes()
        # Nor records with their probabilities on the device: those tensors are complete on the caller's stream.
        if direct or sum(dense) > 0 or opts.get("_blocks") or opts.get("_tensors") or any(_bpp_of(r) is not None for r in records):
            lanes = 1
        mkey = (tuple(tuple(sorted((k, str(v)) for k, v in ps.items())) for ps in records[0][4]),       # (the paramsets by content: an id() is reused)
                int(opts.get("poollim", 1000)), max(len(r[0]) for r in records) // 64)
        plan = SubBatchPlan(per_rec, dense, cap, switches.dense_gb() * 1e9, lanes, self._pool_scale.get(mkey, 1.0))
        n = len(records)
        out, refs = [None] * n, [None] * n

        def work(k):
            import torch
            if lanes > 1 and k not in self._lane_streams:
                self._lane_streams[k] = torch.cuda.Stream()
            ctx = torch.cuda.stream(self._lane_streams[k]) if lanes > 1 else contextlib.nullcontext()
            try:
                with ctx:
                    for a, b, g in iter(plan.take, None):
                        info = {}
                        o, r = self._fold_groups([records[a:b]], [g], opts, info=info, inflight=lanes)
                        out[a:b] = o[0]
                        refs[a:b] = r[0]
                        plan.report(a, b, info["driver"], info["peak"])
            except BaseException as e:                                   # (re-raised on the caller's thread)
                plan.fail(e)

        if lanes == 1:
            work(0)
        else:
            ths = [threading.Thread(target=work, args=(k,)) for k in range(lanes)]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
        if plan.reported:
            self._pool_scale[mkey] = plan.scale
        if plan.error is not None:
            raise plan.error
        self.last_fold_driver, self.last_fold_peak = plan.driver, plan.peak
        self.last_ref_scores = refs
        return out

    def _make_batch(self, records, slots_hint, opts, grow=(1, 1)):
        """(Batch, fold options) for these records.  opts: fold_records' keyword arguments (not modified).  grow: factors on
        the candidate capacity per nucleotide and on the structure slots (a fold that outgrew them is repeated)."""
        opts = dict(opts)
        opts.pop("_packed", None)
        opts.pop("_blocks", None)
        opts.pop("_tensors", None)
        interchainonly = opts.pop("interchainonly", False)
        keep = opts.pop("keep", None)
        M, B = opts.pop("M", 1.8), opts.pop("B", -0.6)
        prepared = [Prepared(r[0], r[1], r[2], r[3]) for r in records]
        psets = [r[4] for r in records]
        # (a record's matrix of probabilities on the device -- given with the record, or returned by the provider -- is handed
        # to the batch as it is: the same unmodified tensor for every batch built from the record)
        bpp, bpp_dev = bpp_terms(prepared, psets, M, B, given=[_bpp_of(r) for r in records], device=True)
        mul = None
        mul_shared = None
        if _shared_weights(records):
            # alignment step 2 with the stem matrix still on the GPU: no per-record copies (Batch(mul_shared=...))
            sm0 = records[0][5]
            ref, val = self._sm_maxabs
            if ref is None or ref() is not sm0:
                val = float(sm0.abs().max().item())
                self._sm_maxabs = (weakref.ref(sm0), val)
            mul_shared = (sm0, [np.flatnonzero(~gap_mask(r[0])).astype(np.int32) for r in records], val)
        elif any(len(r) > 5 and r[5] is not None for r in records):
            mul = []
            for r, p in zip(records, prepared):
                sm = r[5] if len(r) > 5 else None
                if sm is not None and hasattr(sm, "is_cuda"):
                    sm = sm.cpu().numpy()
                if sm is not None:                                   # :1031-1034
                    sm = np.delete(np.delete(np.asarray(sm, dtype=np.float64), p.gapidx, 0), p.gapidx, 1)
                mul.extend([sm] * len(r[4]))
        # (a fold that still outgrows the default slots is repeated by the library's host loop)
        max_structs = default_structs(sum(len(pl) for pl in psets), self.max_structs)
        if not self.max_structs and opts.get("poollim", 1000) > 1:
            want = slots_hint if slots_hint else int(pool_slots_wanted_many(
                [len(p.shortseq) for p in prepared], psets, opts.get("poollim", 1000), rarely_branch=_shared_weights(records)).sum())
            max_structs = max(max_structs, min(want, pool_slot_cap(max(len(p.shortseq) for p in prepared), want=want)))
        cand = self.cand_per_nt
        if grow[0] > 1:
            # (the library sizes a structure's candidate records by max(cand_per_nt x N, its estimate for random sequences --
            # ~0.19 N^2 runs at minlen 1): the factor applies to the larger of the two
            nmax = max(len(p.shortseq) for p in prepared)
            runs = max(0.375 ** (max(1.0, float(np.ceil(ps["minlen"]))) - 1.0) for pl in psets for ps in pl)
            cand = int(max(cand, MIN_CAND_PER_NT, 0.117 * 1.6 * nmax * runs) * grow[0]) + 1
        b = Batch(prepared, psets, interchainonly=interchainonly, mul=mul, fp32=False, bpp=bpp,
                  max_structs=max_structs * grow[1], cand_per_nt=cand, mul_shared=mul_shared,
                  pool_lists=opts.get("poollim", 1000) > 1 and mul_shared is None, bpp_dev=bpp_dev)
        b.limit_results(keep)
        return b, opts

    def _fits_device(self, records, slots_hint, opts, grow):
        """Whether a batch of these records with its capacities grown by `grow` still fits the free device memory (half of
        it: the fold's scratch and the caller's tensors live there too)."""
        n = max((len(r[0]) for r in records), default=1)
        njobs = sum(len(r[4]) for r in records)
        structs = default_structs(njobs, self.max_structs) * grow[1]
        cand = max(self.cand_per_nt, MIN_CAND_PER_NT) * grow[0] * n * 32.0   # candidate records of a structure, 32 bytes each
        return structs * slot_bytes(n, opts.get("poollim", 1000) > 1) + min(structs, 4 * njobs) * cand <= _free_device_bytes() // 2

    def _fold_with_retry(self, groups, hints, opts, inflight=1):
        """The folded batches of the groups, one each, all folded at the same time; the caller closes them.
        The reference has no capacities (SQRNdbnseq.py:427-495 builds Python lists): a fold that outgrows what its batch
        was created with -- the candidate records of a structure are sized for random sequences, GC-only or minlen = 1
        inputs hold several times as many runs -- is repeated with a larger batch; the caller never sees the error."""
        import torch
        if len(groups) > 1:
            torch.cuda.current_stream().synchronize()            # (inputs made on this stream, e.g. the shared stem matrix)
        grow, batches = [1, 1], []
        try:
            for attempt in range(8):
                for q, (recs, hint) in enumerate(zip(groups, hints)):
                    # concurrent batches on streams of their own: kernels of one fill the gaps of the other
                    ctx = torch.cuda.stream(torch.cuda.Stream()) if q > 0 else contextlib.nullcontext()
                    with ctx:
                        b, fold_opts = self._make_batch(recs, hint, opts, tuple(grow))
                    batches.append(b)
                try:
                    if len(batches) == 1:
                        if inflight > 1:
                            batches[0].set_inflight(inflight)            # (sub-batches folded side by side from the engine's threads)
                        batches[0].fold(**fold_opts)
                    else:
                        fold_concurrently(batches, **fold_opts)
                    return batches
                except _lib.CapacityError as e:
                    # which capacity, from the library's own code (sq_last_capacity): candidate records and a round's output
                    # records grow with cand_per_nt, the log of final structures with max_structs; a fixed limit is raised.
                    # The growth stops where the batch would no longer fit the device: the ORIGINAL error is raised then, not
                    # an allocation failure
                    which = {_lib.CAP_CANDIDATES: 0, _lib.CAP_OUTPUT: 0, _lib.CAP_STRUCTS: 1}.get(e.kind)
                    if which is None or attempt == 7:
                        raise
                    grow[which] *= 4
                    if not all(self._fits_device(recs, hint, opts, tuple(grow)) for recs, hint in zip(groups, hints)):
                        raise
                    self.capacity_retries += 1
                    for b in batches:
                        b.close()
                    batches = []
        except BaseException:
            for b in batches:
                b.close()
            raise

    def _fold_groups(self, groups, hints, opts, info=None, inflight=1):
        """Folds every group of records as one batch, all of them at the same time; ([results], [reference scores]) per
        group."""
        groups, hints, back = _cut_in_two_lanes(groups, hints, bool(opts.get("_tensors")))
        batches = self._fold_with_retry(groups, hints, opts, inflight)
        try:
            driver, peak = max(b.fold_driver for b in batches), batches[0].fold_peak_structs
            if info is not None:
                info["driver"], info["peak"] = driver, peak
            else:
                self.last_fold_driver, self.last_fold_peak = driver, peak
            if opts.get("_packed"):
                res = _packed_results(batches)
            elif opts.get("_blocks"):
                res = _block_results(batches, groups, opts["_blocks"])
            elif opts.get("_tensors"):
                res = _tensor_results(batches)
            else:
                res = _tuple_results(batches)
        finally:
            for b in batches:
                b.close()
        if any(isinstance(both, _BlockRun) for both in res):
            # (whole-text results stay whole when there is one batch; several batches / lanes: per-record entries)
            if len(res) == 1 and back is None:
                return [res[0]], [[None] * len(res[0].blocks)]
            res = [[(("text", t), None) for t in both.blocks] if isinstance(both, _BlockRun) else both for both in res]
        outs, refs = [[r[0] for r in both] for both in res], [[r[1] for r in both] for both in res]
        return _undo_two_lane_cut(back, outs, refs) if back is not None else (outs, refs)

    def yield_stems(self, records, bpweights, minlen, minbpscore, interchainonly=False):
        """Alignment step 1 (SQRNdbnali.py:60-108): for every (seq, reacts, restraints) the stems of
        the gap-free sequence in emission order.  Returns [(shortseq, [(i, j, len, score), ...])]."""
        ps = dict(bpweights=bpweights, bpp=0, algorithms={"G"}, suboptmax=1.0, suboptmin=1.0, suboptsteps=1.0,
                  minlen=minlen, minbpscore=minbpscore, minfinscorefactor=1.0, bracketweight=-2.0, distcoef=0.09,
                  orderpenalty=1.0, loopbonus=0.125, maxstemnum=1e6)
        prepared = []
        for seq, reacts, restraints in records:
            p = Prepared(seq, reacts if reacts else None, restraints, None)
            if not reacts:
                p.shortreacts = [0.5] * len(p.shortseq)                # YieldStems passes reacts=None (:83)
                p.plain_reacts = True
            prepared.append(p)
        out, cap = [], 1 << 21
        est = [int(0.25 * len(p.shortseq) ** 2 * 0.375 ** (max(minlen, 1) - 1)) + 256 for p in prepared]
        lo = 0
        while lo < len(prepared):                                      # chunks sized to the stem buffer
            hi, tot = lo, 0
            while hi < len(prepared) and (hi == lo or tot + est[hi] <= cap):
                tot += est[hi]
                hi += 1
            chunk = prepared[lo:hi]
            with Batch(chunk, [[ps]] * len(chunk), interchainonly=interchainonly, max_structs=self.max_structs,
                       cand_per_nt=max(self.cand_per_nt, 64), fp32=False) as b:
                res = b.optimal(list(range(len(chunk))), [[] for _ in chunk], mode=1, out_cap=max(cap, tot),
                                as_array=True)
            out.extend((p.shortseq, st) for p, st in zip(chunk, res))
            lo = hi
        return out

    def stem_matrix(self, records, bpweights, minlen, minbpscore, interchainonly=False):
        """Alignment step 1 on the device (SQRNdbnali.py:211-242 without MatrixToDBNs): the L x L fp64 column
        matrix of stem scores over all (seq, reacts, restraints) records, as a torch tensor on the GPU.
        Sequences are applied in order, one scatter launch each, so every cell is summed in the reference's
        order; nothing but the gap maps crosses PCIe."""
        import torch
        ps = dict(bpweights=bpweights, bpp=0, algorithms={"G"}, suboptmax=1.0, suboptmin=1.0, suboptsteps=1.0,
                  minlen=minlen, minbpscore=minbpscore, minfinscorefactor=1.0, bracketweight=-2.0, distcoef=0.09,
                  orderpenalty=1.0, loopbonus=0.125, maxstemnum=1e6)
        Lcols = len(records[0][0])
        dev = torch.device("cuda", torch.cuda.current_device())
        matrix = torch.zeros((Lcols, Lcols), dtype=torch.float64, device=dev)
        r0 = records[0][2]
        if (not any(r[1] for r in records) and all((r[2] or None) == (r0 or None) for r in records)
                and all(len(r[0]) == Lcols for r in records) and not switches.no_packed_rows()):
            # the usual alignment: no per-row reactivities, one restraint line for every row (iteration 2) or none -- all rows
            # prepared at once as array code (PackedRows), chunks of rows sized like the per-row form below
            lo = 0
            while lo < len(records):
                hi, cells = lo, 0
                while hi < len(records) and (hi == lo or cells + Lcols ** 2 <= 16e9):
                    cells += Lcols ** 2
                    hi += 1
                pk = PackedRows([r[0] for r in records[lo:hi]], r0 or None)
                with Batch(pk, [[ps]] * (hi - lo), interchainonly=interchainonly, max_structs=self.max_structs,
                           cand_per_nt=max(self.cand_per_nt, 64), fp32=False) as b:
                    b.align_accumulate_packed(pk, matrix)
                    torch.cuda.synchronize(dev)
                lo = hi
            return matrix
        prepared, cols = [], []
        for seq, reacts, restraints in records:
            p = Prepared(seq, reacts if reacts else None, restraints, None)
            if not reacts:
                p.shortreacts = [0.5] * len(p.shortseq)                # YieldStems passes reacts=None (:83)
                p.plain_reacts = True
            prepared.append(p)
            cols.append(np.flatnonzero(~gap_mask(seq)).astype(np.int32))   # ReAlignDict (:20-37)
        # chunks of sequences sized to ~24 GB of bit matrices + candidates
        lo = 0
        while lo < len(prepared):
            hi, cells = lo, 0
            while hi < len(prepared) and (hi == lo or cells + len(prepared[hi].shortseq) ** 2 <= 16e9):
                cells += len(prepared[hi].shortseq) ** 2
                hi += 1
            chunk = prepared[lo:hi]
            with Batch(chunk, [[ps]] * len(chunk), interchainonly=interchainonly, max_structs=self.max_structs,
                       cand_per_nt=max(self.cand_per_nt, 64), fp32=False) as b:
                b.align_accumulate(list(range(len(chunk))), cols[lo:hi], matrix)
                torch.cuda.synchronize(dev)
            lo = hi
        return matrix

    def entropy_tensors(self, recs, interchainonly=False, M=1.8, B=-0.6, stem_matrix=None, bpp=None, scratch_bytes=None):
        """Entropy mode as data (SQRNdbnseq.py:520-545, 1087-1089; sq_entropy_rows): recs = [(seq, reacts, restraints,
        paramset)], one paramset (a dict) per record.  Returns device tensors in gap-free coordinates: position float64 -- the
        row entropies H_i of record r's stem matrix from pos_off[r] on --, pos_off int64[R + 1], mean float64[R] (sum H_i / N;
        NaN for a record without a position), nstems int32[R]; and the host array lengths int64[R].
        stem_matrix: ONE L x L float64 CUDA tensor that weights the pair scores of every record through its gap map
        (Batch(mul_shared=...): read where it is, never written); bpp: per record a CUDA float64 N x N tensor or None, for a
        paramset with bpp != 0.  The records go through Batch in chunks whose dense N x N fp64 tiles fit scratch_bytes
        (default 1 GiB; a larger record gets a chunk of its own); a chunk's kernels see its own tiles alone, so a record's
        values do not depend on its chunk.  Nothing but sizes and offsets crosses PCIe."""
        import torch
        R = len(recs)
        budget = int(scratch_bytes) if scratch_bytes else 1 << 30
        prepared = [Prepared(r[0], r[1], r[2], None) for r in recs]
        lens = np.array([len(p.shortseq) for p in prepared], np.int64)
        if R and int(lens.max()) > 32768:
            k = int(lens.argmax())
            raise ValueError("entropy_tensors: record %d has %d nt; at most 32768 are supported" % (k, lens[k]))
        pos_off = offsets(lens)
        dev = torch.device("cuda", torch.cuda.current_device())
        L = _lib.load()
        lists = {}                                                   # (one list object per paramset: records that share it share the batch's job table)
        psets = [lists.setdefault(id(r[3]), [r[3]]) for r in recs]
        maxabs = None
        if stem_matrix is not None:
            assert stem_matrix.is_cuda and stem_matrix.dtype == torch.float64 and stem_matrix.dim() == 2 and stem_matrix.is_contiguous()
            maxabs = float(stem_matrix.abs().max().item()) if stem_matrix.numel() else 0.0
        live = [k for k in range(R) if lens[k] > 0]                  # (a record without a position: no job, no row, mean NaN)
        chunks, lo = [], 0
        while lo < len(live):
            hi, cells = lo, 0
            while hi < len(live) and (hi == lo or int(L.sq_entropy_scratch(hi - lo + 1, cells + int(lens[live[hi]]) ** 2)) <= budget):
                cells += int(lens[live[hi]]) ** 2
                hi += 1
            chunks.append((live[lo:hi], int(L.sq_entropy_scratch(hi - lo, cells))))
            lo = hi
        with torch.cuda.device(dev):
            position = torch.empty(max(int(pos_off[-1]), 1), dtype=torch.float64, device=dev)[:int(pos_off[-1])]
            mean = torch.full((R,), float("nan"), dtype=torch.float64, device=dev)
            nstems = torch.zeros(R, dtype=torch.int32, device=dev)
            scratch = torch.empty(max((nb for _, nb in chunks), default=0), dtype=torch.uint8, device=dev)
            for idx, nbytes in chunks:
                chunk = [prepared[k] for k in idx]
                cpsets = [psets[k] for k in idx]
                terms, bpp_dev = bpp_terms(chunk, cpsets, M, B, given=[bpp[k] if bpp is not None else None for k in idx], device=True)
                mul_shared = None
                if stem_matrix is not None:
                    mul_shared = (stem_matrix, [np.flatnonzero(~gap_mask(recs[k][0])).astype(np.int32) for k in idx], maxabs)
                d_off, = _upload_once([np.append(pos_off[idx], pos_off[idx[-1] + 1])], dev)
                cmean = torch.empty(len(idx), dtype=torch.float64, device=dev)
                cnst = torch.empty(len(idx), dtype=torch.int32, device=dev)
                cand = max(self.cand_per_nt, 64)
                for attempt in range(4):
                    try:
                        with Batch(chunk, cpsets, interchainonly=interchainonly, max_structs=self.max_structs, cand_per_nt=cand,
                                   fp32=False, bpp=terms, bpp_dev=bpp_dev, mul_shared=mul_shared) as b:
                            b.entropy_rows(list(range(len(idx))), d_off, position, cmean, cnst, scratch[:nbytes])
                        break
                    except _lib.CapacityError as e:
                        # more maximal runs than the candidate records were sized for (GC-only records, minlen 1): the chunk
                        # again with four times as many, as fold_records does
                        if e.kind != _lib.CAP_CANDIDATES or attempt == 3:
                            raise
                        runs = max(0.375 ** (max(1.0, float(np.ceil(pl[0]["minlen"]))) - 1.0) for pl in cpsets)
                        cand = int(max(cand, 0.117 * 1.6 * int(lens[idx].max()) * runs) * 4) + 1
                        self.capacity_retries += 1
                at = torch.from_numpy(np.asarray(idx, np.int64)).to(dev)
                mean[at], nstems[at] = cmean, cnst
            d_pos_off, = _upload_once([pos_off], dev)
        return dict(position=position, pos_off=d_pos_off, mean=mean, nstems=nstems, lengths=lens)

    def entropy(self, record, interchainonly=False):
        """Mean row entropy of the stem matrix under the FIRST paramset, as a string
        (SQRNdbnseq.py:520-545, 1087-1089); the stems come from the GPU scan (mode 1)."""
        seq, reacts, restraints, dbn, paramsets = record[:5]
        p = Prepared(seq, reacts, restraints, dbn)
        ps = paramsets[0]
        mul = None
        sm = record[5] if len(record) > 5 else None
        if sm is not None:                                           # alignment step 2: bpscorematrix * shortsmat
            mul = [np.delete(np.delete(np.asarray(sm, dtype=np.float64), p.gapidx, 0), p.gapidx, 1)]   # (:1031-1034,1084-1085)
        with Batch([p], [[ps]], interchainonly=interchainonly, max_structs=self.max_structs, mul=mul,
                   cand_per_nt=max(self.cand_per_nt, 64)) as b:
            stems = b.optimal([0], [[]], mode=1)[0]
        n = len(p.shortseq)
        sm = np.zeros((n, n))
        for i, j, ln, sc, _ in stems:
            for k in range(ln):
                sm[i + k, j - k] = sc
                sm[j - k, i + k] = sc
        ent = 0
        for i in range(n):
            row = sm[i, :]
            if row.sum():
                probs = [q for q in row / row.sum() if q]
                ent += sum(-(probs * np.log2(probs)))
        return str(round(ent / n, 3))


_engine = None


def get_engine():
    global _engine
    if _engine is None:
        _engine = HipEngine()
    return _engine


@contextlib.contextmanager
def use_engine(engine):
    """Temporarily install another engine (tests only)."""
    global _engine
    old = _engine
    _engine = engine
    try:
        yield engine
    finally:
        _engine = old
