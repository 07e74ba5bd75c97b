"""Batch: the ctypes wrapper of one device-resident batch of fold jobs (libsquarna_hip.so through its C ABI; the workspace
is a torch uint8 tensor)."""
import ctypes as C

import numpy as np

from . import _lib
from .bpp import check_bpp_matrix
from .dbn import DBNToPairs, encode_seq
from .plan import workspace_size_class
from .records import PackedRows
from .results import unpack_result, _metrics, _MASK_IDS, _Blocks
from .rows import offsets


_STEM_DT = np.dtype([("i", "<i4"), ("j", "<i4"), ("len", "<i4"), ("reserved", "<i4"),
                     ("bpscore", "<f8"), ("finscore", "<f8")])


def _pset_struct(ps):
    out = _lib.ParamSet()
    for key, val in ps["bpweights"].items():                         # SQRNdbnseq.py:282-284
        a, b = encode_seq(key)
        if a > 25 or b > 25:
            raise ValueError("bpweights keys must be two letters: %r" % key)
        out.bpweight[a * 32 + b] = val
        out.inbps[a * 32 + b] = 1
        out.bpweight[b * 32 + a] = val
        out.inbps[b * 32 + a] = 1
    out.bpp = float(ps.get("bpp", 0))
    for k in ("suboptmax", "suboptmin", "suboptsteps", "minlen", "minbpscore", "minfinscorefactor",
              "bracketweight", "distcoef", "orderpenalty", "loopbonus", "maxstemnum"):
        setattr(out, k, float(ps[k]))
    out.algorithms = sum(_lib.ALGO_BITS[a] for a in ps["algorithms"])
    return out


def _ptr(a, t=C.c_void_p):
    return a.ctypes.data_as(t)


class Batch:
    """A device-resident batch of fold jobs (one per (record, paramset))."""

    def __init__(self, prepared, psets_per_record, interchainonly=False, ext=None, mul=None,
                 max_structs=0, cand_per_nt=0, device=None, fp32=True, bpp=None, mul_shared=None, pool_lists=False,
                 bpp_dev=None):
        """fp32=False leaves the fp32 score matrices out of the workspace (4 N^2 bytes per job): everything
        but fill() works -- folding only needs the 1-bit-per-cell matrices.
        pool_lists=True: the batch will be folded with pools wider than one; with sequences of 257-1,024 nt the workspace
        then holds the pages of the lists a pool's structures hand to their children (SQ_BATCH_POOL_LISTS).
        mul_shared = (M, cols, maxabs): ONE L x L fp64 torch tensor on the GPU that weights every job of every record
        (alignment step 2), cols[k] = the alignment columns of record k's gap-free positions, maxabs >= max |M|.
        bpp_dev: per record a CUDA float64 N x N torch tensor of base-pair probabilities (values >= 0), or None: the terms of
        the record's bpp != 0 jobs (|bpp| 0.5 or 1) are formed on the device at creation (sq_batch_desc.bpp_matrix_dev) instead
        of being uploaded per job through `bpp`.  A tensor may be a view with a row stride >= N and unit column stride: it is
        passed with its stride, not copied.  It must be complete on the current stream, is never written, and the Batch
        keeps a reference until close()."""
        import torch
        L = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("squarna_amd needs an AMD GPU (MI355X / gfx950): torch.cuda is not "
                               "available and there is no CPU fallback")
        self.torch = torch
        self.L = L
        if isinstance(prepared, PackedRows):
            # an alignment's rows as arrays (no per-row records: the batch computes, it has no results to decode)
            pk, prepared = prepared, None
            nseq = pk.nseq
            self.prepared = None
            self.seq_off, self.codes, self.flags, self.reacts, self.rbp_off, self.rbps = pk.seq_off, pk.codes, pk.flags, pk.reacts, pk.rbp_off, pk.rbps
        else:
            nseq = self._host_arrays(prepared)
        self._pool_lists = bool(pool_lists)
        self._job_lists(nseq, psets_per_record)
        self._describe(interchainonly, ext, mul, max_structs, cand_per_nt, fp32, bpp, mul_shared, bpp_dev)
        self._create_on_device(device)

    def _host_arrays(self, prepared):
        """The per-position arrays of the batch from a list of Prepared records; the number of records."""
        self.prepared = prepared
        nseq = len(prepared)
        self.seq_off = np.zeros(nseq + 1, np.int32)
        np.cumsum(np.fromiter((len(p.shortseq) for p in prepared), np.int64, nseq), out=self.seq_off[1:])
        ltot = int(self.seq_off[-1])
        self.codes = np.frombuffer(encode_seq(''.join(p.shortseq for p in prepared)), np.uint8).copy() \
            if ltot else np.zeros(1, np.uint8)
        self.flags = np.zeros(max(ltot, 1), np.uint8)
        # no record with reactivities: the library takes NULL for "0.5 everywhere" (8 bytes per position neither filled,
        # scanned nor uploaded)
        self.reacts = None if all(p.plain_reacts for p in prepared) else np.full(max(ltot, 1), 0.5, np.float64)
        self.rbp_off = np.zeros(nseq + 1, np.int32)
        rbps = []
        # (most records of a big input are plain: only the ones with restraints or reactivities take the loop)
        for k, p in enumerate(prepared):
            if p.plain_reacts and not (p.rbps or p.rxs or p.rlefts or p.rrights):
                continue
            o = int(self.seq_off[k])
            for i in p.rxs:
                self.flags[o + i] |= 1
            for i in p.rlefts:
                self.flags[o + i] |= 2
            for i in p.rrights:
                self.flags[o + i] |= 4
            if not p.plain_reacts:
                self.reacts[o:o + len(p.shortseq)] = p.shortreacts
            if p.rbps:
                rbps.extend(p.rbps)
                self.rbp_off[k + 1] = len(p.rbps)
        np.cumsum(self.rbp_off, out=self.rbp_off)
        self.rbps = np.array(rbps, np.int32).reshape(-1) if rbps else np.zeros(2, np.int32)
        return nseq

    def _job_lists(self, nseq, psets_per_record):
        """The batch's jobs, one per (record, paramset of its list), and its unique paramsets (by identity)."""
        uniq, self.psets_py = {}, []
        first = psets_per_record[0] if nseq else []
        if nseq and all(pl is first for pl in psets_per_record):
            # one configuration for every record (the usual case): the job lists are a repeat / tile
            idx = []
            for ps in first:
                if id(ps) not in uniq:
                    uniq[id(ps)] = len(self.psets_py)
                    self.psets_py.append(ps)
                idx.append(uniq[id(ps)])
            npl = len(first)
            self.job_seq = np.repeat(np.arange(nseq, dtype=np.int32), npl)
            self.job_pset = np.tile(np.array(idx, np.int32), nseq)
            self.seq_jobs = None                                     # (k -> range(k * npl, (k + 1) * npl), formed on demand)
            self._npl = npl
        else:
            job_seq, job_pset = [], []
            self.seq_jobs = []
            for k, plist in enumerate(psets_per_record):
                mine = []
                for ps in plist:
                    if id(ps) not in uniq:
                        uniq[id(ps)] = len(self.psets_py)
                        self.psets_py.append(ps)
                    mine.append(len(job_seq))
                    job_seq.append(k)
                    job_pset.append(uniq[id(ps)])
                self.seq_jobs.append(mine)
            self.job_seq = np.array(job_seq, np.int32)
            self.job_pset = np.array(job_pset, np.int32)
        self.psets_c = (_lib.ParamSet * len(self.psets_py))(*[_pset_struct(p) for p in self.psets_py])
        self.njobs = len(self.job_seq)
        self.nseq = nseq

    def _describe(self, interchainonly=False, ext=None, mul=None, max_structs=0, cand_per_nt=0, fp32=True, bpp=None, mul_shared=None,
                  bpp_dev=None):
        """Fills self.desc (sq_batch_desc) from the host arrays and the job lists: no device work -- torch is touched only for
        mul_shared's matrix, which lives on the GPU."""
        nseq, njobs, ltot = self.nseq, self.njobs, int(self.seq_off[-1])
        d = _lib.BatchDesc()
        d.nseq = nseq
        d.seq_off = _ptr(self.seq_off, C.POINTER(C.c_int32))
        d.codes = _ptr(self.codes, C.POINTER(C.c_uint8))
        d.flags = _ptr(self.flags, C.POINTER(C.c_uint8))
        d.reacts = _ptr(self.reacts, C.POINTER(C.c_double)) if self.reacts is not None else None
        d.rbp_off = _ptr(self.rbp_off, C.POINTER(C.c_int32))
        d.rbps = _ptr(self.rbps, C.POINTER(C.c_int32))
        d.npset = len(self.psets_py)
        d.psets = self.psets_c
        d.njobs = njobs
        d.job_seq = _ptr(self.job_seq, C.POINTER(C.c_int32))
        d.job_pset = _ptr(self.job_pset, C.POINTER(C.c_int32))
        self._keep = []

        def ptr_array(mats):
            arr = (C.c_void_p * njobs)()
            for j, m in enumerate(mats):
                if m is not None:
                    m = np.ascontiguousarray(m, dtype=np.float64)
                    self._keep.append(m)
                    arr[j] = m.ctypes.data
            return arr

        if ext is not None:
            self._eb = ptr_array([e[0] if e is not None else None for e in ext])
            self._es = ptr_array([e[1] if e is not None else None for e in ext])
            d.ext_bool = C.cast(self._eb, C.POINTER(C.c_void_p))
            d.ext_score = C.cast(self._es, C.POINTER(C.c_void_p))
        if mul is not None:
            self._mul = ptr_array(mul)
            d.mul_score = C.cast(self._mul, C.POINTER(C.c_void_p))
        if mul_shared is not None:
            import torch
            M, cols, maxabs = mul_shared
            assert M.is_cuda and M.dtype == torch.float64 and M.dim() == 2 and M.shape[0] == M.shape[1] and M.is_contiguous()
            self._mul_M = M
            self._mul_cols = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int32) for c in cols])
                                                  if ltot else np.zeros(1, np.int32), dtype=np.int32)
            assert len(self._mul_cols) == max(ltot, 1)
            self._mul_flag = np.ones(max(njobs, 1), np.uint8)
            d.mul_matrix_dev = C.c_void_p(M.data_ptr())
            d.mul_L = int(M.shape[0])
            d.mul_cols = _ptr(self._mul_cols, C.POINTER(C.c_int32))
            d.mul_shared = _ptr(self._mul_flag, C.POINTER(C.c_uint8))
            d.mul_maxabs = float(maxabs)
        if bpp is not None:                                          # per job: (bppm/max)**|bpp| or None (SQRNdbnseq.py:350-364)
            self._bpp = ptr_array(bpp)
            d.bpp_term = C.cast(self._bpp, C.POINTER(C.c_void_p))
        self._bpp_dev = None
        if bpp_dev is not None and any(m is not None for m in bpp_dev):   # per record: the probabilities themselves, on the device
            if len(bpp_dev) != nseq:
                raise ValueError("bpp_dev: %d matrices for %d records" % (len(bpp_dev), nseq))
            self._bpp_dev = list(bpp_dev)                            # (kept until close(): the create's kernels read them)
            self._bpp_ptr = (C.c_void_p * nseq)()
            self._bpp_ld = np.zeros(max(nseq, 1), np.int32)
            for k, m in enumerate(bpp_dev):
                n = int(self.seq_off[k + 1] - self.seq_off[k])
                self._bpp_ld[k] = n
                if m is not None:
                    check_bpp_matrix(m, n, "bpp_dev[%d]" % k)
                    self._bpp_ptr[k] = m.data_ptr()
                    self._bpp_ld[k] = int(m.stride(0)) if n > 1 else n
            d.bpp_matrix_dev = C.cast(self._bpp_ptr, C.POINTER(C.c_void_p))
            d.bpp_matrix_ld = _ptr(self._bpp_ld, C.POINTER(C.c_int32))
        d.interchainonly = int(bool(interchainonly))
        d.max_structs = int(max_structs)
        d.cand_per_nt = int(cand_per_nt)
        d.batch_flags = (0 if fp32 else _lib.BATCH_NO_FP32) | (_lib.BATCH_POOL_LISTS if self._pool_lists else 0)
        self.desc = d

    def workspace_bytes(self):
        """Bytes of device workspace the described batch needs (sq_batch_workspace_bytes: arithmetic, no device)."""
        nbytes = C.c_size_t(0)
        _lib.check(_lib.load().sq_batch_workspace_bytes(C.byref(self.desc), C.byref(nbytes)))
        return nbytes.value

    def _create_on_device(self, device):
        """The workspace tensor and the device batch (sq_batch_create) of the described batch."""
        torch, L = self.torch, self.L
        nbytes = self.workspace_bytes()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.workspace = torch.empty(workspace_size_class(nbytes + 256), dtype=torch.uint8, device=self.device)
        base = self.workspace.data_ptr()
        aligned = (base + 255) // 256 * 256
        self.stream = torch.cuda.current_stream(self.device)
        h = C.c_void_p()
        _lib.check(L.sq_batch_create(C.byref(h), C.byref(self.desc), C.c_void_p(aligned),
                                     C.c_size_t(nbytes), C.c_void_p(self.stream.cuda_stream)))
        self.h = h
        self._refs = None

    # -- lifecycle
    def close(self):
        if getattr(self, "h", None):
            self.L.sq_batch_destroy(self.h)
            self.h = None
            self.workspace = None
            self._bpp_dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- a-1
    def fill(self):
        _lib.check(self.L.sq_bpmatrix_fill(self.h))

    def bpmatrix(self, job):
        n = int(self.seq_off[self.job_seq[job] + 1] - self.seq_off[self.job_seq[job]])
        b = np.zeros((n, n)); s = np.zeros((n, n))
        _lib.check(self.L.sq_bpmatrix_read(self.h, job, _ptr(b), _ptr(s)))
        return b, s

    # -- a-2..a-6
    def optimal(self, struct_job, struct_stems, subopt=None, mode=0, out_cap=None, as_array=False):
        """struct_stems: list (per structure) of (i, j, len) tuples -> list of lists of
        (i, j, len, bpscore, finalscore)."""
        ns = len(struct_job)
        sj = np.array(struct_job, np.int32)
        off = np.zeros(ns + 1, np.int32)
        flat = []
        for k, st in enumerate(struct_stems):
            flat.extend(st)
            off[k + 1] = len(flat)
        stems = (_lib.Stem * max(len(flat), 1))()
        for k, t in enumerate(flat):
            stems[k].i, stems[k].j, stems[k].len = int(t[0]), int(t[1]), int(t[2])
        so = np.array(subopt if subopt is not None else [1.0] * ns, np.float64)
        if out_cap is None:
            out_cap = 1 << 16 if mode == 0 else 1 << 20
        out = (_lib.Stem * out_cap)()
        out_off = np.zeros(ns + 1, np.int32)
        _lib.check(self.L.sq_optimal_stems(self.h, ns, _ptr(sj), _ptr(off), stems, _ptr(so), mode,
                                           out, out_cap, _ptr(out_off)))
        if as_array:                                                   # structured views, no per-stem objects
            arr = np.frombuffer(out, dtype=_STEM_DT, count=int(out_off[ns])).copy()
            return [arr[out_off[k]:out_off[k + 1]] for k in range(ns)]
        res = []
        for k in range(ns):
            res.append([(out[q].i, out[q].j, out[q].len, out[q].bpscore, out[q].finscore)
                        for q in range(out_off[k], out_off[k + 1])])
        return res

    # -- alignment step 1
    def align_accumulate(self, jobs, cols_per_job, matrix):
        """Adds the stem scores of the listed jobs, in order, into the device L x L fp64 tensor `matrix`
        through the gap maps cols_per_job[k] (unaligned index -> column); SQRNdbnali.py:233-237."""
        L = int(matrix.shape[0])
        assert matrix.dtype == self.torch.float64 and matrix.is_contiguous() and tuple(matrix.shape) == (L, L)
        ja = np.array(jobs, np.int32)
        off = np.zeros(len(jobs) + 1, np.int32)
        for k, c in enumerate(cols_per_job):
            off[k + 1] = off[k] + len(c)
        cols = np.concatenate([np.asarray(c, np.int32) for c in cols_per_job]) if len(jobs) else np.zeros(1, np.int32)
        cols = np.ascontiguousarray(cols, np.int32)
        _lib.check(self.L.sq_align_accumulate(self.h, len(jobs), _ptr(ja), _ptr(off), _ptr(cols), L,
                                              C.c_void_p(matrix.data_ptr())))

    def align_accumulate_packed(self, pk, matrix):
        """align_accumulate for every row of a PackedRows batch, its gap maps as they are (no per-row lists)."""
        L = int(matrix.shape[0])
        assert matrix.dtype == self.torch.float64 and matrix.is_contiguous() and tuple(matrix.shape) == (L, L)
        ja = np.arange(pk.nseq, dtype=np.int32)
        _lib.check(self.L.sq_align_accumulate(self.h, pk.nseq, _ptr(ja), _ptr(pk.seq_off), _ptr(pk.cols), L,
                                              C.c_void_p(matrix.data_ptr())))

    # -- entropy mode as data
    def entropy_rows(self, jobs, pos_off, position, mean, nstems, scratch):
        """The row entropies of the listed jobs' stem matrices (sq_entropy_rows; SQRNdbnseq.py:520-545): list entry k's N values
        go to position[pos_off[k] ..], their mean to mean[k], the number of its stems to nstems[k].  pos_off int64[len(jobs) + 1],
        position / mean float64, nstems int32, scratch uint8 (sq_entropy_scratch bytes for the jobs' N^2 cells): CUDA tensors of
        the caller on the batch's device, complete on the batch's stream.  The results are complete when the call returns."""
        torch = self.torch
        assert pos_off.dtype == torch.int64 and pos_off.numel() == len(jobs) + 1 and nstems.dtype == torch.int32
        assert position.dtype == torch.float64 and mean.dtype == torch.float64 and scratch.dtype == torch.uint8
        assert all(t.is_cuda and t.is_contiguous() for t in (pos_off, position, mean, nstems, scratch))
        assert mean.numel() >= len(jobs) and nstems.numel() >= len(jobs)
        ja = np.array(jobs, np.int32)
        _lib.check(self.L.sq_entropy_rows(self.h, len(jobs), _ptr(ja), C.c_void_p(pos_off.data_ptr()), C.c_void_p(position.data_ptr()),
                                          C.c_void_p(mean.data_ptr()), C.c_void_p(nstems.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                          C.c_size_t(scratch.numel())))

    # -- a-8 / a-9 / Nussinov
    def run_algo(self, jobs, algo, levellimit=None, out_cap=1 << 16):
        """RunAlgo (SQRNdbnseq.py:548-595) for the listed jobs under 'E', 'H' or 'N':
        list (per job) of (i, j, len, score, score)."""
        nj = len(jobs)
        ja = np.array(jobs, np.int32)
        out = (_lib.Stem * out_cap)()
        off = np.zeros(nj + 1, np.int32)
        _lib.check(self.L.sq_run_algos(self.h, nj, _ptr(ja), _lib.ALGO_BITS[algo],
                                       -1 if levellimit is None else int(levellimit), out, out_cap, _ptr(off)))
        return [[(out[q].i, out[q].j, out[q].len, out[q].bpscore, out[q].finscore)
                 for q in range(off[k], off[k + 1])] for k in range(nj)]

    def set_inflight(self, n):
        """Tell the batch that n batches are folded at the same time from threads of the caller (sq_batch_set_inflight)."""
        _lib.check(self.L.sq_batch_set_inflight(self.h, int(n)))

    # -- a-7 + a-10
    def fold(self, **opts):
        """priority: per record, set of local paramset indices (or one set for all)."""
        o, ref_off, rp, has = self._fold_args(**opts)
        _lib.check(self.L.sq_fold(self.h, C.byref(o), _ptr(ref_off), _ptr(rp), _ptr(has)))

    def limit_results(self, k):
        """The result getters show only the first k structures of every record (sq_result_limit; 0 = all)."""
        _lib.check(self.L.sq_result_limit(self.h, int(k or 0)))

    @property
    def fold_peak_structs(self):
        """Most structures any round of the last fold held at once (sq_fold_peak_structs; 0: host-driven loop)."""
        return int(self.L.sq_fold_peak_structs(self.h))

    @property
    def fold_driver(self):
        """Driver of the last fold's greedy pool loop (sq_fold_driver): 0 host loop, 1 chained rounds, 2 device pools,
        3 device pools repeated by the host loop."""
        return int(self.L.sq_fold_driver(self.h))

    @property
    def fold_paths(self):
        """Bit 0: the last fold's ranking tail ran on the device, bit 1: RunAlgo's edge lists and filters did (sq_fold_paths)."""
        return int(self.L.sq_fold_paths(self.h))

    def _fold_args(self, poollim=1000, conslim=1, toplim=5, hardrest=False, rankbydiff=False,
                   rankby=(0, 2, 1), levellimit=None, algos=frozenset(), priority=None):
        o = _lib.FoldOpts()
        o.poollim, o.conslim, o.toplim = int(poollim), int(conslim), int(toplim)
        o.hardrest, o.rankbydiff = int(bool(hardrest)), int(bool(rankbydiff))
        for t in range(3):
            o.rankby[t] = int(rankby[t])
        o.levellimit = -1 if levellimit is None else int(levellimit)
        o.algos = sum(_lib.ALGO_BITS[a] for a in algos)
        mask = 0
        for p in (priority or ()):
            mask |= 1 << int(p)
        o.priority_mask = mask
        if self._refs is None:                       # reference pairs are static per batch
            ref_off = np.zeros(self.nseq + 1, np.int32)
            has = np.zeros(max(self.nseq, 1), np.uint8)
            dbns = [p.shortdbn or "" for p in self.prepared]
            text = "".join(dbns)
            if text.isascii():
                # DBNToPairs (SQRNdbnseq.py:172-207) for all known structures in one library call (sq_dbn_pairs)
                off = offsets([len(x) for x in dbns])
                poff = np.zeros(self.nseq + 1, np.int64)
                rp = np.zeros(max(len(text), 2), np.int32)                  # (a line of n characters has at most n / 2 pairs)
                _lib.check(self.L.sq_dbn_pairs(text.encode("ascii"), _ptr(off), self.nseq, _ptr(rp), len(rp) // 2, _ptr(poff)))
                ref_off[:] = poff
                has[:self.nseq] = [1 if x else 0 for x in dbns]
                rp = rp[:max(2 * int(poff[-1]), 2)]
            else:                                                        # (bracket letters beyond ASCII: the Python form)
                refs = []
                for k, p in enumerate(self.prepared):
                    if p.shortdbn:
                        has[k] = 1
                        if p.refpairs is None:
                            p.refpairs = DBNToPairs(p.shortdbn)
                        refs.extend(p.refpairs)
                    ref_off[k + 1] = len(refs)
                rp = np.array(refs, np.int32).reshape(-1) if refs else np.zeros(2, np.int32)
            self._refs = (ref_off, rp, has)
        ref_off, rp, has = self._refs
        return o, ref_off, rp, has

    def result(self, k, with_ref=False):
        """SQRNdbnseq return tuple of record k (SQRNdbnseq.py:1285-1286); with_ref: (tuple, reference scores or None)."""
        L = self.L
        nbytes = L.sq_result_pack_size(self.h, k)
        buf = bytearray(nbytes)
        cbuf = (C.c_char * nbytes).from_buffer(buf)
        _lib.check(L.sq_result_pack(self.h, k, cbuf, nbytes))
        out = self._unpack(k, buf, 0)
        return out if with_ref else out[0]

    def results_all(self):
        """[(SQRNdbnseq tuple, reference scores or None)] for every record, from ONE sq_result_pack_all call: the whole
        dot-bracket rows come as ASCII text from one sq_result_dbn_all call, headers / scores / masks through numpy views; a
        record then costs a few slices (records with gap columns, separators or > 30 pseudoknot levels take the per-record
        path)."""
        buf, off = self.pack_all()
        raw = buf.tobytes()
        # the dot-bracket rows of every record as ASCII, formed by the library in one call
        tbytes = int(self.L.sq_result_dbn_all_size(self.h))
        tbuf = np.zeros(max(tbytes, 8), np.uint8)
        toff = np.zeros(self.nseq + 1, np.int64)
        deep = np.zeros(max(self.nseq, 1), np.uint8)
        _lib.check(self.L.sq_result_dbn_all(self.h, _ptr(tbuf), tbytes, _ptr(toff), _ptr(deep)))
        text_all = tbuf[:tbytes].tobytes().decode('latin-1')
        toffl, deepl = toff.tolist(), deep.tolist()
        # headers, metrics, scores and masks of all records through numpy views (the records start 8-byte aligned)
        q = np.frombuffer(raw, '<i8', len(raw) // 8)
        qu = np.frombuffer(raw, '<u8', len(raw) // 8)               # paramset masks: bit 63 may be set (64 paramsets)
        d = np.frombuffer(raw, '<f8', len(raw) // 8)
        b8 = (off[:-1] // 8).astype(np.int64)
        ns_a, n_a, ref_a = q[b8].tolist(), q[b8 + 1].tolist(), q[b8 + 2].tolist()
        met_a = d[b8[:, None] + (4 + np.arange(16))].tolist()
        b8l = b8.tolist()
        nan6, nan7 = [np.nan] * 6, [np.nan] * 7
        out = []
        for k in range(self.nseq):
            p = self.prepared[k]
            if p.gapidx or p.sepidx or deepl[k]:
                out.append(self._unpack(k, raw, int(off[k])))
                continue
            ns, n, sb = ns_a[k], n_a[k], b8l[k] + 20
            sc = d[sb:sb + 3 * ns].tolist()
            mk = qu[sb + 3 * ns:sb + 4 * ns].tolist()
            t0 = toffl[k]                                          # the record's rows in text_all
            preds = [(text_all[t0 + (t + 1) * n:t0 + (t + 2) * n], tuple(sc[3 * t:3 * t + 3]),
                      list(_MASK_IDS[mk[t]]) if mk[t] < 16 else [b for b in range(64) if (mk[t] >> b) & 1]) for t in range(ns)]
            if ref_a[k]:
                met = met_a[k]
                out.append(((text_all[t0:t0 + n], preds, _metrics(met[:6]), _metrics(met[6:12]) + [int(met[12])]), tuple(met[13:16])))
            else:
                out.append(((text_all[t0:t0 + n], preds, list(nan6), list(nan7)), None))
        return out

    def _unpack(self, k, buf, base):
        return unpack_result(self.prepared[k], buf, base)

    def write_blocks(self, names, seqs, reactlines, restrs, refs, nameset, psnames, conslim, outplim):
        """The output blocks of RunSQRNdbnseq (SQRNdbnseq.py:1301-1406) for every record, formed by the library from the
        packed results of the last fold (sq_write_blocks): list of str, None for a record the library leaves to the
        caller (bracket levels beyond ASCII).  None when the batch's results are not packed (host tail) or some input
        line is not ASCII: the caller formats from results_all()."""
        if not (self.fold_paths & 1):
            return None
        fields = []
        for col in (names, seqs, reactlines, restrs, refs):
            if all(x is None or x == "" for x in col):
                fields.append(None)
                continue
            text = "\n".join(x or "" for x in col)
            if not text.isascii() or "\0" in text:                    # (the library reads NUL-terminated ASCII lines)
                return None
            fields.append(text.encode("ascii"))
        if fields[0] is None or fields[1] is None:
            return None
        d = _lib.BlockDesc()
        d.nrec = self.nseq
        d.names, d.seqs, d.reacts, d.restr, d.refs = fields
        ns = np.ascontiguousarray(nameset, np.int32)
        d.nameset = _ptr(ns, C.POINTER(C.c_int32))
        if not all(nm.isascii() and "\0" not in nm and "\n" not in nm for x in psnames for nm in x):
            return None                                               # (paramset names the library cannot carry: the caller formats)
        pn = [("\n".join(x)).encode("ascii") for x in psnames]
        arr = (C.c_char_p * len(pn))(*pn)
        d.psnames = arr
        d.nsets, d.conslim, d.outplim = len(pn), int(conslim), int(outplim)
        off = np.zeros(self.nseq + 1, np.int64)
        skipped = np.zeros(max(self.nseq, 1), np.uint8)
        cap = int(self.L.sq_result_dbn_all_size(self.h)) + sum(len(f) for f in fields if f) * 2 + 200 * self.nseq * (2 + int(outplim)) + 4096
        for _ in range(2):
            buf = np.empty(cap, np.uint8)                              # (no zero fill: the library writes what it reports)
            n = int(self.L.sq_write_blocks(self.h, C.byref(d), _ptr(buf), cap, _ptr(off), _ptr(skipped)))
            if n >= 0:
                break
            if n > -16:
                _lib.check(int(n))
            cap = -n
        text = str(memoryview(buf)[:n], "ascii")
        if not skipped[:self.nseq].any():
            return _Blocks(text, off)
        o = off.tolist()
        sk = skipped.tolist()
        return [None if sk[k] else text[o[k]:o[k + 1]] for k in range(self.nseq)]

    def pack_all(self, copy=False):
        """(uint8 array, int64 offsets[nseq + 1]): the packed results of every record (sq_result_view, else sq_result_pack_all)
        -- the payload of the multi-GPU result gather.  The array is a view of a buffer the batch reuses (copy=True: of the
        batch's own pack buffer, never of the library's pinned one)."""
        # the records where the device tail wrote them (the library's pinned buffer): no copy.  The views are valid until the
        # batch folds again or closes -- every caller below turns them into bytes / tuples before that
        pb, po, nb = C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = self.L.sq_result_view(self.h, C.byref(pb), C.byref(po), C.byref(nb))
        if rc == 0 and not copy:
            n = max(int(nb.value), 0)
            buf = np.ctypeslib.as_array((C.c_uint8 * max(n, 1)).from_address(pb.value))[:n]
            off = np.ctypeslib.as_array((C.c_int64 * (self.nseq + 1)).from_address(po.value))
            return buf, off
        if rc < 0:
            _lib.check(rc)
        nbytes = int(self.L.sq_result_pack_all_size(self.h))
        # the batch keeps its pack buffer (fresh pages for tens of MB per call cost more than the packing itself); the
        # returned view is valid until the next pack_all of this batch
        buf = getattr(self, "_packbuf", None)
        if buf is None or buf.size < max(nbytes, 8):
            buf = self._packbuf = np.empty(max(nbytes, 8) + (max(nbytes, 8) >> 3), np.uint8)
        off = np.zeros(self.nseq + 1, np.int64)
        _lib.check(self.L.sq_result_pack_all(self.h, _ptr(buf), nbytes, _ptr(off)))
        return buf[:nbytes], off

    def result_tensors(self):
        """The last fold's results as torch tensors on the batch's device (sq_result_pairs_dev): dict of
        partner int32[cells], scores float64[rows, 3], pset_mask int64[rows] (the uint64 masks' bit patterns),
        metrics float64[nseq, 16], row_off / cell_off int64[nseq + 1] -- the layout of include/squarna_hip.h, gap-free
        coordinates.  None when the results are not in the device tail's form (the host tail ran): pack_all then.
        Enqueued on the batch's stream; the tensors are the caller's and outlive the batch."""
        torch = self.torch
        rows, cells = C.c_int64(), C.c_int64()
        rc = self.L.sq_result_pairs_size(self.h, C.byref(rows), C.byref(cells))
        if rc == 1:
            return None
        _lib.check(rc)
        rows, cells = int(rows.value), int(cells.value)
        with torch.cuda.stream(self.stream):
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
            # (at least one element each: an empty tensor has no address to pass)
            out = dict(partner=new(max(cells, 1), torch.int32)[:cells], scores=new((max(rows, 1), 3), torch.float64)[:rows],
                       pset_mask=new(max(rows, 1), torch.int64)[:rows], metrics=new((max(self.nseq, 1), 16), torch.float64)[:self.nseq],
                       row_off=new(self.nseq + 1, torch.int64), cell_off=new(self.nseq + 1, torch.int64))
        rc = self.L.sq_result_pairs_dev(self.h, out["partner"].data_ptr(), cells, out["scores"].data_ptr(), out["pset_mask"].data_ptr(),
                                        rows, out["metrics"].data_ptr(), out["row_off"].data_ptr(), out["cell_off"].data_ptr(),
                                        C.c_void_p(self.stream.cuda_stream))
        if rc == 1:
            return None
        _lib.check(rc)
        return out

    def result_counts(self):
        """(nstruct, lengths) of every record as host int64 arrays -- the sizes behind result_tensors' offsets, read from the
        headers of the packed records (no device round trip)."""
        buf, off = self.pack_all()
        q = np.frombuffer(buf, '<i8', len(buf) // 8)
        return q[off[:-1] // 8].astype(np.int64), np.diff(self.seq_off).astype(np.int64)

    def detach_packed(self):
        """The packed results of every record as read-only memoryviews of the library's pinned buffer, which leaves the batch
        with them (sq_result_detach): no copy; the buffer goes back to the library when the last view is dropped.  None when
        the records are not in that form (the host tail ran): pack_all then."""
        pb, po, nb = C.c_void_p(), C.c_void_p(), C.c_int64()
        if self.L.sq_result_view(self.h, C.byref(pb), C.byref(po), C.byref(nb)) != 0:
            return None
        off = np.ctypeslib.as_array((C.c_int64 * (self.nseq + 1)).from_address(po.value)).tolist()
        if self.L.sq_result_detach(self.h, C.byref(pb), C.byref(nb)) != 0:
            return None
        arr = (C.c_uint8 * max(int(nb.value), 1)).from_address(pb.value)
        arr._owner = _PinnedOwner(self.L, pb.value)
        mv = memoryview(arr).toreadonly()
        return [mv[off[k]:off[k + 1]] for k in range(self.nseq)]

    def evals(self, k):
        return int(self.L.sq_result_evals(self.h, k))

    # -- measurement
    def profile(self, on=True):
        self.L.sq_profile_enable(self.h, int(on))

    def profile_reset(self):
        self.L.sq_profile_reset(self.h)

    def mwm_counters(self):
        """Blossom kernel work since the last profile_reset: dict(graphs, passes, and the critical graph's
        max_passes, max_events, n, m) -- sq_profile_counters."""
        out = (C.c_int64 * 6)()
        _lib.check(self.L.sq_profile_counters(self.h, 4, out))
        return dict(zip(("graphs", "passes", "max_passes", "max_events", "n", "m"), [int(x) for x in out]))

    def profile_get(self, kernel):
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(self.L.sq_profile_get(self.h, kernel, C.byref(ms), C.byref(n), C.byref(by)))
        return ms.value, n.value, by.value


class _PinnedOwner:
    """Returns a detached pinned buffer to the library when the last view of it is gone (Batch.detach_packed)."""

    def __init__(self, L, ptr):
        self.L, self.ptr = L, ptr

    def __del__(self):
        try:
            self.L.sq_buffer_release(C.c_void_p(self.ptr))
        except Exception:                                            # (interpreter shutdown)
            pass


def fold_concurrently(batches, reps=1, **opts):
    """Fold several batches at the same time (sq_fold_concurrent: one host thread per batch inside the library):
    while one batch's host code books a round, the kernels of the others keep the GPU busy.  Batches are
    independent, so the results are the ones of folding them one after the other.  reps > 1: every batch is folded
    that many times back to back without a barrier between the repetitions (sq_fold_concurrent_n)."""
    args = [b._fold_args(**opts) for b in batches]
    n = len(batches)
    hs = (C.c_void_p * n)(*[b.h for b in batches])
    offs = (C.c_void_p * n)(*[a[1].ctypes.data for a in args])
    rps = (C.c_void_p * n)(*[a[2].ctypes.data for a in args])
    has = (C.c_void_p * n)(*[a[3].ctypes.data for a in args])
    if reps > 1:
        _lib.check(batches[0].L.sq_fold_concurrent_n(hs, n, C.byref(args[0][0]), offs, rps, has, int(reps)))
    else:
        _lib.check(batches[0].L.sq_fold_concurrent(hs, n, C.byref(args[0][0]), offs, rps, has))
