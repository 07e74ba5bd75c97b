"""``Fold``: bulk prediction that returns data instead of text.

``Predict`` prints the reference's blocks and ``SQRNdbnseq`` returns one record's tuple; ``Fold`` takes the same inputs and
prediction keywords as ``Predict`` and returns a :class:`FoldResult`: pair tables, scores, paramset masks and metrics of
every record as torch tensors.  With the GPU engine the tables are formed by a kernel from the ranking tail's scratch
(``sq_result_pairs_dev``) and never leave the device; an engine without ``fold_tensors`` (the tests' CPU engine) gets the
same object built on the CPU from its ``fold_records`` tuples.  ``Fold`` prints nothing.
"""
import contextlib

import numpy as np

from . import api as _api
from . import engine as _engine
from .engine import _TABLES
from .core import resolve_priority
from .dbn import DBNToPairs, PairsToDBN, GAPS, SEPS, gap_mask
from .options import batches, check_sources, configs_by_length, input_records, pick, prediction_options
from .results import TensorResult
from .rows import offsets, partner_row, row_pairs


def _seg_copy(torch, dst, dst_start, src, src_start, seg_len, colmap=None, map_start=None):
    """dst[dst_start[s] + t] = src[src_start[s] + t] for every segment s and t < seg_len[s], as torch index operations on
    the tensors' device (the per-segment numbers are host int64 arrays, uploaded once).  With colmap (a device tensor)
    and map_start, segment s is a row of partners that moves into other coordinates: entry t goes to column
    colmap[map_start[s] + t] and a partner v >= 0 becomes colmap[map_start[s] + v]."""
    total = int(seg_len.sum())
    if not total:
        return
    dev = src.device
    cum = offsets(seg_len)[:-1]
    cols = [dst_start, src_start - cum, cum, seg_len] + ([map_start] if colmap is not None else [])
    meta = torch.from_numpy(np.stack(cols)).to(dev)
    seg = torch.repeat_interleave(torch.arange(len(seg_len), device=dev), meta[3], output_size=total)
    flat = torch.arange(total, device=dev)
    val = src[flat + meta[1][seg]]
    t = flat - meta[2][seg]
    if colmap is None:
        dst[meta[0][seg] + t] = val
        return
    base = meta[4][seg]
    moved = colmap[base + val.clamp(min=0).long()]
    dst[meta[0][seg] + colmap[base + t]] = torch.where(val >= 0, moved, torch.full_like(moved, -1)).to(dst.dtype)


def _offsets(nstruct, lengths):
    """(row_off, cell_off) of the tables' layout, int64[R + 1] each."""
    return offsets(nstruct), offsets((1 + nstruct) * lengths)


class FoldResult(TensorResult):
    """Predictions of ``Fold`` for R records.

    Host lists: ``names``, ``sequences`` (as given), ``paramset_names`` (per record: the names its mask bits stand for).
    Torch tensors (``device``: where they live): ``lengths`` and ``nstruct`` int64[R]; ``row_off`` / ``cell_off``
    int64[R + 1]; ``partner`` int32[cells] -- record r has 1 + nstruct[r] rows of lengths[r] entries from
    cell_off[r] on, row 0 the consensus, rows 1.. the structures in rank order, entry i the 0-based partner of position i
    or -1; ``scores`` float64[rows, 3] (total, structure, reactivity) and ``pset_mask`` int64[rows] (bit p: paramset p
    produced the structure; the bit pattern of the library's uint64) for the structure rows, record r from row_off[r] on;
    ``metrics`` float64[R, 16]: TP FP FN FS PR RC of the consensus, the same + rank of the best of the top structures, the
    known structure's three scores (NaN without one).  ``source``: "device", "host" or "mixed" -- where the tables
    were formed (HipEngine.fold_tensors).

    Positions count the sequence AS GIVEN: gap columns are -1 and partners point at input columns, so ``dbn(r, k)`` is the
    string ``SQRNdbnseq`` returns."""

    _TENSORS = _TABLES + ("lengths", "nstruct")

    def __init__(self, names, sequences, paramset_names, tables, nstruct, lengths, source):
        import torch
        self.names, self.sequences, self.paramset_names, self.source = names, sequences, paramset_names, source
        self.partner, self.scores, self.pset_mask, self.metrics, self.row_off, self.cell_off = (tables[k] for k in _TABLES)
        # the host's copy of the sizes: the helpers below index with it, no device round trip
        self._nstruct, self._lengths = np.asarray(nstruct, np.int64), np.asarray(lengths, np.int64)
        self._row_off, self._cell_off = _offsets(self._nstruct, self._lengths)
        self.lengths, self.nstruct = (torch.from_numpy(a).to(self.partner.device) for a in (self._lengths, self._nstruct))

    def __len__(self):
        return len(self.names)

    def _row(self, r, k):
        """Row k of record r (0: the consensus) as a host int32 array."""
        if not 0 <= k <= self._nstruct[r]:
            raise IndexError("record %d has %d structures" % (r, self._nstruct[r]))
        n, o = int(self._lengths[r]), int(self._cell_off[r])
        return self.partner[o + k * n:o + (k + 1) * n].cpu().numpy()

    def pairs(self, r, k):
        """Sorted (i, j) pairs, i < j, of structure k (0-based, rank order) of record r."""
        return row_pairs(self._row(r, k + 1))

    def _dbn(self, r, row):
        seq = self.sequences[r]
        dbn = PairsToDBN(row_pairs(row), len(seq))
        return ''.join(seq[q] if seq[q] in SEPS else ch for q, ch in enumerate(dbn)) if any(ch in SEPS for ch in seq) else dbn

    def dbn(self, r, k):
        """Dot-bracket string of structure k of record r, as SQRNdbnseq returns it."""
        return self._dbn(r, self._row(r, k + 1))

    def consensus(self, r):
        """Dot-bracket string of record r's consensus."""
        return self._dbn(r, self._row(r, 0))

    def paramsets(self, r, k):
        """Names of the paramsets that produced structure k of record r."""
        if not 0 <= k < self._nstruct[r]:
            raise IndexError("record %d has %d structures" % (r, self._nstruct[r]))
        m = int(self.pset_mask[int(self._row_off[r]) + k]) & 0xFFFFFFFFFFFFFFFF
        names = self.paramset_names[r]
        return [names[p] for p in range(len(names)) if (m >> p) & 1]

    def to_padded(self, k=None):
        """int32[R, K, Lmax]: the first K structures (default: the most any record has) of every record, -1 where a
        record is shorter or has fewer; formed on the tensors' device."""
        import torch
        R = len(self.names)
        K = int(self._nstruct.max(initial=0)) if k is None else int(k)
        Lmax = int(self._lengths.max(initial=0))
        out = torch.full((R, K, Lmax), -1, dtype=torch.int32, device=self.device)
        take = np.minimum(self._nstruct, K)
        rec = np.repeat(np.arange(R), take)
        j = np.arange(len(rec)) - np.repeat(np.cumsum(take) - take, take)
        _seg_copy(torch, out.view(-1), (rec * K + j) * Lmax, self.partner, self._cell_off[rec] + (1 + j) * self._lengths[rec],
                  self._lengths[rec])
        return out

    def contact_map(self, r, k):
        """bool[L, L] of structure k of record r: True where i and j pair (symmetric), on the tensors' device."""
        import torch
        if not 0 <= k < self._nstruct[r]:
            raise IndexError("record %d has %d structures" % (r, self._nstruct[r]))
        n, o = int(self._lengths[r]), int(self._cell_off[r])
        row = self.partner[o + (k + 1) * n:o + (k + 2) * n].long()
        return row[:, None] == torch.arange(n, device=self.device)[None, :]


def _oracle_tables(results, seqs, keep):
    """The tables of an engine's fold_records tuples, on the CPU: the strings are in input coordinates already."""
    import torch
    partner, scores, masks, nstruct = [], [], [], []
    metrics = np.full((len(results), 16), np.nan)

    def row(dbn, n):
        return partner_row(DBNToPairs(dbn), n)
    for r, ((cons, preds, cm, bm), seq, ref) in enumerate(results):
        preds = preds[:keep]
        nstruct.append(len(preds))
        partner.append(row(cons, len(seq)))
        for dbn, sc, ids in preds:
            partner.append(row(dbn, len(seq)))
            scores.append([float(x) for x in sc])
            masks.append(sum(1 << p for p in ids))
        if ref is not None:
            metrics[r, :6], metrics[r, 6:13], metrics[r, 13:16] = cm, bm, ref
    tables = dict(partner=torch.from_numpy(np.concatenate(partner)),
                  scores=torch.from_numpy(np.array(scores, np.float64).reshape(-1, 3)),
                  pset_mask=torch.from_numpy(np.array(masks, np.uint64).astype(np.int64)),
                  metrics=torch.from_numpy(metrics))
    nstruct, lengths = np.array(nstruct, np.int64), np.array([len(s) for s in seqs], np.int64)
    tables["row_off"], tables["cell_off"] = (torch.from_numpy(a) for a in _offsets(nstruct, lengths))
    return tables, nstruct, lengths


def _join(parts, seqs):
    """(tables, nstruct, lengths) in input order and input coordinates from the engine calls' results.  parts: (tables,
    nstruct, lengths, records' places in the input, whether the coordinates are gap-free)."""
    import torch
    R = len(seqs)
    if len(parts) == 1 and (not parts[0][4] or not any(g in s for s in seqs for g in GAPS)):
        tables, ns, ln = parts[0][:3]                                # one call, no gap column: the kernel's output as it is
        return {k: tables[k] for k in _TABLES}, ns, ln
    nstruct, short, out_len = np.zeros(R, np.int64), np.zeros(R, np.int64), np.array([len(s) for s in seqs], np.int64)
    for _, ns, ln, idx, _ in parts:
        nstruct[idx], short[idx] = ns, ln
    row_off, cell_off = _offsets(nstruct, out_len)
    dev = parts[0][0]["partner"].device
    partner = torch.full((int(cell_off[-1]),), -1, dtype=torch.int32, device=dev)
    scores = torch.empty((int(row_off[-1]), 3), dtype=torch.float64, device=dev)
    masks = torch.empty(int(row_off[-1]), dtype=torch.int64, device=dev)
    metrics = torch.empty((R, 16), dtype=torch.float64, device=dev)
    for tables, ns, ln, idx, gapfree in parts:
        idx = np.asarray(idx, np.int64)
        rows = 1 + ns
        rec = np.repeat(np.arange(len(idx)), rows)                   # one segment per row of partners
        j = np.arange(len(rec)) - np.repeat(np.cumsum(rows) - rows, rows)
        src_cell = offsets(rows * ln)
        colmap = map_start = None
        if gapfree and any(short[k] != out_len[k] for k in idx):
            # where every gap-free position of the part's records lies in its input sequence
            pos = offsets(ln)
            cm = np.arange(int(pos[-1]), dtype=np.int64) - np.repeat(pos[:-1], ln)
            for q, k in enumerate(idx):
                if short[k] != out_len[k]:
                    cm[pos[q]:pos[q + 1]] = np.flatnonzero(~gap_mask(seqs[k]))
            colmap, map_start = torch.from_numpy(cm).to(dev), pos[rec]
        _seg_copy(torch, partner, cell_off[idx][rec] + j * out_len[idx][rec], tables["partner"], src_cell[rec] + j * ln[rec], ln[rec],
                  colmap, map_start)
        first = np.cumsum(ns) - ns                                   # the part's structure rows, record after record
        dst = torch.from_numpy(np.repeat(row_off[idx] - first, ns) + np.arange(int(ns.sum()))).to(dev)
        scores[dst], masks[dst] = tables["scores"], tables["pset_mask"]
        metrics[torch.from_numpy(idx).to(dev)] = tables["metrics"]
    return dict(partner=partner, scores=scores, pset_mask=masks, metrics=metrics, row_off=torch.from_numpy(row_off).to(dev),
                cell_off=torch.from_numpy(cell_off).to(dev)), nstruct, out_len


def Fold(inputfile=None, fileformat="unknown", inputseq=None, configfile=None, inputformat="qtrf", maxstemnum=None,
         algorithms='', rankby="r", hardrest=False, interchainonly=False, toplim=5, outplim=None, conslim=1, poollim=1000,
         levellimit=None, ignorewarn=False, HOME_DIR=None, priority=None, M=1.8, B=-0.6, records=None,
         alignment=False, evalonly=False, entropy=False, rfam=False, g4=False, rbp=False,
         i=None, ff=None, c=None, config=None, s=None, seq=None, algo=None, algorithm=None, rb=None, ll=None, levlim=None,
         tl=None, ol=None, cl=None, pl=None, pr=None, msn=None, hr=None, ico=None, iw=None, ignore=None, a=None, ali=None,
         eo=None, inputrestr=None, bpp=None):
    """Predict the structures of every input record and return them as a :class:`FoldResult`.

    The inputs (``inputfile`` / ``inputseq``), the prediction keywords, their defaults, synonyms, validation messages and the
    choice of configuration by length when no ``configfile`` is given are ``Predict``'s.  ``records`` gives the input directly
    instead: sequences, or (name, sequence, reactivities, restraints, reference) tuples with None for what a record lacks.
    ``outplim`` (default: ``toplim``) bounds the structures kept per record.  Alignment mode has a function of its own:
    use ``FoldAlignment``.  ``evalonly``, ``entropy`` and the ``rfam`` / ``g4`` / ``rbp`` restraint searches belong to
    ``Predict``.  All of these raise ValueError here.

    ``bpp`` gives the base-pair probabilities of the records for the ``bpp != 0`` paramsets (7 of the default
    configuration's 12) instead of the host provider (ViennaRNA): a list with one square matrix or None per record, or one
    ``[R, Lmax, Lmax]`` tensor whose leading N x N corner is record r's matrix -- N is the record's gap-free length with
    separators counted, what the reference hands to ViennaRNA.  CUDA float64 tensors are used where they are (a corner of
    the 3-D form is passed as a strided view, not copied) and the terms are formed on the GPU; float32 tensors are widened on
    their device; CPU tensors and arrays are uploaded once per record, not once per paramset.  The tensors are not modified.
    With an engine without ``fold_tensors`` the matrices go through the provider hook (``set_bpp_provider``) instead; records
    with the same sequence must then carry the same matrix."""
    inputfile = pick(inputfile, i); fileformat = pick(fileformat, ff)
    configfile = pick(configfile, config, c); inputseq = pick(inputseq, seq, s)
    algorithms = pick(algorithms, algorithm, algo); rankby = pick(rankby, rb)
    levellimit = pick(levellimit, levlim, ll); toplim = pick(toplim, tl); outplim = pick(outplim, ol)
    conslim = pick(conslim, cl); poollim = pick(poollim, pl); priority = pick(priority, pr)
    maxstemnum = pick(maxstemnum, msn); hardrest = pick(hardrest, hr); interchainonly = pick(interchainonly, ico)
    ignorewarn = pick(ignorewarn, ignore, iw)
    for flag, what in ((pick(alignment, ali, a), "alignment mode"), (pick(evalonly, eo), "evalonly"), (entropy, "entropy"),
                       (rfam, "rfam"), (g4, "g4"), (rbp, "rbp")):
        if flag:
            raise ValueError("Fold does not cover {}: use Predict".format(what))

    # ---- validation: Predict's checks of the keywords both take, same messages (SQUARNA.py:677-820): options.py
    inputfile, configfile, configfileset, priority, HOME_DIR = check_sources(records, inputfile, inputseq, fileformat, configfile,
                                                                             inputformat, HOME_DIR, priority)
    opt = prediction_options(maxstemnum=maxstemnum, M=M, B=B, algorithms=algorithms, rankby=rankby, outplim=outplim,
                             toplim=toplim, conslim=conslim, poollim=poollim, levellimit=levellimit)
    M, B = opt["M"], opt["B"]
    config_for = configs_by_length(configfile, configfileset, HOME_DIR, opt["maxstemnum"])
    inputs = input_records(records, inputseq, inputfile, inputformat, fileformat, ignorewarn, inputrestr, M, B)

    eng = _engine.get_engine()
    keep = max(int(opt["outplim"]), 1)
    common = dict(hardrest=hardrest, interchainonly=interchainonly, M=M, B=B, keep=keep,
                  **{k: opt[k] for k in ("conslim", "toplim", "rankbydiff", "rankby", "poollim", "algos", "levellimit")})
    seqs = [rec[1] for rec in inputs]
    psnames = [config_for(sq)[0] for sq in seqs]
    parts = []
    mats = _bpp_matrices(bpp, seqs, hasattr(eng, "fold_tensors")) if bpp is not None else None

    def flush(batch):
        # records with different priority index sets cannot share one fold call (as in Predict)
        groups = {}
        for k in batch:
            groups.setdefault(tuple(sorted(resolve_priority(priority, psnames[k]))), []).append(k)
        for prio, idx in groups.items():
            recs = [(inputs[k][1], inputs[k][2], inputs[k][3], inputs[k][4], config_for(seqs[k])[1], None) for k in idx]
            if hasattr(eng, "fold_tensors"):
                given = dict(bpp=[mats[k] for k in idx]) if mats is not None else {}
                t = eng.fold_tensors(recs, priority=set(prio), **given, **common)
                parts.append((t, t["nstruct"], t["lengths"], idx, True, t["source"]))
            else:
                with _given_to_provider(mats, seqs, idx):
                    res = eng.fold_records(recs, priority=set(prio), **common)
                refsc = getattr(eng, "last_ref_scores", None) or [None] * len(idx)
                full = [(r, seqs[k], (rs if rs is not None else _ref_scores(inputs[k])) if inputs[k][4] else None)
                        for r, k, rs in zip(res, idx, refsc)]
                parts.append(_oracle_tables(full, [seqs[k] for k in idx], keep) + (idx, False, "host"))

    for batch in batches(range(len(seqs)), lambda k: len(seqs[k]) * len(seqs[k]) * len(config_for(seqs[k])[1]),
                         _api.BATCH_RECORDS, _api.BATCH_CELLS):      # Predict's batches (api._predict_records)
        flush(batch)
    sources = {p[5] for p in parts}
    tables, nstruct, lengths = _join([p[:5] for p in parts], seqs)
    return FoldResult([rec[0] for rec in inputs], seqs, psnames, tables, nstruct, lengths,
                      sources.pop() if len(sources) == 1 else "mixed")


def _bpp_matrices(bpp, seqs, on_device):
    """Fold's bpp argument as one matrix or None per record: float64 N x N, N the record's gap-free length (separators
    counted).  on_device: CUDA torch tensors for HipEngine.fold_tensors (tensors already there are views, not copies; fp32
    is widened on its device; host data is uploaded once per record).  Else numpy arrays for the provider hook."""
    import torch
    R = len(seqs)
    lens = [int(np.count_nonzero(~gap_mask(sq))) for sq in seqs]
    if hasattr(bpp, "dim") and bpp.dim() == 3 or isinstance(bpp, np.ndarray) and bpp.ndim == 3:
        if bpp.shape[0] != R or bpp.shape[1] != bpp.shape[2] or bpp.shape[1] < max(lens):
            raise ValueError("bpp: shape %s; [%d, Lmax, Lmax] with Lmax >= %d is needed" % (tuple(bpp.shape), R, max(lens)))
        bpp = [bpp[k, :n, :n] for k, n in enumerate(lens)]
    elif len(bpp) != R:
        raise ValueError("bpp: %d matrices for %d records" % (len(bpp), R))
    out = []
    for k, (m, n) in enumerate(zip(bpp, lens)):
        if m is None:
            out.append(None)
            continue
        if not hasattr(m, "is_cuda"):
            m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64))
        if m.dim() != 2 or tuple(m.shape) != (n, n):
            raise ValueError("bpp[%d]: shape %s, the record needs %d x %d (its gap-free length, separators counted)" % (k, tuple(m.shape), n, n))
        if m.dtype not in (torch.float64, torch.float32):
            raise ValueError("bpp[%d]: dtype %s; float64 or float32 is needed" % (k, m.dtype))
        if not on_device:
            out.append(m.detach().double().cpu().numpy())
            continue
        if m.dtype != torch.float64:
            m = m.double()
        if not m.is_cuda:
            m = m.to(torch.device("cuda", torch.cuda.current_device()))
        if n > 1 and m.stride(1) != 1:
            m = m.contiguous()
        out.append(m)
    return out


@contextlib.contextmanager
def _given_to_provider(mats, seqs, idx):
    """For an engine without fold_tensors: the given matrices of records idx answer the provider hook, by gap-free
    sequence; every other sequence falls through to the provider installed before."""
    if mats is None or all(mats[k] is None for k in idx):
        yield
        return
    from .records import Prepared
    table = {}
    for k in idx:
        if mats[k] is None:
            continue
        key = Prepared(seqs[k]).shortseq
        if key in table and not np.array_equal(table[key], mats[k]):
            raise ValueError("bpp: two records with the sequence of record %d carry different matrices" % k)
        table[key] = mats[k]

    def provider(shortseq, reacts, M, B):
        m = table.get(shortseq)
        if m is None:
            return old(shortseq, reacts, M, B)
        return m if np.max(m, initial=0.0) > 0 else None                # (:350,360)
    old = _engine.set_bpp_provider(provider)
    try:
        yield
    finally:
        _engine.set_bpp_provider(old)


def _ref_scores(rec):
    """ScoreStruct of a record's known structure for an engine that does not report it (ReferenceScores, SQRNdbnseq.py:958-970)."""
    from .core import ReferenceScores
    return ReferenceScores(rec[1], rec[4], rec[2])
