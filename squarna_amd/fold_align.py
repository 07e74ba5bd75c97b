"""``FoldAlignment``: alignment mode that returns data instead of text.

``Predict(alignment=True)`` prints three dot-bracket lines; ``FoldAlignment`` takes the same input and keywords and returns an
:class:`AlignmentResult`: the three consensus structures, the normalised column stem matrix step 2 read, how often every
column pair was predicted across the rows, and the rows' own predictions in alignment coordinates, as torch tensors.

With the GPU engine nothing of size rows x L or L^2 crosses PCIe: the stem matrix is accumulated, thresholded and its cells
ranked on the device, the greedy assembly is a kernel (``sq_first_fit_dev``), step 2's pair tables stay where
``fold_tensors`` left them, and a kernel lifts them through the gap maps and counts them (``sq_align_pair_count``).  What
is O(L) -- the chosen pairs as a restraint line, bracket levels, the step-3 combination, metrics -- runs on the host through
``dbn.py``.  An engine without these device methods (the tests' CPU engine, the sharded one) gets the same object built on
the CPU through ``align.SQRNdbnali`` and ``Fold``'s host path.  ``FoldAlignment`` prints nothing.
"""
import contextlib
import io
import os

import numpy as np

from . import engine as _engine
from . import align as _align
from . import fold as _fold
from .dbn import DBNToPairs, PairsToDBN, gap_mask
from .inputs import ParseInput
from .options import alignment_defaults, check_sources, configs_by_length, pick, prediction_options
from .results import TensorResult
from .rows import checked_fit, first_fit, pair_table, partner_row, row_pairs

_DEVICE_METHODS = ("stem_matrix", "matrix_select", "first_fit", "fold_tensors", "align_pair_count")


def _consensus_order(torch, flat, count, first, nrows):
    """The permutation that puts the table in Consensus' order (SQRNdbnali.py:285 -- a stable sort by descending count over
    the dict's insertion order: rows in order, a row's pairs sorted): count descending, first row ascending, then v, w."""
    by_cell = torch.argsort(flat)
    key = (nrows - count.long()) * nrows + first.long()
    return by_cell[torch.sort(key[by_cell], stable=True)[1]]


def _rank_cells(torch, idx, val):
    """Matrix cells in MatrixToDBNs' order (SQRNdbnali.py:127-148 -- a stable sort by descending value over the index-ordered
    cells): value descending, flat index ascending."""
    idx, order = torch.sort(idx)
    return idx[torch.sort(val[order], descending=True, stable=True)[1]]


class AlignmentResult(TensorResult):
    """What alignment mode computes for an alignment of R rows and L columns.

    Host attributes: ``names``, ``sequences`` (as given), ``L``, the ``step3`` / ``freqlimit`` / ``levellimit`` the call
    used, ``source`` ("device" or "host": where the tables were formed) and ``first_fit_rounds`` (device path: the rounds
    of every greedy pass, in call order).  Torch tensors on ``device``:

    ``steps`` int32[3, L]: the partner rows of the Step-1, Step-2 and Step-3 lines over the alignment's columns, -1 where
    unpaired (Step-2 all -1 with step3 '1').  ``stem_matrix`` float64[L, L]: the normalised matrix step 2 read (smat / max * 5).
    ``pair_cols`` int32[P, 2], ``pair_count`` int32[P], ``pair_first`` int32[P]: every distinct column pair (v < w) that the
    consensus of any row holds, the number of rows that hold it and the first such row, in Consensus' order (count
    descending, first row, v, w ascending); empty when step 2 is skipped.  ``rows``: the :class:`FoldResult` of the
    step-2 predictions in alignment coordinates (gap columns -1), None when step 2 is skipped.  ``metrics`` float64[3, 6]:
    TP FP FN FS PR RC of the three lines (NaN without a reference line).  ``react_scores`` float64[3] (0.5 without
    reactivities, as in the reference)."""

    _TENSORS = ("steps", "stem_matrix", "pair_cols", "pair_count", "pair_first", "metrics", "react_scores")
    _NESTED = ("rows",)

    def __init__(self, names, sequences, steps, stem_matrix, pair_cols, pair_count, pair_first, rows, metrics, react_scores, source,
                 step3, freqlimit, levellimit, lines, first_fit_rounds=()):
        self.names, self.sequences, self.L = names, sequences, len(sequences[0])
        self._lines = tuple(lines)                                       # (the printed lines: their bracket levels were given BEFORE levellimit cut them)
        self.steps, self.stem_matrix, self.pair_cols, self.pair_count, self.pair_first = steps, stem_matrix, pair_cols, pair_count, pair_first
        self.rows, self.metrics, self.react_scores, self.source = rows, metrics, react_scores, source
        self.step3, self.freqlimit, self.levellimit, self.first_fit_rounds = step3, freqlimit, levellimit, tuple(first_fit_rounds)

    def __len__(self):
        return len(self.names)

    def _step(self, step):
        if step not in (1, 2, 3):
            raise IndexError("steps are 1, 2 and 3")
        return self.steps[step - 1].cpu().numpy()

    def pairs(self, step):
        """Sorted (v, w) column pairs, v < w, of the Step-`step` line."""
        return row_pairs(self._step(step))

    def dbn(self, step):
        """The dot-bracket line Predict prints for Step-`step` (as there, separator columns show '.')."""
        if step not in (1, 2, 3):
            raise IndexError("steps are 1, 2 and 3")
        return self._lines[step - 1]

    def pair_frequency(self):
        """float64[L, L] on the tensors' device: the share of rows whose consensus pairs columns v and w (symmetric)."""
        import torch
        out = torch.zeros((self.L, self.L), dtype=torch.float64, device=self.device)
        if self.pair_cols.numel():
            v, w = self.pair_cols[:, 0].long(), self.pair_cols[:, 1].long()
            # (divided by a tensor: by a Python number the device form multiplies with the reciprocal, which is not count / rows
            # in the last bit)
            c = self.pair_count.double()
            f = c / torch.full_like(c, len(self.names))
            out[v, w] = f
            out[w, v] = f
        return out

    def consensus_at(self, freqlimit, levellimit=None):
        """Consensus of the rows' predictions for another frequency limit, from the stored table (no fold): the line
        align.Consensus returns; with levellimit (e.g. the result's own), cut to that many bracket levels as the Step-2
        line is."""
        if self.rows is None:
            raise ValueError("step 2 was skipped (step3='1'): there is no table")
        eng = _engine.get_engine()
        n = int((self.pair_count.double() >= float(freqlimit) * len(self.names)).sum())   # (a prefix: the counts only fall)
        if self.pair_cols.is_cuda and hasattr(eng, "first_fit"):
            flat = self.pair_cols[:n, 0].long() * self.L + self.pair_cols[:n, 1].long()
            pairs = row_pairs(_fitted_row(eng.first_fit(flat, self.L, 0), None))
        else:
            pairs = first_fit(self.pair_cols[:n].tolist())
        dbn = PairsToDBN(list(set(pairs)), self.L)
        return dbn if levellimit is None else PairsToDBN(DBNToPairs(dbn), self.L, levellimit=levellimit)


def _fitted_row(fit, rounds):
    """The host's copy of a first fit's partner row (L int32: the only part of it that leaves the device)."""
    partner, info = fit
    checked_fit(info, rounds)
    return partner.cpu().numpy()


def _device_steps(eng, objs, defS, ps0, interchainonly, step3, freqlimit, fold_opts, paramsets, keep):
    """Steps 1 and 2 with the GPU engine: (pairs of step 1's second iteration, pairs of the consensus or None, normalised
    matrix, table tensors, rows' tables, rounds)."""
    import torch
    N, R = len(objs[0][1]), len(objs)
    rounds = []

    def iteration(rests):
        recs = [(obj[1].upper().replace("T", "U"), obj[2], rests if rests else obj[3]) for obj in objs]
        smat = eng.stem_matrix(recs, ps0['bpweights'], ps0['minlen'], ps0['minbpscore'], interchainonly)
        idx, val = eng.matrix_select(smat, ps0['minbpscore'] * R, 4)
        return row_pairs(_fitted_row(eng.first_fit(_rank_cells(torch, idx, val), N, 4), rounds)), smat

    pairs, smat = iteration(defS)
    pairs1 = DBNToPairs(PairsToDBN(iteration(PairsToDBN(pairs, N))[0], N))   # iteration 2: the found line as restraints (:359-364)
    smat = (smat / smat.max() * 5).contiguous()                      # :371 (the same two IEEE operations per cell as numpy's)
    if step3 == '1':
        return pairs1, None, smat, None, None, rounds
    recs = [(obj[1], obj[2], obj[3], obj[4], paramsets, smat) for obj in objs]
    t = eng.fold_tensors(recs, levellimit=None, priority=set(), keep=keep, **fold_opts)
    gap_maps = [np.flatnonzero(~gap_mask(obj[1])).astype(np.int32) for obj in objs]
    assert [len(g) for g in gap_maps] == t["lengths"].tolist(), "a row's table does not have its gap-free length"
    flat, count, first = eng.align_pair_count(t["partner"], t["cell_off"], gap_maps, N)
    order = _consensus_order(torch, flat, count, first, R)
    flat, count, first = flat[order], count[order], first[order]
    n = int((count.double() >= freqlimit * R).sum())                 # :286 (a prefix: the counts only fall)
    pairs2 = row_pairs(_fitted_row(eng.first_fit(flat[:n], N, 0), rounds))
    cols = torch.stack((flat // N, flat % N), 1).to(torch.int32)
    return pairs1, pairs2, smat, (cols, count, first), t, rounds


def _host_table(rows, N):
    """(pair_cols, pair_count, pair_first) as numpy arrays from the consensus rows of a host FoldResult, in Consensus' order."""
    uniq, counts, first = pair_table(rows.partner.numpy(), rows._cell_off, rows._lengths, N)
    order = np.lexsort((uniq, first, -counts))
    uniq, first, counts = uniq[order], first[order], counts[order]
    return np.stack((uniq // N, uniq % N), 1).astype(np.int32), counts.astype(np.int32), first.astype(np.int32)


def _host_steps(eng, objs, defR, defS, defF, ps0, interchainonly, step3, freqlimit, fold_opts, paramsetnames, paramsets, keep, M, B):
    """Steps 1 and 2 through the engine's host interface (align.SQRNdbnali, Fold's host path)."""
    import torch
    N = len(objs[0][1])
    sink = io.StringIO()
    args = (ps0['bpweights'], interchainonly, ps0['minlen'], ps0['minbpscore'], 1, False)
    pred, smat = _align.SQRNdbnali(objs, defS, defR, defF, *args, sink=sink, M=M, B=B)
    pairs1 = DBNToPairs(_align.SQRNdbnali(objs, pred, defR, defF, *args, sink=sink, M=M, B=B)[0])
    if not isinstance(smat, np.ndarray):
        smat = smat.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        smat = smat / np.max(smat) * 5                                # :371
    if step3 == '1':
        return pairs1, None, torch.from_numpy(smat), None, None
    seqs = [obj[1] for obj in objs]
    recs = [(obj[1], obj[2], obj[3], obj[4], paramsets, smat) for obj in objs]
    res = eng.fold_records(recs, levellimit=None, priority=set(), keep=keep, **fold_opts)
    refsc = getattr(eng, "last_ref_scores", None) or [None] * len(objs)
    full = [(r, obj[1], (rs if rs is not None else _fold._ref_scores(obj)) if obj[4] else None) for r, obj, rs in zip(res, objs, refsc)]
    tables, nstruct, lengths = _fold._oracle_tables(full, seqs, keep)
    rows = _fold.FoldResult([obj[0] for obj in objs], seqs, [paramsetnames] * len(objs), tables, nstruct, lengths, "host")
    cols, count, first = _host_table(rows, N)
    n = int((count.astype(np.float64) >= freqlimit * len(objs)).sum())
    pairs2 = first_fit(cols[:n].tolist())
    return pairs1, pairs2, torch.from_numpy(smat), tuple(torch.from_numpy(a) for a in (cols, count, first)), rows


def FoldAlignment(inputfile=None, fileformat="unknown", configfile=None, inputformat="qtrf", maxstemnum=None, algorithms='',
                  rankby="r", hardrest=False, interchainonly=False, toplim=5, outplim=None, conslim=1, poollim=1000,
                  levellimit=None, freqlimit=0.35, step3="u", ignorewarn=False, HOME_DIR=None, priority=None, M=1.8, B=-0.6,
                  verbose=False, entropy=False, rfam=False, g4=False, rbp=False,
                  i=None, ff=None, c=None, config=None, algo=None, algorithm=None, rb=None, fl=None, freqlim=None, ll=None,
                  levlim=None, tl=None, ol=None, cl=None, pl=None, pr=None, s3=None, msn=None, hr=None, ico=None, iw=None,
                  ignore=None, v=None):
    """Alignment-based prediction for the alignment in ``inputfile``, returned as an :class:`AlignmentResult`.

    The input, the prediction keywords, ``freqlimit``, ``step3`` and ``levellimit``, their defaults, synonyms, validation
    messages and the choice of ``ali.conf`` when no ``configfile`` is given are those of ``Predict(alignment=True)``;
    ``outplim`` (default: ``toplim``) bounds the structures kept per row in ``rows``.  ``verbose``, ``entropy`` and the
    ``rfam`` / ``g4`` / ``rbp`` restraint searches belong to ``Predict`` and raise ValueError here."""
    import torch
    inputfile = pick(inputfile, i); fileformat = pick(fileformat, ff)
    configfile = pick(configfile, config, c); algorithms = pick(algorithms, algorithm, algo)
    rankby = pick(rankby, rb); freqlimit = pick(freqlimit, freqlim, fl)
    levellimit = pick(levellimit, levlim, ll); toplim = pick(toplim, tl); outplim = pick(outplim, ol)
    conslim = pick(conslim, cl); poollim = pick(poollim, pl); priority = pick(priority, pr)
    step3 = pick(step3, s3); maxstemnum = pick(maxstemnum, msn); hardrest = pick(hardrest, hr)
    interchainonly = pick(interchainonly, ico); ignorewarn = pick(ignorewarn, ignore, iw)
    for flag, what in ((pick(verbose, v), "verbose"), (entropy, "entropy"), (rfam, "rfam"), (g4, "g4"), (rbp, "rbp")):
        if flag:
            raise ValueError("FoldAlignment does not cover {}: use Predict".format(what))

    # ---- validation: Predict's checks of the keywords both take, same messages (SQUARNA.py:677-820): options.py
    inputfile, configfile, configfileset, priority, HOME_DIR = check_sources(None, inputfile, None, fileformat, configfile,
                                                                             inputformat, HOME_DIR, priority)
    opt = prediction_options(maxstemnum=maxstemnum, M=M, B=B, algorithms=algorithms, rankby=rankby, outplim=outplim,
                             toplim=toplim, conslim=conslim, poollim=poollim, levellimit=levellimit, freqlimit=freqlimit,
                             step3=step3)
    M, B, levellimit, freqlimit, step3 = (opt[k] for k in ("M", "B", "levellimit", "freqlimit", "step3"))
    if not configfileset:                                            # SQUARNA.py:822-824
        configfile = os.path.join(HOME_DIR, "ali.conf")
    paramsetnames, paramsets = configs_by_length(configfile, True, HOME_DIR, opt["maxstemnum"])("")

    with contextlib.redirect_stdout(io.StringIO()):                  # (the parser announces a guessed file format)
        inputs, fmt, _ = ParseInput(None, inputfile, inputformat, fmt=fileformat, ignore=ignorewarn, M=M, B=B)
        objs = [obj for obj in inputs]
        defR, defS, defF = ParseInput(None, inputfile, inputformat, returndefaults=True, fmt=fmt, ignore=ignorewarn, M=M, B=B)[0]
    assert objs, "No input records."
    N = len(objs[0][1])                                              # SQUARNA.py:938-991
    assert all(len(obj[1]) == N for obj in objs), 'The sequences are not aligned'
    defR = alignment_defaults(defR, defS, defF, N, M, B)
    if levellimit is None:
        levellimit = 3 - int(N > 500)

    eng = _engine.get_engine()
    keep = max(int(opt["outplim"]), 1)
    fold_opts = dict(hardrest=hardrest, interchainonly=interchainonly, M=M, B=B,
                     **{k: opt[k] for k in ("conslim", "toplim", "rankbydiff", "rankby", "poollim", "algos")})
    names, seqs = [obj[0] for obj in objs], [obj[1] for obj in objs]
    rows, rounds = None, ()
    on_device = all(hasattr(eng, m) for m in _DEVICE_METHODS) and not hasattr(eng, "reduce_matrix")
    if on_device:
        pairs1, pairs2, smat, table, t, rounds = _device_steps(eng, objs, defS, paramsets[0], interchainonly, step3, freqlimit,
                                                               fold_opts, paramsets, keep)
        dev = smat.device
        if t is not None:
            tables, nstruct, lengths = _fold._join([(t, t["nstruct"], t["lengths"], list(range(len(objs))), True)], seqs)
            rows = _fold.FoldResult(names, seqs, [paramsetnames] * len(objs), tables, nstruct, lengths, t["source"])
    else:
        pairs1, pairs2, smat, table, rows = _host_steps(eng, objs, defR, defS, defF, paramsets[0], interchainonly, step3, freqlimit,
                                                        fold_opts, paramsetnames, paramsets, keep, M, B)
        dev = smat.device

    # ---- O(L) on the host: bracket levels, the step-3 combination, metrics (SQRNdbnali.py:366-368, 400-402, 428-458)
    step1dbn = PairsToDBN(pairs1, N, levellimit=levellimit)
    step2dbn = PairsToDBN(list(set(pairs2)), N) if pairs2 is not None else '.' * N
    step2dbn = PairsToDBN(DBNToPairs(step2dbn), N, levellimit=levellimit)
    if step3 == '1':
        step3dbn = step1dbn
    elif step3 == '2':
        step3dbn = step2dbn
    elif step3 == 'i':
        step3dbn = PairsToDBN(sorted(set(DBNToPairs(step1dbn)) & set(DBNToPairs(step2dbn))), N)
    else:
        step1pairs = DBNToPairs(step1dbn)
        seen_pos = set(pos for bp in step1pairs for pos in bp)
        for v, w in DBNToPairs(step2dbn):
            if v not in seen_pos and w not in seen_pos:
                step1pairs.append((v, w))
        step3dbn = PairsToDBN(sorted(step1pairs), N)
    lines = (step1dbn, step2dbn, step3dbn)
    steps = np.stack([partner_row(DBNToPairs(line), N) for line in lines])
    metrics = np.array([[float(x) for x in _align.Metrics(defF, line)] for line in lines], np.float64)
    reacts = np.array([float(_align.ReactScore(defR, seqs[0], line)) for line in lines], np.float64)
    if table is None:
        table = (torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                 torch.zeros(0, dtype=torch.int32, device=dev))
    up = lambda a: torch.from_numpy(a).to(dev)
    return AlignmentResult(names, seqs, up(steps), smat, table[0], table[1], table[2], rows, up(metrics), up(reacts),
                           "device" if on_device else "host", step3, freqlimit, levellimit, lines, rounds)
