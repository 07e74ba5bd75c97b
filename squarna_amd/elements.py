"""``Elements``: what every position of a GIVEN structure is.

``Score`` turns structures into numbers; ``Elements`` annotates them: the pseudoknot level of every pair (the rule of
``dbn.PairsToDBN``), the loop every column belongs to and that loop's type (the "structure array" of bpRNA), and the list of
the loops with their sizes.  It takes the structures in the three forms ``Score`` takes and returns an
:class:`ElementsResult`.  With the GPU engine the rows are annotated by two kernels (``sq_elements_rows``), one wave per row,
and a tensor of partners that is on the device already is read where it is; an engine without ``elements_tensors`` (the
tests' CPU engine, the sharded engine) gets the same object built on the CPU, by a stack walk -- not the kernels' form.
"""
import contextlib
import os

import numpy as np

from . import engine as _engine
from .config import DATA_DIR
from .dbn import PairsToDBN, levels_to_dbn
from .options import input_records
from .results import TensorResult
from .rows import offsets
from .score import ScoreRecord, _partner_rows

#: the codes of ``ElementsResult.element`` (SQ_ELEM_* of csrc/sq_elements.h); the first six are the loop types as well
EXTERIOR, STEM, HAIRPIN, BULGE, INTERNAL, MULTI, PK, BREAK, GAP = range(9)
CODES = 9
#: the letter of every code, for ``ElementsResult.text``
LETTERS = "ESHBIMK&-"


def loop_type(exterior, brk, branches, unpaired, side5):
    """The type of a loop, or None for a stack: the first rule that matches."""
    if exterior or brk:
        return EXTERIOR
    if branches == 0:
        return HAIRPIN
    if branches >= 2:
        return MULTI
    if unpaired == 0:
        return None
    return BULGE if side5 in (0, unpaired) else INTERNAL


def elements_row_host(rec, row):
    """One partner row (input columns of ``rec``; longer rows: their first columns) on the CPU: (status, element int8[width],
    level int16[width], loop_of int32[width], loops [(type, i, j, branches, unpaired, side5)], number of pairs, number of
    levels).  Status 1: a partner outside the record, p[p[i]] != i, p[i] == i or a pair on a separator; such a row holds -1,
    0, -1 and has no loop."""
    lin = len(rec.seq)
    row = np.asarray(row[:lin], np.int64)
    element, level, loop_of = np.full(lin, -1, np.int8), np.zeros(lin, np.int16), np.full(lin, -1, np.int32)
    idx = np.flatnonzero(row != -1)
    p = row[idx]
    if ((p < 0) | (p >= lin) | (p == idx)).any() or (row[p] != idx).any() or rec.sepcol[idx].any():
        return 1, element, level, loop_of, [], 0, 0
    up = idx[p > idx]
    v, w = rec.colmap[up], rec.colmap[row[up]]
    keep = (v >= 0) & (w >= 0)                                       # a pair that touches a gap column is dropped
    pairs = list(zip(v[keep].tolist(), w[keep].tolist()))
    levels = PairsToDBN(pairs, rec.n, returnlevels=True)
    lev = [0] * rec.n                                                # signed, by gap-free position
    for (a, b), l in levels.items():
        lev[a], lev[b] = l, -l
    sep = rec.sepcol[rec.gfcol]
    # one pass with a stack of the open loops: [closing pair's opener, branches, unpaired, side5, break, positions]
    ext = [-1, 0, 0, 0, False, []]
    stack, made = [ext], [ext]
    for g in range(rec.n):
        cur = stack[-1]
        if lev[g] == 1:
            cur[1] += 1
            stack.append([g, 0, 0, 0, False, []])
            made.append(stack[-1])
        elif lev[g] == -1:
            stack.pop()
        elif sep[g]:
            cur[4] = True
        else:
            cur[2] += 1
            cur[3] += cur[1] == 0
            cur[5].append(g)
    partner = dict(pairs)
    element[:] = np.where(rec.colmap < 0, GAP, EXTERIOR)
    element[rec.sepcol] = BREAK
    loops = []
    for g, branches, unpaired, side5, brk, members in made:          # (made in the order of the openers: by i ascending)
        kind = loop_type(g < 0, brk, branches, unpaired, side5)
        if kind is None:
            continue
        cols = rec.gfcol[members]
        loop_of[cols] = len(loops)
        element[cols] = kind
        loops.append((kind, -1, lin, branches, unpaired, side5) if g < 0 else
                     (kind, int(rec.gfcol[g]), int(rec.gfcol[partner[g]]), branches, unpaired, side5))
    for (a, b), l in levels.items():
        for g, s in ((a, l), (b, -l)):
            level[rec.gfcol[g]] = s
            element[rec.gfcol[g]] = STEM if l == 1 else PK
    return 0, element, level, loop_of, loops, len(pairs), max(levels.values(), default=0)


def _elements_host(recs, partner, row_start, row_rec):
    """The tables of ElementsResult on the CPU, as numpy arrays."""
    rows = len(row_rec)
    cell_off = offsets([len(recs[r].seq) for r in row_rec])
    out = dict(element=np.full(int(cell_off[-1]), -1, np.int8), level=np.zeros(int(cell_off[-1]), np.int16),
               loop_of=np.full(int(cell_off[-1]), -1, np.int32), cell_off=cell_off)
    for k in ("status", "npairs", "nlevels", "nloops"):
        out[k] = np.zeros(rows, np.int32)
    loops = []
    for q in range(rows):
        rec = recs[row_rec[q]]
        st, el, lv, lo, ll, npairs, nlevels = elements_row_host(rec, partner[row_start[q]:row_start[q] + len(rec.seq)])
        a, b = cell_off[q], cell_off[q + 1]
        out["element"][a:b], out["level"][a:b], out["loop_of"][a:b] = el, lv, lo
        out["status"][q], out["npairs"][q], out["nlevels"][q], out["nloops"][q] = st, npairs, nlevels, len(ll)
        loops.extend(ll)
    out["loops"] = np.array(loops, np.int32).reshape(-1, 6)
    out["loop_off"] = offsets(out["nloops"])
    return out


class ElementsResult(TensorResult):
    """The annotation of ``Elements`` for the structure rows of R records.

    Host attributes: ``names``, ``sequences`` (as given); ``source``: "device" or "host" -- where the rows were annotated;
    ``recomputed``: how many rows the device handed back to the host (more stems than its LDS holds, more than 64 levels).
    Torch tensors (``device``: where they live): ``row_off`` int64[R + 1] -- record r's rows are row_off[r] .. row_off[r + 1].
    Per column, the rows flat, row q's input columns at ``cell_off``[q] .. cell_off[q + 1] (int64[rows + 1]): ``element`` int8
    (0 E exterior, 1 S stem: in a pair of level 1, 2 H hairpin, 3 B bulge, 4 I internal, 5 M multiloop, 6 K in a pair of level
    >= 2, 7 & a separator, 8 - a gap column; an unpaired column carries its loop's type, and a column of a pair that touches
    a gap column counts as unpaired), ``level`` int16 (+L opens, -L closes a pair of level L, else 0), ``loop_of`` int32 (the
    column's loop in the row's list; -1 for S, & and - columns).  Per row: ``status`` int32 (0; 1: an invalid row, whose
    columns hold -1, 0, -1 and which has no loop), ``npairs``, ``nlevels``, ``nloops`` int32.  ``loops`` int32[S, 6] = (type, i,
    j, branches, unpaired, side5), row q's from ``loop_off``[q] on (int64[rows + 1]): the loops that the pairs (i, j) of level
    1 close, in columns of the sequence AS GIVEN; the exterior loop first, with i = -1 and j = the row's width, the others by
    i ascending; a loop that holds a separator is of type exterior; stacks are not listed.  ``unpaired`` counts the loop's
    columns that are neither gap nor separator (columns of pairs of level >= 2 among them), ``side5`` those of them before
    the first branch."""

    _TENSORS = ("element", "level", "loop_of", "cell_off", "status", "npairs", "nlevels", "nloops", "loops", "loop_off", "row_off")

    def __init__(self, names, sequences, tables, source, recomputed=0):
        self.names, self.sequences, self.source, self.recomputed = names, sequences, source, recomputed
        for k in self._TENSORS:
            setattr(self, k, tables[k])
        # the host's copy of the offsets: the helpers below index with it, no device round trip per call
        self._cell_off, self._loop_off = (tables[k].cpu().numpy() for k in ("cell_off", "loop_off"))

    def __len__(self):
        return len(self.names)

    def _cells(self, q):
        return slice(int(self._cell_off[q]), int(self._cell_off[q + 1]))

    def text(self, q):
        """The element string of row q, one letter of ``E S H B I M K & -`` per column ('?' throughout an invalid row)."""
        return ''.join(LETTERS[c] if c >= 0 else '?' for c in self.element[self._cells(q)].tolist())

    def dbn(self, q):
        """Dot-bracket string of row q from its levels (a dropped pair prints as dots)."""
        return levels_to_dbn(self.level[self._cells(q)].tolist())

    def loops_of(self, q):
        """[(type, i, j, branches, unpaired, side5)] of row q."""
        a, b = (int(x) for x in self._loop_off[q:q + 2])
        return [tuple(s) for s in self.loops[a:b].tolist()]

    def _row_of_cell(self):
        import torch
        rows, total = len(self._cell_off) - 1, int(self._cell_off[-1])
        return torch.repeat_interleave(torch.arange(rows, device=self.device), self.cell_off[1:] - self.cell_off[:-1], output_size=total)

    def to_padded(self, fill=-1):
        """int8[rows, Lmax]: every row's elements, `fill` where a row is shorter; formed on the tensors' device."""
        import torch
        rows, total = len(self._cell_off) - 1, int(self._cell_off[-1])
        Lmax = int(np.diff(self._cell_off).max(initial=0))
        out = torch.full((rows, Lmax), fill, dtype=torch.int8, device=self.device)
        if total:
            row = self._row_of_cell()
            out[row, torch.arange(total, device=self.device) - self.cell_off[row]] = self.element
        return out

    def one_hot(self):
        """int8[cells, 9]: 1 at every column's code (a column of an invalid row: zeros); formed on the tensors' device."""
        import torch
        return (self.element[:, None] == torch.arange(CODES, dtype=torch.int8, device=self.device)[None, :]).to(torch.int8)

    def composition(self):
        """float64[rows, 9]: every code's share of the row's columns that are no gap columns (the gap code's own: 0); NaN for
        a row without such a column and for an invalid row."""
        import torch
        rows = len(self._cell_off) - 1
        counts = torch.zeros(rows * CODES, dtype=torch.int64, device=self.device)
        ok = (self.element >= 0) & (self.element != GAP)
        counts.index_add_(0, (self._row_of_cell() * CODES + self.element.long())[ok], torch.ones_like(counts[:1]).expand(int(ok.sum())))
        counts = counts.view(rows, CODES).double()
        # (divided by tensors: by a Python number the device form multiplies with the reciprocal -- as CovariationResult.score)
        return counts / counts.sum(1, keepdim=True).expand_as(counts)


@contextlib.contextmanager
def _own_wording():
    """The helpers shared with Score name it in their errors: the same words with this entry's name in front."""
    try:
        yield
    except ValueError as e:
        msg = str(e)
        raise ValueError("Elements: " + msg[len("Score: "):] if msg.startswith("Score: ") else msg) from None


def Elements(records=None, structures=None, inputfile=None, inputseq=None, inputformat="qtrf", fileformat="unknown", ignorewarn=False,
             strict=True, nstruct=None):
    """Annotate the given structures of every record and return an :class:`ElementsResult`.

    The records and ``structures`` come as for ``Score``: lists of dot-bracket strings per record; one int tensor or array
    ``[R, K, Lmax]`` of partners with ``nstruct``, a CUDA tensor where it is; a ``FoldResult`` (without ``records``, its
    sequences are the records); or None: every record's known structure is its only row.  Reactivities and restraints play
    no part.

    Coordinates are columns of the sequence as given.  Gap columns are transparent: a pair that touches one is dropped, and
    stacking is decided on the gap-free sequence.  An invalid row -- a partner outside the record, p[p[i]] != i, p[i] == i, a
    pair on a separator -- raises ValueError under ``strict``; else its status is 1.  Records longer than 32,768 nt raise
    ValueError."""
    import torch
    from .fold import FoldResult
    if records is None and inputfile is None and not inputseq and isinstance(structures, FoldResult):
        records = [(name, seq, None, None, None) for name, seq in zip(structures.names, structures.sequences)]
    if records is None:
        if inputfile is not None and not os.path.exists(inputfile) and os.path.exists(os.path.join(DATA_DIR, inputfile)):
            inputfile = os.path.join(DATA_DIR, inputfile)            # (as Fold: a name inside the package's data directory)
        assert inputseq or os.path.exists(str(inputfile)), "Input file does not exist."
    inputs = input_records(records, inputseq, inputfile, inputformat, fileformat, ignorewarn, None, 1.8, -0.6)
    if structures is None:
        structures = [[rec[4]] if rec[4] else [] for rec in inputs]
    eng = _engine.get_engine()
    on_device = hasattr(eng, "elements_tensors")
    with _own_wording():
        recs = [ScoreRecord(rec[0], rec[1]) for rec in inputs]
        partner, row_start, row_rec, row_off = _partner_rows(structures, nstruct, recs, on_device)
    recomputed = 0
    if on_device:
        tables = eng.elements_tensors(recs, partner, row_start, row_rec)
        dev = tables["status"].device
        status = tables["status"].cpu().numpy()
        redo = np.flatnonzero(status == 2).tolist()
        recomputed = len(redo)
        if redo:                                                     # rows the kernels left to the host
            cell_off, old_off = tables["cell_off"].cpu().numpy(), tables["loop_off"].cpu().numpy()
            pieces, done = [], 0
            for q in redo:
                rec, a = recs[row_rec[q]], int(row_start[q])
                st, el, lv, lo, ll, npairs, nlevels = elements_row_host(rec, partner[a:a + len(rec.seq)].cpu().numpy())
                cells = slice(int(cell_off[q]), int(cell_off[q + 1]))
                for k, v in (("element", el), ("level", lv), ("loop_of", lo)):
                    tables[k][cells] = torch.from_numpy(v).to(dev)
                for k, v in (("status", st), ("npairs", npairs), ("nlevels", nlevels), ("nloops", len(ll))):
                    tables[k][q] = v
                status[q] = st
                # (such a row had no loop on the device: the loops of the rows before it, then its own)
                pieces += [tables["loops"][done:int(old_off[q])], torch.tensor(ll, dtype=torch.int32, device=dev).reshape(-1, 6)]
                done = int(old_off[q])
            tables["loops"] = torch.cat(pieces + [tables["loops"][done:]])
            tables["loop_off"] = torch.zeros_like(tables["loop_off"])
            tables["loop_off"][1:] = torch.cumsum(tables["nloops"], 0, dtype=torch.int64)
        tables["row_off"] = torch.from_numpy(row_off).to(dev)
    else:
        host = _elements_host(recs, partner.numpy(), row_start, row_rec)
        status = host["status"]
        tables = {k: torch.from_numpy(v) for k, v in host.items()}
        tables["row_off"] = torch.from_numpy(row_off)
    if strict and status.any():
        q = int(np.flatnonzero(status)[0])
        r = int(row_rec[q])
        raise ValueError("Elements: record %d (%s), row %d: not a valid structure of the record" % (r, recs[r].name, q - int(row_off[r])))
    return ElementsResult([rec[0] for rec in inputs], [rec[1] for rec in inputs], tables, "device" if on_device else "host", recomputed)
