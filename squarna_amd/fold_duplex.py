"""``FoldDuplex``: RNA-RNA interaction screens -- targets folded against queries as two-chain records, with what every duplex
does to its two partners formed where the folds are.

An interaction screen asks, for every pair of a set of targets and a set of queries (sRNA or miRNA against mRNA windows,
antisense oligos against a transcript), whether the two bind, where, and which part of each partner's own structure must open
for it.  ``FoldDuplex`` folds every target and query alone (one ``Fold(records=...)`` call), builds the ``A&B`` records of the
wanted pairs and folds them (a second call), and compares every duplex's consensus row with its two chains' rows: the pairs
between the chains (``inter``) and inside each (``intra_a``, ``intra_b``), the pairs of each chain alone that the duplex lacks
(``lost_a``, ``lost_b``), the stretch of each chain that pairs across, and per position of every solo record the number of
duplexes in which it pairs across.

With the GPU engine no row leaves the device: ``sq_duplex_summary`` forms the summary from the pair tables the two ``Fold``
calls left there, one wave per duplex.  An engine without the device method (the tests' CPU engine) gets the same object
built with numpy.  ``FoldDuplex`` prints nothing.
"""
import numpy as np

from . import engine as _engine
from . import fold as _fold
from .dbn import GAPS, SEPS
from .options import derived_inputs, pick
from .results import TensorResult
from .rows import position_axis

_DEVICE_METHODS = ("fold_tensors", "duplex_summary")
#: the columns of ``DuplexResult.summary``
COLUMNS = ("inter", "intra_a", "intra_b", "lost_a", "lost_b", "a_first", "a_last", "b_first", "b_last")
#: Fold's input keywords: FoldDuplex builds the records of both Fold calls itself
_FOLD_INPUTS = ("records", "inputfile", "inputseq", "inputrestr", "i", "s", "seq")


def _side(what, filekey, records, inputfile, inputformat, fileformat, ignorewarn, M, B, kw):
    """One side's (name, sequence, reactivities, restraints, reference) tuples, checked: no chain boundary inside; and the
    keywords for Fold."""
    if records is not None and inputfile is not None:
        raise ValueError("FoldDuplex: {} and {} are both given; one of them is needed".format(what, filekey))
    recs, kw = derived_inputs("FoldDuplex", list(records) if records is not None else None, inputfile, None, inputformat,
                              fileformat, ignorewarn, M, B, kw)
    for name, seq, reacts, rests, _ in recs:
        if any(ch in GAPS or ch in SEPS for ch in seq):
            raise ValueError("FoldDuplex: the sequence of record {} of the {} holds a gap or separator character: a chain "
                             "boundary inside an input would make \"the other chain\" ambiguous".format(name, what))
        if isinstance(reacts, str):
            raise ValueError("FoldDuplex: the reactivities of record {} of the {} are a string; a list of numbers is needed".format(name, what))
    return recs, kw


def _pair_lists(pairs, T, Q, homodimers):
    """(a, b) int64 arrays of the pairs to fold: indices into the targets and into the queries (Q None: both into the targets)."""
    if pairs is None:
        if Q is None:
            a, b = np.triu_indices(T, 0 if homodimers else 1)        # every a < b (and a == b), row after row
            return a.astype(np.int64), b.astype(np.int64)
        return np.repeat(np.arange(T, dtype=np.int64), Q), np.tile(np.arange(Q, dtype=np.int64), T)
    nb = T if Q is None else Q
    a, b = [], []
    try:
        pairs = [tuple(p) for p in pairs]
    except TypeError:
        raise ValueError("FoldDuplex: pairs must be a list of (a, b) index pairs")
    for p in pairs:
        if len(p) != 2 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in p):
            raise ValueError("FoldDuplex: {!r} is not an (a, b) pair of 0-based integers".format(p))
        if not (0 <= p[0] < T and 0 <= p[1] < nb):
            raise ValueError("FoldDuplex: the pair {!r} lies outside the {} targets x {} {}".format(p, T, nb, "targets" if Q is None else "queries"))
        a.append(int(p[0])); b.append(int(p[1]))
    return np.array(a, np.int64), np.array(b, np.int64)


def _joined(x, y, nx, ny, fill, as_line):
    """Two per-position annotations of the chains as one of the duplex: `fill` for every position of a side that has none and
    for the separator column, None when neither side has any."""
    if x is None and y is None:
        return None
    return as_line(x if x is not None else fill * nx) + fill + as_line(y if y is not None else fill * ny)


def _duplex_record(ra, rb):
    """The two-chain record of the solo records ra and rb: the reactivities concatenated with 0.5 for the separator column and
    for a side without any, the restraints with '.', no reference."""
    na, nb = len(ra[1]), len(rb[1])
    return (ra[0] + "&" + rb[0], ra[1] + "&" + rb[1], _joined(ra[2], rb[2], na, nb, [0.5], list), _joined(ra[3], rb[3], na, nb, ".", str), None)


def _host_summary(solos, folds, a_rec, b_rec, pos_off):
    """(summary int32[P, 9], bound int32[Ltot]) with numpy from the consensus rows of two host FoldResults (folds None: no
    duplex)."""
    P = len(a_rec)
    summary = np.zeros((P, 9), np.int32)
    summary[:, 5:] = -1
    bound = np.zeros(int(pos_off[-1]), np.int32)
    if not P:
        return summary, bound
    ps, cs, ls = solos.partner.numpy(), solos._cell_off, solos._lengths
    pd, cd, ld = folds.partner.numpy(), folds._cell_off, folds._lengths
    for k, (a, b) in enumerate(zip(a_rec.tolist(), b_rec.tolist())):
        nA, nB = int(ls[a]), int(ls[b])
        assert int(ld[k]) == nA + 1 + nB, "a duplex's table does not have its two chains' lengths"
        A, B, D = ps[cs[a]:cs[a] + nA], ps[cs[b]:cs[b] + nB], pd[cd[k]:cd[k] + nA + 1 + nB]
        assert D[nA] == -1, "the separator column of a duplex is paired"
        Da, Db = D[:nA], D[nA + 1:]
        ta, tb, ub = np.arange(nA), np.arange(nA + 1, nA + 1 + nB), np.arange(nB)
        inter_a, inter_b = Da > nA, (Db >= 0) & (Db < nA)
        summary[k, :5] = (inter_a.sum(), ((Da > ta) & (Da < nA)).sum(), (Db > tb).sum(), ((A > ta) & (Da != A)).sum(),
                          ((B > ub) & (Db != B + nA + 1)).sum())
        for col, hit in ((5, inter_a), (7, inter_b)):
            at = np.flatnonzero(hit)
            if len(at):
                summary[k, col], summary[k, col + 1] = at[0], at[-1]
        bound[pos_off[a]:pos_off[a] + nA] += inter_a
        bound[pos_off[b]:pos_off[b] + nB] += inter_b
    return summary, bound


class DuplexResult(TensorResult):
    """What ``FoldDuplex`` computes for T targets, Q queries and P duplexes.

    Host attributes: ``target_names``, ``query_names``, ``target_sequences``, ``query_sequences`` (the queries' lists are
    empty when the targets were screened against themselves: ``self_screen``), ``solos``: the :class:`FoldResult` of the targets followed by
    the queries, each folded alone, ``folds``: the :class:`FoldResult` of the P duplex records ``nameA&nameB`` (None when
    there is no pair), and ``source`` ("device" or "host": where the summary was formed).  Torch tensors on ``device``:
    ``a_rec`` / ``b_rec`` int32[P] -- the records of ``solos`` that are the first and the second chain of duplex k --,
    ``pos_off`` int64[T + Q + 1] -- the solo records' offsets on the axis on which they follow one another --, ``summary``
    int32[P, 9] -- per duplex, pairs counted at their 5' ends, the columns ``COLUMNS``: the pairs between the chains, inside
    chain A, inside chain B, the pairs of A alone whose 5' end has another partner or none in the duplex, the same for B,
    the lowest and the highest position of A with a partner in B, the same for B in its own coordinates (-1 without one)
    --, ``bound`` int32[sum of the solo lengths] -- per solo position the duplexes in which it pairs across the separator,
    in either role; record r starts at pos_off[r]."""

    _TENSORS = ("a_rec", "b_rec", "pos_off", "summary", "bound")
    _NESTED = ("solos", "folds")

    def __init__(self, target_names, query_names, target_sequences, query_sequences, self_screen, source, solos, folds, a_rec, b_rec,
                 pos_off, summary, bound):
        self.target_names, self.query_names = target_names, query_names
        self.target_sequences, self.query_sequences = target_sequences, query_sequences
        self.self_screen, self.source, self.solos, self.folds = self_screen, source, solos, folds
        self.a_rec, self.b_rec, self.pos_off, self.summary, self.bound = a_rec, b_rec, pos_off, summary, bound
        # the host's copy of the pairs and offsets: the helpers below index with it
        self._a, self._b, self._pos_off = a_rec.cpu().numpy().astype(np.int64), b_rec.cpu().numpy().astype(np.int64), pos_off.cpu().numpy()
        self._b0 = 0 if self_screen else len(target_names)            # (the solo record of query 0)

    def __len__(self):
        return len(self._a)

    def _duplex(self, k):
        if not 0 <= k < len(self._a):
            raise IndexError("there are %d duplexes" % len(self._a))
        return int(k)

    def _partners(self):
        """(targets, second partners): T and the number of queries, or of targets in a screen of the targets against themselves."""
        T = len(self.target_names)
        return T, T if self.self_screen else len(self.query_names)

    def index(self, a, b):
        """The first duplex k of target a and query b (of targets a and b in a screen of the targets against themselves)."""
        at = np.flatnonzero((self._a == a) & (self._b == b + self._b0))
        if not len(at):
            raise KeyError((a, b))
        return int(at[0])

    def dbn(self, k):
        """Dot-bracket line of duplex k's consensus, the separator in its column."""
        return self.folds.consensus(self._duplex(k))

    def solo_dbn(self, r):
        """Dot-bracket line of the consensus of solo record r (the targets, then the queries) folded alone."""
        if not 0 <= r < len(self.solos):
            raise IndexError("there are %d solo records" % len(self.solos))
        return self.solos.consensus(r)

    def site(self, k):
        """((a_first, a_last), (b_first, b_last)) of duplex k as host ints: the stretch of each chain that pairs across."""
        a0, a1, b0, b1 = self.summary[self._duplex(k), 5:].tolist()
        return (a0, a1), (b0, b1)

    def disruption(self, k=None):
        """lost_a + lost_b of duplex k (a 0-dim tensor), or int32[P] of all duplexes: the pairs of the two partners' own
        structures that the duplex opens."""
        d = self.summary[:, 3] + self.summary[:, 4]
        return d if k is None else d[self._duplex(k)]

    def to_matrix(self, col=0):
        """int32[T, Q] on the tensors' device: column `col` of the summary (its place in ``COLUMNS``) by target x query (target
        x target in a screen of the targets against themselves), -1 where a pair was not folded."""
        import torch
        if not 0 <= col < 9:
            raise IndexError("the summary has 9 columns")
        T, Q = self._partners()
        flat = self._a * Q + (self._b - self._b0)
        if len(np.unique(flat)) != len(flat):
            raise ValueError("DuplexResult.to_matrix: a pair was folded more than once")
        out = torch.full((T * Q,), -1, dtype=torch.int32, device=self.device)
        out[torch.from_numpy(flat).to(self.device)] = self.summary[:, col]
        return out.view(T, Q)

    def contacts(self, k):
        """bool[nA, nB] on the tensors' device: True where position i of chain A pairs with position j of chain B in duplex k."""
        import torch
        k = self._duplex(k)
        nA, nB = (int(self.solos._lengths[r]) for r in (self._a[k], self._b[k]))
        o = int(self.folds._cell_off[k])
        row = self.folds.partner[o:o + nA].long()
        return row[:, None] == torch.arange(nA + 1, nA + 1 + nB, device=row.device)[None, :]

    def bound_of(self, r):
        """int32[N_r]: per position of solo record r the duplexes in which it pairs across the separator."""
        if not 0 <= r < len(self.solos):
            raise IndexError("there are %d solo records" % len(self.solos))
        return self.bound[int(self._pos_off[r]):int(self._pos_off[r + 1])]

    def best_partners(self, a, n=10):
        """int64[min(n, partners)]: the queries (the other targets in a screen of the targets against themselves) with the
        largest `inter` with target a, ties to the lower index."""
        import torch
        if not 0 <= a < len(self.target_names):
            raise IndexError("there are %d targets" % len(self.target_names))
        first = self._a == a
        other = np.where(first, self._b - self._b0, self._a)
        mine = np.flatnonzero(first | ((self._b == a) & ~first) if self.self_screen else first)
        mine = mine[np.argsort(other[mine], kind="stable")]                      # (by partner, then a stable sort by inter)
        at = torch.from_numpy(mine).to(self.device)
        order = torch.sort(self.summary[at, 0], descending=True, stable=True)[1][:max(int(n), 0)]
        return torch.from_numpy(other[mine]).to(self.device)[order]

    def score_gain(self):
        """float64[P] on the tensors' device: the total score of every duplex's first structure minus those of its two chains'
        first structures folded alone; NaN where one of the three has no structure."""
        import torch
        if not len(self._a):
            return torch.empty(0, dtype=torch.float64, device=self.device)

        def first_total(f, recs):
            have = f.nstruct[recs] > 0
            rows = f.row_off[:-1][recs].clamp(max=max(int(f.scores.shape[0]) - 1, 0))
            total = f.scores[rows, 0] if f.scores.shape[0] else torch.zeros(len(recs), dtype=torch.float64, device=self.device)
            return torch.where(have, total, torch.full_like(total, float("nan")))
        every = torch.arange(len(self._a), device=self.device)
        return first_total(self.folds, every) - first_total(self.solos, self.a_rec.long()) - first_total(self.solos, self.b_rec.long())


def FoldDuplex(targets=None, queries=None, pairs=None, homodimers=False, targetfile=None, queryfile=None, inputformat="qtrf",
               fileformat="unknown", ignorewarn=False, M=1.8, B=-0.6, **fold_keywords):
    """Fold targets against queries as two-chain records and return a :class:`DuplexResult`.

    ``targets`` / ``queries`` take what ``Fold(records=...)`` takes (sequences, or (name, sequence, reactivities, restraints,
    reference) tuples), ``targetfile`` / ``queryfile`` what ``Fold(inputfile=...)`` takes, parsed as there; the list and the
    file of one side together raise ValueError.  Which pairs are folded: with queries and ``pairs`` None all T x Q pairs,
    duplex ``k = a * Q + b``; without queries the targets against themselves, every ``a < b`` and with ``homodimers`` also
    ``(a, a)``; ``pairs`` = [(a, b), ...] names exactly those, 0-based indices into the targets and the queries (both into the
    targets without queries), repeats allowed.  A sequence with a gap or separator character raises ValueError: a chain
    boundary inside an input would make "the other chain" ambiguous.

    Duplex (a, b) is the record ``(nameA&nameB, seqA&seqB, reactivities, restraints, None)``: numeric reactivity lists
    concatenated with 0.5 for the separator column and for a side that has none, restraint strings with ``.``, each None
    when neither side has any.  The solo records go through one ``Fold`` call with ``interchainonly=False`` and the duplexes
    through a second one with the caller's ``interchainonly``; every other keyword is forwarded unchanged to both
    (validation and messages are ``Fold``'s).  A record's structure is its consensus row.  ``bpp`` raises ValueError: a
    chain's matrix is not its duplexes'."""
    import torch
    kw = dict(fold_keywords)
    interchainonly = pick(kw.pop("interchainonly", False), kw.pop("ico", None))
    for key in _FOLD_INPUTS:
        if kw.get(key) is not None:
            raise ValueError("FoldDuplex takes its input as targets / queries (targetfile / queryfile), not as {}".format(key))
        kw.pop(key, None)
    trecs, common = _side("targets", "targetfile", targets, targetfile, inputformat, fileformat, ignorewarn, M, B, kw)
    self_screen = queries is None and queryfile is None
    qrecs = [] if self_screen else _side("queries", "queryfile", queries, queryfile, inputformat, fileformat, ignorewarn, M, B, kw)[0]
    T, Q = len(trecs), len(qrecs)
    a, b = _pair_lists(pairs, T, None if self_screen else Q, bool(homodimers))

    # ---- the solo records on one axis, the duplex records
    srecs = [tuple(rec) for rec in trecs + qrecs]
    a_rec, b_rec = a, b + (0 if self_screen else T)
    pos_off, Ltot = position_axis([rec[1] for rec in srecs])
    drecs = [_duplex_record(srecs[p], srecs[q]) for p, q in zip(a_rec.tolist(), b_rec.tolist())]

    solos = _fold.Fold(records=srecs, interchainonly=False, **common)
    folds = _fold.Fold(records=drecs, interchainonly=interchainonly, **common) if drecs else None

    eng = _engine.get_engine()
    on_device = all(hasattr(eng, m) for m in _DEVICE_METHODS) and solos.partner.is_cuda and (folds is None or folds.partner.is_cuda)
    dev = solos.device
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    d_a, d_b, d_pos_off = up(a_rec.astype(np.int32)), up(b_rec.astype(np.int32)), up(pos_off)
    if on_device:
        tables = (folds.partner, folds.cell_off, folds.lengths) if folds is not None else (None, None, None)
        summary, bound = eng.duplex_summary(solos.partner, solos.cell_off, solos.lengths, *tables, d_a, d_b, d_pos_off, Ltot)
    else:
        summary, bound = (torch.from_numpy(x) for x in _host_summary(solos, folds, a_rec, b_rec, pos_off))
    return DuplexResult([rec[0] for rec in trecs], [rec[0] for rec in qrecs], [rec[1] for rec in trecs], [rec[1] for rec in qrecs],
                        self_screen, "device" if on_device else "host", solos, folds, d_a, d_b, d_pos_off, summary, bound)
