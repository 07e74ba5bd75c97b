"""``FoldMutants``: the substitution variants of a sequence folded beside it, with the change of structure formed where the
folds are.

An in-silico mutational scan asks which substitutions change the structure of an RNA: every position of an N-nt record gets
its three other letters, 3 N variants as long as the wild type (or the caller names the variants, any number of sites each:
double and compensatory mutants).  ``FoldMutants`` builds the variant records, sends the wild types and ALL variants of ALL
input records through ONE ``Fold(records=...)`` call, and compares every variant's consensus row with its wild type's: the
pairs ``lost``, ``gained`` and ``kept``, the positions whose partner ``changed`` with the ``first`` and the ``last`` of them,
and per wild-type position how many variants changed its partner.

With the GPU engine no row leaves the device: ``sq_variant_diff`` forms the summary from the pair tables ``Fold`` left there,
one wave per variant.  An engine without the device method (the tests' CPU engine) gets the same object built with numpy.
``FoldMutants`` prints nothing.
"""
import numpy as np

from . import engine as _engine
from . import fold as _fold
from .dbn import GAPS, SEPS
from .options import derived_inputs
from .results import TensorResult
from .rows import position_axis

_DEVICE_METHODS = ("fold_tensors", "variant_diff")

LETTERS = "ACGU"
_CODES = np.frombuffer(LETTERS.encode(), np.uint8)
#: the RNA letter a character stands for (upper-cased, T -> U), 0 for any other character
_NORM = np.zeros(128, np.uint8)
for _given, _letter in zip("ACGUTacgut", "ACGUUACGUU"):
    _NORM[ord(_given)] = ord(_letter)
#: the column of an RNA letter in ``to_matrix``
_COLUMN = np.zeros(256, np.int64)
_COLUMN[_CODES] = np.arange(4)
_CHUNK = 1 << 22                                                     # characters of variant sequences formed at once


def _codes(seq):
    """One uint32 per character of a str."""
    return np.frombuffer(seq.encode("utf-32-le"), dtype="<u4")


def _normalised(codes):
    """The RNA letters (uint8 ASCII) of an array of characters, 0 where a character is none."""
    return np.where(codes < 128, _NORM[codes & 127], 0).astype(np.uint8)


def _scan_positions(positions, shortest):
    """`positions` as an ascending array without duplicates (None: None), checked against the shortest record."""
    if positions is None:
        return None
    pos = list(positions)
    for p in pos:
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= p < shortest:
            raise ValueError("Inappropriate positions entry (0-based integer below the shortest record's length, {}): {!r}".format(shortest, p))
    return np.unique(np.array(pos, np.int64))


def _explicit_sites(name, seq, entries):
    """(site_off, site_pos, site_letter) of one record's explicitly given variants, validated."""
    try:
        entries = [list(v) for v in entries]
    except TypeError:
        raise ValueError("FoldMutants: the variants of record {} are not a list of lists of (pos, letter)".format(name))
    off, pos, new = [0], [], []
    for v in entries:
        if not v:
            raise ValueError("FoldMutants: an empty variant of record {}".format(name))
        for site in v:
            try:
                p, ch = site
            except (TypeError, ValueError):
                raise ValueError("FoldMutants: {!r} of record {} is not a (pos, letter) substitution".format(site, name))
            if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= p < len(seq):
                raise ValueError("FoldMutants: position {!r} lies outside record {} (0-based, {} columns)".format(p, name, len(seq)))
            if seq[p] in GAPS or seq[p] in SEPS:
                raise ValueError("FoldMutants: position {} of record {} is a gap or separator character".format(p, name))
            if not isinstance(ch, str) or len(ch) != 1 or ord(ch) >= 128 or not _NORM[ord(ch)]:
                raise ValueError("FoldMutants: {!r} is not a letter to substitute (one of ACGU, acgu, T, t)".format(ch))
            pos.append(int(p)); new.append(_NORM[ord(ch)])
        if len({int(site[0]) for site in v}) != len(v):
            raise ValueError("FoldMutants: a variant of record {} names a position twice".format(name))
        off.append(len(pos))
    return np.array(off, np.int64), np.array(pos, np.int64), np.array(new, np.uint8)


def _variant_records(rec, site_off, site_pos, site_letter):
    """The variant records of one wild type: site_off int64[V + 1] into site_pos / site_letter (uint8 ASCII)."""
    name, seq, reacts, rests, _ = rec
    V, N = len(site_off) - 1, len(seq)
    codes = _codes(seq)
    given = _codes(seq.upper()) if len(seq.upper()) == N else codes   # (the label's letter: as given, upper-cased)
    var = np.repeat(np.arange(V), np.diff(site_off))
    labels = ["%s%d%s" % (chr(a), p + 1, chr(b)) for a, p, b in zip(given[site_pos].tolist(), site_pos.tolist(), site_letter.tolist())]
    out = []
    per = max(1, _CHUNK // max(N, 1))
    for lo in range(0, V, per):                                       # the sequences of `per` variants at once, as one array
        hi = min(V, lo + per)
        a, b = int(site_off[lo]), int(site_off[hi])
        block = np.tile(codes, (hi - lo, 1))
        block[var[a:b] - lo, site_pos[a:b]] = site_letter[a:b]
        text = block.tobytes().decode("utf-32-le")
        for k in range(lo, hi):
            label = "+".join(labels[int(site_off[k]):int(site_off[k + 1])])
            out.append((name + "/" + label, text[(k - lo) * N:(k - lo + 1) * N], reacts, rests, None))
    return out


def _host_diff(folds, R, wt_rec, pos_off):
    """(diff int32[V, 6], pos_changed int32[sum N]) with numpy from the consensus rows of a host FoldResult."""
    partner, cell_off, lengths = folds.partner.numpy(), folds._cell_off, folds._lengths
    V = len(wt_rec)
    diff = np.zeros((V, 6), np.int32)
    diff[:, 4:] = -1
    pos_changed = np.zeros(int(pos_off[-1]), np.int32)
    for r in range(R):
        mine = np.flatnonzero(wt_rec == r)
        n = int(lengths[r])
        if not len(mine) or not n:
            continue
        t = np.arange(n)
        w = partner[cell_off[r]:cell_off[r] + n][None, :]
        v = partner[cell_off[R + mine][:, None] + t[None, :]]
        up, changed = w > t, v != w
        diff[mine, 0] = (up & changed).sum(1)
        diff[mine, 1] = ((v > t) & changed).sum(1)
        diff[mine, 2] = (up & ~changed).sum(1)
        diff[mine, 3] = changed.sum(1)
        some = changed.any(1)
        diff[mine, 4] = np.where(some, changed.argmax(1), -1)
        diff[mine, 5] = np.where(some, n - 1 - changed[:, ::-1].argmax(1), -1)
        pos_changed[pos_off[r]:pos_off[r + 1]] = changed.sum(0)
    return diff, pos_changed


class MutantResult(TensorResult):
    """What ``FoldMutants`` computes for R records with V variants of S substitution sites in all.

    Host attributes: ``names``, ``sequences`` (the wild types'), ``mode`` ("scan" or "explicit"), ``source`` ("device" or
    "host": where the summary was formed) and ``folds``: the :class:`FoldResult` of the R wild types followed by the V
    variants, record after record, a variant named ``name/A12G`` (the letter as given upper-cased, the 1-based column, the new
    letter; several sites joined with ``+``).  Torch tensors on ``device``: ``pos_off`` int64[R + 1] -- the wild types'
    offsets on the axis on which they follow one another --, ``var_off`` int64[R + 1] -- the offsets of the records' variants
    --, ``site_off`` int64[V + 1] -- the offsets of the variants' sites --, ``site_pos`` int32[S], ``site_letter`` uint8[S]
    (ASCII of the new letter), ``diff`` int32[V, 6] -- per variant against the wild type's consensus row: the wild type's
    pairs it lacks, its pairs the wild type lacks, the pairs of both, the positions whose partner differs, the lowest and the
    highest of them (-1 without one) --, ``pos_changed`` int32[sum N] -- per wild-type position how many of its record's
    variants changed that position's partner; record r starts at pos_off[r]."""

    _TENSORS = ("pos_off", "var_off", "site_off", "site_pos", "site_letter", "diff", "pos_changed")
    _NESTED = ("folds",)

    def __init__(self, names, sequences, mode, source, folds, pos_off, var_off, site_off, site_pos, site_letter, diff, pos_changed):
        self.names, self.sequences, self.mode, self.source, self.folds = names, sequences, mode, source, folds
        self.pos_off, self.var_off, self.site_off, self.site_pos, self.site_letter = pos_off, var_off, site_off, site_pos, site_letter
        self.diff, self.pos_changed = diff, pos_changed
        # the host's copy of the offsets: the helpers below index with it
        self._var_off, self._site_off = var_off.cpu().numpy(), site_off.cpu().numpy()

    def __len__(self):
        return len(self.names)

    def _block(self, r, k=None):
        """The variants [lo, hi) of record r, or the one place of its variant k."""
        if not 0 <= r < len(self.names):
            raise IndexError("there are %d records" % len(self.names))
        lo, hi = int(self._var_off[r]), int(self._var_off[r + 1])
        if k is None:
            return lo, hi
        if not 0 <= k < hi - lo:
            raise IndexError("record %d has %d variants" % (r, hi - lo))
        return lo + k

    def variant(self, r, k):
        """(name, [(pos, from, to), ...]) of variant k of record r: the 0-based positions, the wild type's letters as given
        and the letters put there."""
        m = self._block(r, k)
        a, b = int(self._site_off[m]), int(self._site_off[m + 1])
        pos, new = self.site_pos[a:b].tolist(), self.site_letter[a:b].tolist()
        return self.folds.names[len(self.names) + m], [(p, self.sequences[r][p], chr(c)) for p, c in zip(pos, new)]

    def distance(self, r):
        """int32[V_r]: the base-pair distance lost + gained of every variant of record r to its wild type."""
        lo, hi = self._block(r)
        return self.diff[lo:hi, 0] + self.diff[lo:hi, 1]

    def dbn(self, r, k=None):
        """Dot-bracket line of record r's wild-type consensus, or of its variant k's."""
        if k is None:
            self._block(r)
            return self.folds.consensus(r)
        return self.folds.consensus(len(self.names) + self._block(r, k))

    def _scan_only(self, what):
        if self.mode != "scan":
            raise ValueError("MutantResult.{} is defined for scans only: explicit variants may have several sites".format(what))

    def to_matrix(self, r):
        """int32[N, 4] on the tensors' device: the distance of record r's variant by position x new letter (A, C, G, U), -1
        for the position's own letter and for positions that were not scanned.  Scan mode only."""
        import torch
        self._scan_only("to_matrix")
        lo, hi = self._block(r)                                      # (a scan's variants have one site each: sites lo .. hi)
        out = torch.full((len(self.sequences[r]), 4), -1, dtype=torch.int32, device=self.device)
        column = torch.from_numpy(_COLUMN).to(self.device)
        out[self.site_pos[lo:hi].long(), column[self.site_letter[lo:hi].long()]] = self.distance(r)
        return out

    def profile(self, r):
        """float64[N, 2] on the tensors' device: the mean and the largest distance over the position's variants, NaN for a
        position without one.  Scan mode only."""
        import torch
        self._scan_only("profile")
        m = self.to_matrix(r).double()
        have = m >= 0
        count = have.sum(1).double()
        mean = torch.where(have, m, torch.zeros_like(m)).sum(1) / count          # (0 / 0: NaN where there is none)
        top = torch.where(count > 0, m.max(1)[0], torch.full_like(count, float("nan")))
        return torch.stack((mean, top), 1)

    def most_disruptive(self, r, n=10):
        """int64[min(n, V_r)]: the variants of record r with the largest distance, ties to the lower index."""
        import torch
        return torch.sort(self.distance(r), descending=True, stable=True)[1][:max(int(n), 0)]


def FoldMutants(inputfile=None, inputseq=None, records=None, positions=None, variants=None, inputformat="qtrf",
                fileformat="unknown", ignorewarn=False, M=1.8, B=-0.6, **fold_keywords):
    """Fold every input record beside its substitution variants and return a :class:`MutantResult`.

    The inputs are ``Fold``'s (``inputfile`` / ``inputseq`` / ``records``, parsed as there).  Scan mode (``variants`` None):
    every position whose letter, upper-cased with T for U, is one of ACGU gets the three other letters, in the order A, C, G,
    U, written as upper-case RNA letters; gap, separator and other characters are not substituted and stay where they are.
    ``positions``: 0-based ints applied to every record (None: all); duplicates are dropped, the order is ascending.  Explicit
    mode: ``variants`` holds per record a list of variants, each a non-empty sequence of ``(pos, letter)`` with distinct
    positions, none on a gap or separator character; a substitution by the position's own letter is allowed.

    A variant is the record ``(name/label, substituted sequence, the wild type's reactivities, its restraints, None)``; the
    wild types and all variants go through one ``Fold`` call, to which every other keyword is forwarded unchanged (validation
    and messages are ``Fold``'s).  A record's structure is its consensus row.  ``bpp`` raises ValueError: a wild type's
    matrix is not its variants'."""
    import torch
    if variants is not None and positions is not None:
        raise ValueError("FoldMutants: positions belong to a scan; with variants given they must be None")
    inputs, kw = derived_inputs("FoldMutants", records, inputfile, inputseq, inputformat, fileformat, ignorewarn, M, B, fold_keywords)

    # ---- the variants
    names, seqs = [rec[0] for rec in inputs], [rec[1] for rec in inputs]
    R = len(inputs)
    (pos_off, Ltot), var_off = position_axis(seqs), np.zeros(R + 1, np.int64)
    if variants is None:
        scan = _scan_positions(positions, min(len(s) for s in seqs))
    else:
        try:
            variants = list(variants)
        except TypeError:
            variants = None
        if variants is None or len(variants) != R:
            raise ValueError("FoldMutants: variants must hold one list per record ({} records)".format(R))
    vrecs, offs, sites, news, nsites = [], [], [], [], 0
    for r, rec in enumerate(inputs):
        letters = _normalised(_codes(seqs[r]))
        if variants is None:
            at = np.flatnonzero(letters) if scan is None else scan[letters[scan] != 0]
            other = _CODES[None, :] != letters[at][:, None]            # (the three other letters, in the order A, C, G, U)
            site_pos, site_letter = np.repeat(at, 3), np.broadcast_to(_CODES, (len(at), 4))[other]
            site_off = np.arange(3 * len(at) + 1, dtype=np.int64)
        else:
            site_off, site_pos, site_letter = _explicit_sites(names[r], seqs[r], variants[r])
        vrecs += _variant_records(rec, site_off, site_pos, site_letter)
        var_off[r + 1] = var_off[r] + len(site_off) - 1
        offs.append(site_off[1:] + nsites); sites.append(site_pos); news.append(site_letter)
        nsites += len(site_pos)
    V = int(var_off[-1])
    site_off = np.concatenate([np.zeros(1, np.int64)] + offs)
    wt_rec = np.repeat(np.arange(R), np.diff(var_off))

    folds = _fold.Fold(records=[tuple(rec) for rec in inputs] + vrecs, **kw)
    assert folds._lengths[R:].tolist() == folds._lengths[wt_rec].tolist(), "a variant's table does not have its wild type's length"

    eng = _engine.get_engine()
    on_device = all(hasattr(eng, m) for m in _DEVICE_METHODS) and folds.partner.is_cuda
    dev = folds.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pos_off = up(pos_off)
    if on_device:
        diff, pos_changed = eng.variant_diff(folds.partner, folds.cell_off, folds.lengths, R, up(wt_rec.astype(np.int32)), d_pos_off, Ltot)
    else:
        diff, pos_changed = (torch.from_numpy(a) for a in _host_diff(folds, R, wt_rec, pos_off))
    return MutantResult(names, seqs, "scan" if variants is None else "explicit", "device" if on_device else "host", folds, d_pos_off,
                        up(var_off), up(site_off), up(np.concatenate(sites).astype(np.int32)), up(np.concatenate(news).astype(np.uint8)),
                        diff, pos_changed)
