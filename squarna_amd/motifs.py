"""G-quadruplex and protein-binding motif restraints (the ``g4`` / ``rbp`` options, SQRNrfam.py:118-269).

Both are pattern searches over one ungapped sequence whose result is a restraint line: ``+`` marks positions the fold
must leave unpaired, and a Fab hit also forces one base pair.  ``Predict`` runs them for a single input record only
(SQUARNA.py:850-866) and prints the hits as the restraint line's label.

The shapes are kept as data and matched by an explicit scan that makes the choices Python's ``re`` makes for the
reference's overlapping-lookahead patterns: a match is tried at every start position; G-runs are greedy (longest
first) and loops are lazy (shortest first), and the first decomposition in that order is the one that is scored and
marked.  A failing (element, position) state fails from every start, so it is remembered once per sequence: the scan
is linear in the sequence length.
"""
from .dbn import GAPS, SEPS, ReAlign

#: the two G-quadruplex shapes: four G-runs of run_min..run_max separated by loops of loop_min..loop_max word characters
G4_SHAPES = (
    dict(run_min=2, run_max=5, loop_min=1, loop_max=2),
    dict(run_min=3, run_max=5, loop_min=1, loop_max=12),
)
G4_SCORE_LIMIT = 1.2
G4_LABEL = "G4(+)"

#: protein-binding motifs in search order: (protein, motif in IUPAC letters over ACGU, whether a hit forces the pair of
#: its two end positions)
RBP_MOTIFS = (
    ("U1A", "AUUGCAC", False),
    ("LIN28", "GGAGA", False),
    ("RBFOX1/2", "UGCAUG", False),
    ("PUM", "UGUAHAUW", False),
    ("SF1/QKI", "ACUAAC", False),
    ("Fab", "GAAACAC", True),
)
_IUPAC = {"H": "ACU", "W": "AU"}


def _is_word(ch):
    """One character of re's ``\\w`` on str patterns."""
    return ch.isalnum() or ch == '_'


def _short_seq(seq):
    """The searched sequence: gaps dropped, separators as N, upper case (SQRNrfam.py:171,240)."""
    return ''.join(x if x not in SEPS else "N" for x in seq if x not in GAPS).upper()


def G4Hscore(match):
    """G4Hunter-style score: every maximal run of G (or of C) adds (or subtracts) len * min(len, 4); divided by the
    length of the match."""
    total, k, n = 0, 0, len(match)
    while k < n:
        ch = match[k]
        if ch != 'G' and ch != 'C':
            k += 1
            continue
        end = k
        while end < n and match[end] == ch:
            end += 1
        ln = end - k
        total += (ln if ch == 'G' else -ln) * min(ln, 4)
        k = end
    return total / n


def _run_lengths(seq, pred):
    """out[i] = number of consecutive positions from i on where pred holds (out[len(seq)] = 0)."""
    out = [0] * (len(seq) + 1)
    for i in range(len(seq) - 1, -1, -1):
        if pred(seq[i]):
            out[i] = out[i + 1] + 1
    return out


def _g4_decompose(start, shape, gruns, words, dead):
    """Segment lengths (run, loop, run, loop, run, loop, run) of the first match at `start` in re's backtracking order,
    or None.  `dead`: the (element, position) states known to fail, shared by every start of one shape."""
    rmin, rmax, lmin, lmax = shape["run_min"], shape["run_max"], shape["loop_min"], shape["loop_max"]

    def from_(k, i):
        if (k, i) in dead:
            return None
        if k % 2 == 0:                                          # G-run: longest first
            for ln in range(min(gruns[i], rmax), rmin - 1, -1):
                if k == 6:
                    return [ln]
                rest = from_(k + 1, i + ln)
                if rest is not None:
                    return [ln] + rest
        else:                                                   # loop: shortest first
            for ln in range(lmin, min(words[i], lmax) + 1):
                rest = from_(k + 1, i + ln)
                if rest is not None:
                    return [ln] + rest
        dead.add((k, i))
        return None

    return from_(0, start)


def FindG4(seq, g4sym='+', scorelim=G4_SCORE_LIMIT):
    """(line, found): the G-runs of every G-quadruplex match of either shape scoring >= scorelim marked g4sym."""
    n = len(seq)
    gruns = _run_lengths(seq, lambda ch: ch == 'G')
    words = _run_lengths(seq, _is_word)
    line = ['.'] * n
    found = False
    for shape in G4_SHAPES:
        dead = set()
        for start in range(n):
            segs = _g4_decompose(start, shape, gruns, words, dead)
            if segs is None or G4Hscore(seq[start:start + sum(segs)]) < scorelim:
                continue
            found = True
            cur = start
            for k, ln in enumerate(segs):
                if k % 2 == 0:
                    for i in range(cur, cur + ln):
                        line[i] = g4sym
                cur += ln
    return ''.join(line), found


def _motif_hits(seq, motif):
    classes = [_IUPAC.get(ch, ch) for ch in motif]
    m = len(classes)
    return [p for p in range(len(seq) - m + 1) if all(seq[p + q] in classes[q] for q in range(m))]


def FindRBP(seq, emptysym='.'):
    """(line, hits): every (overlapping) motif hit marked '+', a pair-forcing hit's ends as '(' ')'; hits as
    "PROT(start-end)" (1-based), comma-joined, in motif order."""
    line = [emptysym] * len(seq)
    found = []
    for prot, motif, pairs in RBP_MOTIFS:
        for start in _motif_hits(seq, motif):
            end = start + len(motif)
            found.append("{}({}-{})".format(prot, start + 1, end))
            for i in range(start, end):
                line[i] = '+'
            if pairs:
                line[start] = '('
                line[end - 1] = ')'
    return ''.join(line), ','.join(found)


def SearchG4RBP(seq, g4, rbp):
    """(restraints or None, label or False) for a (possibly gapped) input sequence (SQRNrfam.py:259-260 without rfam).
    With both searches the RBP characters win over the G4 ones and the label is "<rbp hits>,G4(+)"."""
    restraints, label = None, False
    if g4:
        marks, found = FindG4(_short_seq(seq))
        if found:
            restraints, label = ReAlign(marks, seq), G4_LABEL
    if rbp:
        marks, hits = FindRBP(_short_seq(seq).replace('T', 'U'))
        if hits:
            line = ReAlign(marks, seq)
            if label:
                line = ''.join(ch if ch != '.' else restraints[i] for i, ch in enumerate(line))
                hits = hits + ',' + label
            restraints, label = line, hits
    return restraints, label
