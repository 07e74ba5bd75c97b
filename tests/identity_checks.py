"""What the row-identity tests share: the definitions of RowIdentity restated in plain Python strings, and the alignments.

The NAIVE reference zips two normalised rows, counts the columns and runs the greedy filter as a loop over a list of kept
rows: no matrix, no bit.  Its cost is R^2 L character comparisons, so it is for the small shapes of these tests."""
import random

from tests.covariation_checks import ALPHABET, GAPS, normalise, random_rows  # noqa: F401

BASES = "ACGU"
DENOMINATORS = ("shorter", "aligned", "columns")


def same_of(p, q):
    """The columns where two normalised rows hold the same base."""
    return sum(x == y and x in BASES for x, y in zip(p, q))


def both_of(p, q):
    """The columns where two normalised rows both hold a residue (any non-gap)."""
    return sum(x not in GAPS and y not in GAPS for x, y in zip(p, q))


_MEMO = {}
_COUNTS = {}


def naive_counts(rows):
    """(same, both) as lists of lists: every pair of rows zipped once (both counts are symmetric), once per alignment."""
    key = tuple(rows)
    if key not in _COUNTS:
        rows = [normalise(r) for r in rows]
        R = len(rows)
        same, both = [[0] * R for _ in range(R)], [[0] * R for _ in range(R)]
        for a in range(R):
            for b in range(a, R):
                same[a][b] = same[b][a] = same_of(rows[a], rows[b])
                both[a][b] = both[b][a] = both_of(rows[a], rows[b])
        if len(_COUNTS) > 64:
            _COUNTS.clear()
        _COUNTS[key] = (same, both)
    return _COUNTS[key]


def naive(rows, denominator="shorter", T=8000, matrix=True):
    """dict(len, bases, neighbours, keep, same, both) of the rows as host lists (same / both: lists of lists, or None)."""
    key = (tuple(rows), denominator, T, matrix)
    if key in _MEMO:
        return _MEMO[key]
    R, L = len(rows), len(rows[0])
    same, both = naive_counts(rows)
    length = [both[a][a] for a in range(R)]
    den = lambda a, b: min(length[a], length[b]) if denominator == "shorter" else both[a][b] if denominator == "aligned" else L
    near = [[a != b and den(a, b) > 0 and same[a][b] * 10000 >= T * den(a, b) for b in range(R)] for a in range(R)]
    kept = []
    for a in range(R):
        if not any(near[a][b] for b in kept):
            kept.append(a)
    out = dict(len=length, bases=[same[a][a] for a in range(R)], neighbours=[1 + sum(n) for n in near],
               keep=[a in kept for a in range(R)], same=same if matrix else None, both=both if matrix else None)
    if len(_MEMO) > 256:
        _MEMO.clear()
    _MEMO[key] = out
    return out


def family_rows(seed, R, L, families=3, rate=0.1, alphabet="ACGU-"):
    """R rows of L characters in `families` families of near-duplicates: every row is its family's founder with each column
    redrawn from `alphabet` with probability `rate`, the families dealt in random order."""
    rng = random.Random(seed)
    founders = ["".join(rng.choice(alphabet) for _ in range(L)) for _ in range(max(families, 1))]
    return ["".join(rng.choice(alphabet) if rng.random() < rate else ch for ch in rng.choice(founders)) for _ in range(R)]


def mixed_rows(seed, R, L):
    """Near-duplicate families over the whole test alphabet with a few unrelated rows in between."""
    rows = family_rows(seed, R, L, families=max(R // 20, 2), rate=0.12, alphabet=ALPHABET)
    noise = random_rows(seed + 1, R, L, helices=0)
    return [noise[k] if k % 7 == 3 else rows[k] for k in range(R)]


def chain_rows(n):
    """n rows of 2 (n + 1) columns in which row k is a neighbour of the rows k - 1 and k + 1 only, at T = 5000 under "shorter"
    and "aligned": row k holds A in the four columns 2 k .. 2 k + 3 and gaps elsewhere, so rows k and k + 1 share two of their
    four residues (identity 2 / 4, or 2 / 2 over the aligned columns) and rows further apart share none (den 0 or same 0)."""
    L = 2 * (n + 1)
    return ["-" * (2 * k) + "AAAA" + "-" * (L - 2 * k - 4) for k in range(n)]


def check_result(got, exp, what=""):
    """A result's tensors (as host lists: got = dict of lists) against the reference dict, exactly."""
    for key in ("len", "bases", "neighbours", "keep", "same", "both"):
        assert got[key] == exp[key], (what, key)


def as_lists(res):
    """An IdentityResult, or a dict of tensors, as a dict of host lists."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    return {k: None if get(k) is None else get(k).tolist() for k in ("len", "bases", "neighbours", "keep", "same", "both")}
