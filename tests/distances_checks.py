"""What the structure-distance tests share: the definitions of Distances restated on Python sets of pairs, and the structures.

The NAIVE reference parses dot-bracket strings into sets of pairs with one stack per bracket kind, intersects the sets of
every two rows of a group and runs the greedy filter as a loop over a list of kept rows: no matrix product, no bit.  A row
given as None stands for an invalid row.  Its cost is the square of a group's rows, so it is for the small shapes of these
tests."""
import random

KINDS = ("()", "[]", "{}", "<>") + tuple(c + c.lower() for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZ")
MODES = ("radius", "relative")


def pairs_of(dbn):
    """The set of pairs (i, j), i < j, of a dot-bracket string."""
    opener, closer, stacks, pairs = {k[0]: k for k in KINDS}, {k[1]: k for k in KINDS}, {}, set()
    for i, ch in enumerate(dbn):
        if ch in opener:
            stacks.setdefault(opener[ch], []).append(i)
        elif ch in closer:
            pairs.add((stacks[closer[ch]].pop(), i))
        else:
            assert ch == ".", ch
    assert not any(stacks.values()), dbn
    return frozenset(pairs)


def partners_of(dbn):
    """The partner row of a dot-bracket string as a list."""
    row = [-1] * len(dbn)
    for i, j in pairs_of(dbn):
        row[i], row[j] = j, i
    return row


def near(mode, threshold, na, nb, common):
    d = na + nb - 2 * common
    return d <= threshold if mode == "radius" else d * 10000 <= threshold * (na + nb)


_MEMO = {}


def naive(groups, mode="radius", threshold=0, matrix=True):
    """dict(status, npairs, neighbours, leader, keep, common) of the groups (a list per group of dot-bracket strings, None for
    an invalid row) as host lists; row indices are global; common is the flat block-diagonal matrix (or None)."""
    key = (tuple(tuple(g) for g in groups), mode, threshold, matrix)
    if key in _MEMO:
        return _MEMO[key]
    out = dict(status=[], npairs=[], neighbours=[], leader=[], keep=[], common=[] if matrix else None)
    first = 0
    for rows in groups:
        sets = [None if r is None else pairs_of(r) for r in rows]
        n = len(rows)
        common = [[0 if sets[a] is None or sets[b] is None else len(sets[a] & sets[b]) for b in range(n)] for a in range(n)]
        count = [0 if s is None else len(s) for s in sets]
        close = [[a != b and sets[a] is not None and sets[b] is not None and near(mode, threshold, count[a], count[b], common[a][b])
                  for b in range(n)] for a in range(n)]
        kept = []
        for a in range(n):
            if sets[a] is None:
                out["leader"].append(-1)
                continue
            led = [b for b in kept if close[a][b]]
            if not led:
                kept.append(a)
            out["leader"].append(first + (led[0] if led else a))
        out["status"] += [int(s is None) for s in sets]
        out["npairs"] += count
        out["neighbours"] += [0 if sets[a] is None else 1 + sum(close[a]) for a in range(n)]
        out["keep"] += [a in kept for a in range(n)]
        if matrix:
            out["common"] += [c for row in common for c in row]
        first += n
    if len(_MEMO) > 256:
        _MEMO.clear()
    _MEMO[key] = out
    return out


def distance_matrix(rows):
    """The base-pair distances of one group of valid rows as a list of lists."""
    sets = [pairs_of(r) for r in rows]
    return [[len(a ^ b) for b in sets] for a in sets]


def random_structure(rng, L, knots=False, density=0.3):
    """A random structure of L columns: round brackets opened and closed along a random walk over the columns, and with
    `knots` square and curly brackets laid in the same way over the columns left unpaired (they cross the round ones)."""
    row = ["."] * L
    for kind in KINDS[:3 if knots else 1]:
        stack = []
        for c in range(L):
            if row[c] != ".":
                continue
            x = rng.random()
            if x < density:
                stack.append(c)
            elif x < 2 * density and stack:
                row[stack.pop()], row[c] = kind[0], kind[1]
    return "".join(row)


def edited(rng, dbn, edits):
    """The structure after `edits` pair edits: a pair removed, or a pair of a letter kind of its own added on two unpaired
    columns."""
    row, letters = list(dbn), [k for k in KINDS[4:] if k[0] not in dbn]
    for _ in range(edits):
        pairs, free = sorted(pairs_of("".join(row))), [c for c, ch in enumerate(row) if ch == "."]
        if pairs and (rng.random() < 0.5 or len(free) < 2 or not letters):
            i, j = rng.choice(pairs)
            row[i] = row[j] = "."
        elif len(free) >= 2 and letters:
            i, j = sorted(rng.sample(free, 2))
            kind = letters.pop()
            row[i], row[j] = kind[0], kind[1]
    return "".join(row)


def random_rows(seed, n, L, knots=False):
    rng = random.Random(seed)
    return [random_structure(rng, L, knots) for _ in range(n)]


def family_rows(seed, n, L, families=3, edits=2, knots=False):
    """n rows of L columns in `families` families: every row is its family's founder after up to `edits` pair edits (so that
    identical rows occur), the families dealt in random order."""
    rng = random.Random(seed)
    founders = [random_structure(rng, L, knots) for _ in range(max(families, 1))]
    return [edited(rng, rng.choice(founders), rng.randrange(edits + 1)) for _ in range(n)]


def chain_rows(n):
    """n rows of 2 (n + 1) columns in which row k is a neighbour of the rows k - 1 and k + 1 only, at radius 2 and at
    relative 0.5: row k holds the two pairs (2 k, 2 k + 1) and (2 k + 2, 2 k + 3), so rows k and k + 1 share one of their two
    pairs (distance 2 of 4) and rows further apart share none (distance 4 of 4)."""
    L = 2 * (n + 1)
    return ["." * (2 * k) + "()()" + "." * (L - 2 * k - 4) for k in range(n)]


KEYS = ("status", "npairs", "neighbours", "leader", "keep", "common")


def check_result(got, exp, what=""):
    """A result's tensors (as host lists: got = dict of lists) against the reference dict, exactly."""
    for key in KEYS:
        assert got[key] == exp[key], (what, key)


def as_lists(res):
    """A DistancesResult, or a dict of tensors, as a dict of host lists."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    return {k: None if get(k) is None else get(k).tolist() for k in KEYS}
