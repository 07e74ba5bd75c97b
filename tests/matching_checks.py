"""Checks shared by the CPU and GPU tests of the graph-level matching entries (tests/test_matching_reference.py,
tests/test_hip_matching_many.py): ctypes wrappers that hand sq_lsap / sq_nussinov / sq_mwm SEVERAL problems per call (the
drop-ins of squarna_amd/core.py always pass one), the references they are judged by -- scipy's linear_sum_assignment on the
dense matrix, a plain fp64 Nussinov DP, the oracle's Nussinov, networkx's max_weight_matching -- and seeded generators of
adversarial inputs: arbitrary sparse cells, weights from small sets of multiples of 1/8 (every sum exact, ties everywhere),
repeated cells.  Not a test module."""
import ctypes as C

import numpy as np

#: weight families: multiples of 1/8, so sums of any number of them in any order are exact in fp64
DYADIC = ((1.0,), (1.0, 2.0), (0.5, 1.5, 3.5, 4.0))
#: ... and one without ties: rng.random() (None as a family)
CONTINUOUS = None


# ------------------------------------------------------------------ the C entries, several problems per call
def _arr(values, dtype):
    """A contiguous array with one spare element, so that the pointer of an empty list is still a valid one."""
    a = np.zeros(len(values) + 1, dtype)
    a[:len(values)] = values
    return a


def _workspace(nbytes, ws_short=0, ws_shift=0):
    """(keep-alive, pointer, bytes, stream): device scratch as core.py takes it; ws_short / ws_shift make it `ws_short` bytes
    too small / move the pointer by `ws_shift` bytes (the refusals of the entries)."""
    from squarna_amd.core import _device_workspace
    ws, ptr, stream = _device_workspace(nbytes + abs(ws_shift))
    return ws, ptr + ws_shift, nbytes - ws_short, stream


def _flatten(cell_lists):
    off = np.zeros(len(cell_lists) + 1, np.int64)
    np.cumsum([len(c) for c in cell_lists], out=off[1:])
    flat = [c for cells in cell_lists for c in cells]
    return (off, _arr([c[0] for c in flat], np.int32), _arr([c[1] for c in flat], np.int32),
            _arr([c[2] for c in flat], np.float64))


def lsap_many(problems, ws_short=0, ws_shift=0):
    """sq_lsap on [(n, [(v, w, weight), ...]), ...] in ONE call: the col4row slice of every problem (lists of ints)."""
    from squarna_amd import _lib
    L = _lib.load()
    ns = _arr([p[0] for p in problems], np.int32)
    off, cv, cw, wt = _flatten([p[1] for p in problems])
    nbytes = C.c_size_t(0)
    _lib.check(L.sq_lsap_workspace_bytes(len(problems), ns.ctypes.data, off.ctypes.data, C.byref(nbytes)))
    ws, ptr, have, stream = _workspace(nbytes.value, ws_short, ws_shift)
    total = int(sum(p[0] for p in problems))
    sol = np.full(total + 1, -7, np.int32)
    _lib.check(L.sq_lsap(len(problems), ns.ctypes.data, off.ctypes.data, cv.ctypes.data, cw.ctypes.data, wt.ctypes.data,
                         sol.ctypes.data, C.c_void_p(ptr), C.c_size_t(have), C.c_void_p(stream)))
    assert sol[total] == -7                                  # nothing written past the last problem
    out, at = [], 0
    for n, _ in problems:
        out.append(sol[at:at + n].tolist())
        at += n
    return out


def _pair_lists(pairs, poff, count):
    poff = poff[:count + 1].tolist()
    assert poff[0] == 0 and all(a <= b for a, b in zip(poff, poff[1:])), poff        # non-decreasing, ends at the total
    return [[(int(pairs[2 * k]), int(pairs[2 * k + 1])) for k in range(poff[g], poff[g + 1])] for g in range(count)], poff[-1]


def nussinov_many(problems, ws_short=0, ws_shift=0, pair_cap=None):
    """sq_nussinov on [(seq, [(v, w, score), ...]), ...] in ONE call (n = len(seq)): the sorted pair list of every problem."""
    from squarna_amd import _lib
    from squarna_amd.dbn import encode_seq
    L = _lib.load()
    ns = _arr([len(p[0]) for p in problems], np.int32)
    codes = _arr(list(b"".join(encode_seq(p[0]) for p in problems)), np.uint8)
    off, cv, cw, sc = _flatten([p[1] for p in problems])
    nbytes = C.c_size_t(0)
    _lib.check(L.sq_nussinov_workspace_bytes(len(problems), ns.ctypes.data, off.ctypes.data, C.byref(nbytes)))
    ws, ptr, have, stream = _workspace(nbytes.value, ws_short, ws_shift)
    cap = int(sum(len(p[0]) + 4 for p in problems)) if pair_cap is None else pair_cap
    pairs = np.zeros(2 * max(cap, 0) + 2, np.int32)
    poff = np.full(len(problems) + 2, -7, np.int64)
    _lib.check(L.sq_nussinov(len(problems), ns.ctypes.data, codes.ctypes.data, off.ctypes.data, cv.ctypes.data, cw.ctypes.data,
                             sc.ctypes.data, pairs.ctypes.data, cap, poff.ctypes.data, C.c_void_p(ptr), C.c_size_t(have),
                             C.c_void_p(stream)))
    assert poff[len(problems) + 1] == -7
    return _pair_lists(pairs, poff, len(problems))[0]


def mwm_many(graphs, ws_short=0, ws_shift=0, pair_cap=None):
    """sq_mwm on [[(u, v, weight), ...], ...] in ONE call: (pair lists as the entry orders them, pair_off as a list)."""
    from squarna_amd import _lib
    L = _lib.load()
    off, eu, ev, ew = _flatten(graphs)
    nbytes = C.c_size_t(0)
    _lib.check(L.sq_mwm_workspace_bytes(len(graphs), off.ctypes.data, eu.ctypes.data, ev.ctypes.data, C.byref(nbytes)))
    ws, ptr, have, stream = _workspace(nbytes.value, ws_short, ws_shift)
    cap = int(off[-1]) + 1 if pair_cap is None else pair_cap
    pairs = np.zeros(2 * max(cap, 0) + 2, np.int32)
    poff = np.full(len(graphs) + 2, -7, np.int64)
    _lib.check(L.sq_mwm(len(graphs), off.ctypes.data, eu.ctypes.data, ev.ctypes.data, ew.ctypes.data, pairs.ctypes.data, cap,
                        poff.ctypes.data, C.c_void_p(ptr), C.c_size_t(have), C.c_void_p(stream)))
    assert poff[len(graphs) + 1] == -7
    lists, total = _pair_lists(pairs, poff, len(graphs))
    assert total == sum(len(p) for p in lists)
    return lists, poff[:len(graphs) + 1].tolist()


def last_error():
    from squarna_amd import _lib
    return _lib.load().sq_last_error().decode()


# ------------------------------------------------------------------ the storage forms of sq_lsap_kernel
LSAP_LDS_CAP = 150 * 1024


def lsap_vec_bytes(n):
    """sq_lsap_vec_bytes of csrc/sq_match.h: the row / column vectors of one problem."""
    return (n * (3 * 8 + 4 * 4 + 2) + 15) & ~15


def lsap_lds_bytes(n, m):
    """sq_lsap_lds_bytes of csrc/sq_match.h: the vectors and the sparse matrix of one problem (m distinct cells)."""
    nw = (n + 31) // 32
    sparse = m * 8 + n * nw * 4 + (((n + 1) * 2 + 3) & ~3) + ((n * nw * 2 + 3) & ~3) + m * 4 + 16
    return lsap_vec_bytes(n) + sparse + 64


def lsap_form(n, m, launch):
    """'a' (sparse matrix and vectors in LDS), 'b' (dense cost in global memory, vectors in LDS) or 'c' (all in global
    memory): the form sq_lsap_kernel takes for a problem of size n with m distinct cells in a launch whose problems are
    `launch` = [(n, m), ...] -- sq_launch_matching's launch-wide LDS size, then the kernel's two tests."""
    lds = max(lsap_lds_bytes(a, b) for a, b in launch)
    if lds > LSAP_LDS_CAP:
        lds = min(lsap_vec_bytes(max(a for a, _ in launch)) + 64, LSAP_LDS_CAP)
    if lsap_vec_bytes(n) + 64 > lds:
        return "c"
    return "a" if m < 32767 and lsap_lds_bytes(n, m) <= lds else "b"


# ------------------------------------------------------------------ references
def dedup_cells(cells):
    """{(v, w) with v < w: weight}: a repeated cell -- in either orientation -- takes the last weight."""
    out = {}
    for v, w, x in cells:
        out[(min(v, w), max(v, w))] = x
    return out


def scipy_col_ind(n, cells):
    """col_ind of scipy.optimize.linear_sum_assignment on the dense matrix SQRNalgos.Hungarian builds (:119-124)."""
    from scipy.optimize import linear_sum_assignment
    mat = np.zeros((n, n))
    for (v, w), x in dedup_cells(cells).items():
        mat[v, w] = mat[w, v] = -x
    row_ind, col_ind = linear_sum_assignment(mat)
    assert row_ind.tolist() == list(range(n))
    return col_ind.tolist()


def nussinov_optimum(n, cells):
    """D[0][n-1] of the recursion D[i][j] = min(D[i][j-1], min over cells (k, j) with i <= k < j - 1 of
    D[i][k-1] + D[k+1][j-1] - score), empty intervals 0, in fp64: column after column, per column the list of its cells,
    all rows i of a cell at once.  E[i][j + 1] holds D[i][j], so that E[i][i] is the empty interval before i."""
    if n < 2:
        return 0.0
    cols = [[] for _ in range(n)]
    for (k, j), s in dedup_cells(cells).items():
        cols[j].append((k, s))
    E = np.zeros((n + 1, n + 1))
    for j in range(1, n):
        col = E[:, j].copy()                                 # D[i][j-1]
        for k, s in cols[j]:
            if k < j - 1:
                col[:k + 1] = np.minimum(col[:k + 1], E[:k + 1, k] + E[k + 1, j] - s)
        E[:j, j + 1] = col[:j]
    return float(E[0, n])


def oracle_nussinov(seq, cells):
    """The exact pair list: oracle.sqrn_oracle.Nussinov on one-cell stems (a later cell overwrites an earlier one)."""
    from oracle import sqrn_oracle as O
    return O.Nussinov(seq, [(v, w, 1, x) for v, w, x in cells], len(seq))


def networkx_pairs(edges):
    """sorted(networkx.max_weight_matching(G)) as SQRNalgos.Edmonds forms it (:96-110): pairs with their orientation."""
    import networkx as nx
    G = nx.Graph()
    G.add_weighted_edges_from(edges)
    return sorted(nx.max_weight_matching(G))


def check_nussinov_pairs(n, cells, pairs):
    """What an optimal answer of a separator-free problem whose cells all span >= 4 has to be: pairs that are cells of the
    input, vertex-disjoint, pairwise nested or side by side, with scores that sum to -nussinov_optimum exactly."""
    score = dedup_cells(cells)
    assert all(p in score for p in pairs), [p for p in pairs if p not in score]
    ends = [x for p in pairs for x in p]
    assert len(set(ends)) == len(ends), pairs
    for a, (i, j) in enumerate(pairs):
        for k, l in pairs[a + 1:]:
            assert not (i < k < j < l or k < i < l < j), ((i, j), (k, l))        # no crossing
    assert sum(score[p] for p in pairs) == -nussinov_optimum(n, cells), (n, pairs)


# ------------------------------------------------------------------ generators
def _weight(rng, family):
    return float(rng.random()) if family is None else float(family[rng.integers(len(family))])


def nussinov_case(seed, n, ncells, family=DYADIC[2], seps=False, repeats=0.15):
    """(seq, cells) of length n: about `ncells` random cells v < w with w - v >= 4 and scores of `family`, a share of them
    listed again later with another score.  seps: ';' and '&' in the sequence and also cells of span 2 and 3, which
    BackTrack reaches only across a separator (compare such a case with the oracle only)."""
    rng = np.random.default_rng(seed)
    seq = [("A", "C", "G", "U")[int(x)] for x in rng.integers(4, size=n)]
    span = 2 if seps else 4
    cells = []
    if n > span:
        for _ in range(ncells):
            v = int(rng.integers(0, n - span))
            w = int(rng.integers(v + span, n))
            cells.append((v, w, _weight(rng, family)))
        for c in range(len(cells)):
            if rng.random() < repeats:
                v, w, x = cells[c]
                cells.append((v, w, x + float(family[rng.integers(len(family))])))
        order = rng.permutation(len(cells))
        cells = [cells[int(t)] for t in order]
    if seps and n >= 3:
        for t in range(max(1, n // 40)):
            seq[int(rng.integers(1, n - 1))] = ";&"[t % 2]
    return "".join(seq), cells


def lsap_case(seed, n, m, family=DYADIC[2], flips=0.3, repeats=0.1):
    """(n, cells): m distinct random off-diagonal cells with weights of `family` (None: rng.random(), a unique optimum among
    the non-zero cells), a share listed as (w, v), a share listed again -- in either orientation -- with another weight."""
    rng = np.random.default_rng(seed)
    m = min(m, n * (n - 1) // 2)
    cells = []
    if m:
        if 4 * m >= n * (n - 1) // 2:                        # dense: draw from all cells
            allc = [(v, w) for v in range(n - 1) for w in range(v + 1, n)]
            pick = [allc[int(t)] for t in rng.permutation(len(allc))[:m]]
        else:
            seen = set()
            while len(seen) < m:
                v, w = (int(x) for x in rng.integers(n, size=2))
                if v != w:
                    seen.add((min(v, w), max(v, w)))
            pick = sorted(seen)
            pick = [pick[int(t)] for t in rng.permutation(m)]
        cells = [(v, w, _weight(rng, family)) for v, w in pick]
        for c in range(m):
            if rng.random() < repeats:
                v, w, x = cells[c]
                cells.append((v, w, _weight(rng, family) + (0.0 if family is None else x)))
        cells = [(w, v, x) if rng.random() < flips else (v, w, x) for v, w, x in cells]
    return n, cells


def mwm_case(seed, n, zero_edges=False, repeat_edge=False):
    """Edge list of a graph on n vertices in the style of test_blossom_several_vertices_per_pass_matches_networkx: low degree,
    few distinct weights, hubs, neighbours of neighbours; labels 3 v + 7 over a shuffled numbering, edges in shuffled order."""
    rng = np.random.default_rng(seed)
    if zero_edges:
        return []
    label = [3 * int(v) + 7 for v in rng.permutation(n)]
    deg = (1, 2, 3, 4, 6)[int(rng.integers(5))]
    family = (DYADIC + ((1.0, 2.0, 3.0, 4.0),))[int(rng.integers(4))]
    hubs = [int(h) for h in rng.permutation(n)[:int(rng.integers(0, 3))]]
    pairs = set()
    for v in range(n):
        for _ in range(int(rng.integers(1, deg + 1))):
            w = hubs[int(rng.integers(len(hubs)))] if hubs and rng.random() < 0.25 else int(rng.integers(n))
            if rng.random() < 0.4:
                w = (v + int(rng.integers(1, 4))) % n
            if w != v:
                pairs.add((min(v, w), max(v, w)))
    if not pairs:
        pairs.add((0, 1))
    edges = [(label[a], label[b], _weight(rng, family)) if rng.random() < 0.5 else (label[b], label[a], _weight(rng, family))
             for a, b in sorted(pairs)]
    edges = [edges[int(t)] for t in rng.permutation(len(edges))]
    if repeat_edge:
        u, v, x = edges[0]
        edges.append((v, u, x + 1.0))                        # keeps its first position, takes the last weight
    return edges
