"""Checks shared by the CPU and GPU tests of the graph-level matching entries (tests/test_matching_reference.py,
tests/test_hip_matching_many.py, tests/test_hip_matching_forms.py): ctypes wrappers that hand sq_lsap / sq_nussinov / sq_mwm SEVERAL problems per call (the
drop-ins of squarna_amd/core.py always pass one), the references they are judged by -- scipy's linear_sum_assignment on the
dense matrix, a plain fp64 Nussinov DP, the oracle's Nussinov, networkx's max_weight_matching -- and seeded generators of
adversarial inputs: arbitrary sparse cells, weights from small sets of multiples of 1/8 (every sum exact, ties everywhere),
repeated cells -- and second statements of the launches' decisions (lsap_form, mwm_launch, nussinov_threads), pinned against the
headers on the CPU.  `python -m tests.matching_checks forms NAME` is the child process of the GPU tests of the process-wide
SQ_MWM_* / SQ_NUSS_THREADS switches (FORMS_SCENARIOS).  Not a test module."""
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


# ------------------------------------------------------------------ the storage forms of the blossom kernels
#: sq_blossom_hdr() of csrc/sq_algo_plan.h: sizeof(SqBlossom) rounded up to 16, the algorithm object in front of a wave's LDS slice
MWM_HDR = 912
MWM_EDGE = 16                                                # sizeof(SqMatchEdge)


def mwm_queue_cap(n, m, tight):
    """SqBlossom::queue_cap, and queue_hot_cap under tight = 2 (csrc/sq_blossom.h)."""
    return 4 * n + 16 if tight == 2 else 4 * n + m + 16 if tight else 8 * n + 2 * m + 16


def mwm_pool_capacity(n, m, tight):
    return 4 * n + m + 256 if tight else n * 32 + 2 * m + 1024


def mwm_frame_ints(n, tight):
    return 8 * (n // 2 + 4) if tight else 10 * (2 * n + 2)


def mwm_hot_bytes(n, m, tight):
    """SqBlossom::hot_bytes: what every scan pass touches -- dualvar, bslack | adj_off, inblossom, bestedge, labeledge, queue |
    label, allow."""
    n2 = 2 * n + 2
    return (n + n2) * 8 + (n + 1 + n + 2 * n2 + mwm_queue_cap(n, m, tight)) * 4 + n2 + m + 64


def mwm_cold_bytes(n, m, tight):
    """SqBlossom::cold_bytes: the blossom structure, the pool, the temporaries and the frames, + bdual."""
    n2 = 2 * n + 2
    ints = 3 * n + 2 * n2 + 8 * n2 + mwm_pool_capacity(n, m, tight) + 2 * n + 2 + 8 * n2 + mwm_frame_ints(n, tight)
    return ints * 4 + n2 * 8 + 64


def mwm_edge_bytes(m):
    return 2 * m * 16 + 64


def mwm_scratch_bytes(n, m, tight=0):
    return mwm_hot_bytes(n, m, tight) + mwm_cold_bytes(n, m, tight) + mwm_edge_bytes(m) + 64


def mwm_crowd(dims, inflight=1):
    """sq_mwm_crowd of csrc/sq_algo_plan.h on [(n, m), ...]."""
    hot_max = max([mwm_hot_bytes(n, m, 2) for n, m in dims] + [0])
    return len(dims) * max(1, inflight) >= 1024 or (len(dims) >= 768 and hot_max + 16 + MWM_HDR > 40 * 1024)


def nussinov_threads(dims, inflight=1, nuss_threads=0):
    """sq_nussinov_threads: the block size of a Nussinov launch of [(n, cells), ...]; nuss_threads: SQ_NUSS_THREADS as
    sq_tuning() reads it (rounded down to whole waves, within 64 .. 256)."""
    if nuss_threads:
        return max(64, min(256, nuss_threads // 64 * 64))
    maxn = max([n for n, _ in dims] + [0])
    return 64 if mwm_crowd(dims, inflight) else max(64, min(256, (maxn + 63) // 64 * 64))


def mwm_dims(edges):
    """(vertices, distinct undirected edges) of an edge list: the (n, m) of the job the entry builds from it."""
    return len({x for u, v, _ in edges for x in (u, v)}), len({(min(u, v), max(u, v)) for u, v, _ in edges})


def mwm_launch(graph_dims, inflight=1, bin_waves=0, bin_bytes=0, all_cap=0, nolds=False):
    """What one blossom launch of the graphs [(n, m distinct edges), ...] looks like: sq_mwm_plan's decisions -- `waves` per
    block, `nbins`, the block's dynamic `lds`, `cap`, `all_in_lds`, each graph's `lds_bytes` and `slices` [lds_off, lds_bytes,
    next], `bin_head`, the `bins` as lists of graphs -- and `forms`: the storage form the KERNEL takes for each graph by the
    two tests at the top of sq_mwm_one (1 all state and the edge list in LDS, 2 the hot part alone, 0 everything in global
    memory, None for a graph without vertices).  With waves == 1 (sq_mwm_single_kernel) every graph sees the launch-wide
    lds - MWM_HDR, whatever the plan meant it to take; a wave of a bin (sq_mwm_kernel) sees its own slice less the header.
    bin_waves / bin_bytes / all_cap / nolds: SQ_MWM_BIN_WAVES / SQ_MWM_BIN_BYTES / SQ_MWM_ALL_CAP / SQ_MWM_NOLDS."""
    nj = len(graph_dims)
    many, crowd = inflight >= 3, mwm_crowd(graph_dims, inflight)
    cap = min(bin_bytes if bin_bytes > 0 else 40 * 1024 if crowd else 96 * 1024 if many else 150 * 1024, 150 * 1024)
    all_cap = all_cap if all_cap > 0 else 1 if crowd else 48 * 1024 if many else 150 * 1024
    waves = bin_waves if bin_waves > 0 else 4 if crowd else (nj * max(1, inflight) + 255) // 256
    waves = max(1, min(waves, 8))
    need, all_in_lds = [], True
    for n, m in graph_dims:
        full = mwm_scratch_bytes(n, m, 1) + ((m * MWM_EDGE + 15) & ~15) + 16
        hot = mwm_hot_bytes(n, m, 2) + 16
        take = MWM_HDR
        if n > 0 and not nolds:
            if MWM_HDR + full <= min(all_cap, cap):
                take = MWM_HDR + full
            elif MWM_HDR + hot <= cap:
                take = MWM_HDR + hot
        if n > 0 and take != MWM_HDR + full:
            all_in_lds = False
        need.append((take + 15) & ~15)
    # first fit in decreasing order of need (a stable sort); bins before first_open are full by count
    used, bins, slices, first_open = [], [], [None] * nj, 0
    for q in sorted(range(nj), key=lambda q: -need[q]):
        k = first_open
        while k < len(used) and (len(bins[k]) >= waves or used[k] + need[q] > cap):
            k += 1
        if k == len(used):
            used.append(0)
            bins.append([])
        else:
            slices[bins[k][-1]][2] = q
        slices[q] = [used[k], need[q], -1]
        used[k] += need[q]
        bins[k].append(q)
        while first_open < len(used) and len(bins[first_open]) >= waves:
            first_open += 1
    lds = (max(used + [0]) + 255) & ~255
    forms = []
    for q, (n, m) in enumerate(graph_dims):
        have = max((lds if waves == 1 else need[q]) - MWM_HDR, 0)
        if n <= 0:
            forms.append(None)
        elif mwm_scratch_bytes(n, m, 1) + ((m * MWM_EDGE + 15) & ~15) + 16 <= have:
            forms.append(1)
        else:
            forms.append(2 if mwm_hot_bytes(n, m, 2) + 16 <= have else 0)
    return dict(waves=waves, nbins=len(bins), lds=lds, cap=cap, all_in_lds=all_in_lds, lds_bytes=need, slices=slices,
                bin_head=[b[0] for b in bins], bins=bins, forms=forms)


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


def _shuffled(rng, n, pairs, family, repeat_edge=False):
    """Edges over the index pairs `pairs` as mwm_case writes them: labels 3 v + 7 over a shuffled numbering, either orientation,
    shuffled order, weights of `family`."""
    label = [3 * int(v) + 7 for v in rng.permutation(n)]
    edges = [(label[a], label[b], _weight(rng, family)) if rng.random() < 0.5 else (label[b], label[a], _weight(rng, family))
             for a, b in sorted(pairs)]
    edges = [edges[int(t)] for t in rng.permutation(len(edges))]
    if repeat_edge:
        u, v, x = edges[0]
        edges.append((v, u, x + 1.0))
    return edges


def mwm_sized(seed, n, chords, family=DYADIC[1], hub=0, repeat_edge=False):
    """A graph of EXACTLY n vertices and n - 1 + chords + (hub spokes not yet there) distinct edges: the path 0 - 1 - ... - n-1,
    `chords` further edges -- half of them across 2 or 3 steps of the path (odd cycles), half at random -- and `hub` spokes from
    vertex 0 to the far end of the path."""
    rng = np.random.default_rng(seed)
    pairs = {(v, v + 1) for v in range(n - 1)}
    want = min(n - 1 + chords, n * (n - 1) // 2)
    while len(pairs) < want:
        a = int(rng.integers(n))
        b = a + int(rng.integers(2, 4)) if rng.random() < 0.5 else int(rng.integers(n))
        if a != b and b < n:
            pairs.add((min(a, b), max(a, b)))
    pairs |= {(0, n - 1 - k) for k in range(hub)}
    return _shuffled(rng, n, pairs, family, repeat_edge)


def mwm_star(seed, n, family=DYADIC[2]):
    """One centre and n - 1 leaves."""
    return _shuffled(np.random.default_rng(seed), n, {(0, v) for v in range(1, n)}, family)


def mwm_hub_cycle(seed, n, family=DYADIC[0]):
    """A hub (vertex 0) in front of a long odd cycle over the other vertices (n even: n - 1 of them), tied to every second."""
    L = n - 1
    assert L % 2 == 1 and L >= 5
    pairs = {(v, v + 1) for v in range(1, L)} | {(1, L)} | {(0, v) for v in range(1, L + 1, 2)}
    return _shuffled(np.random.default_rng(seed), n, pairs, family)


#: the classic small cases of the blossom algorithm as edge lists (u, v, weight); what is expected of them is asked of networkx
MWM_CLASSIC = {
    "s_blossom": [(1, 2, 8), (1, 3, 9), (2, 3, 10), (3, 4, 7)],
    "s_blossom_augment": [(1, 2, 8), (1, 3, 9), (2, 3, 10), (3, 4, 7), (1, 6, 5), (4, 5, 6)],
    "s_relabelled_t_a": [(1, 2, 9), (1, 3, 8), (2, 3, 10), (1, 4, 5), (4, 5, 4), (1, 6, 3)],
    "s_relabelled_t_b": [(1, 2, 9), (1, 3, 8), (2, 3, 10), (1, 4, 5), (4, 5, 3), (1, 6, 4)],
    "s_relabelled_t_c": [(1, 2, 9), (1, 3, 8), (2, 3, 10), (1, 4, 5), (4, 5, 3), (3, 6, 4)],
    "nested_s": [(1, 2, 9), (1, 3, 9), (2, 3, 10), (2, 4, 8), (3, 5, 8), (4, 5, 10), (5, 6, 6)],
    "nested_s_relabel": [(1, 2, 10), (1, 7, 10), (2, 3, 12), (3, 4, 20), (3, 5, 20), (4, 5, 25), (5, 6, 10), (6, 7, 10), (7, 8, 8)],
    "nested_s_expand": [(1, 2, 8), (1, 3, 8), (2, 3, 10), (2, 4, 12), (3, 5, 12), (4, 5, 14), (4, 6, 12), (5, 7, 12), (6, 7, 14),
                        (7, 8, 12)],
    "t_expand": [(1, 2, 23), (1, 5, 22), (1, 6, 15), (2, 3, 25), (3, 4, 22), (4, 5, 25), (4, 8, 14), (5, 7, 13)],
    "nested_t_expand": [(1, 2, 19), (1, 3, 20), (1, 8, 8), (2, 3, 25), (2, 4, 18), (3, 5, 18), (4, 5, 13), (4, 7, 7), (5, 6, 7)],
    "nasty_t_expand_1": [(1, 2, 45), (1, 5, 45), (2, 3, 50), (3, 4, 45), (4, 5, 50), (1, 6, 30), (3, 9, 35), (4, 8, 35), (5, 7, 26),
                         (9, 10, 5)],
    "nasty_t_expand_2": [(1, 2, 45), (1, 5, 45), (2, 3, 50), (3, 4, 45), (4, 5, 50), (1, 6, 30), (3, 9, 35), (4, 8, 26), (5, 7, 40),
                         (9, 10, 5)],
    "nasty_t_expand_least_slack": [(1, 2, 45), (1, 5, 45), (2, 3, 50), (3, 4, 45), (4, 5, 50), (1, 6, 30), (3, 9, 35), (4, 8, 28),
                                   (5, 7, 26), (9, 10, 5)],
    "nasty_nested_t_expand": [(1, 2, 45), (1, 7, 45), (2, 3, 50), (3, 4, 45), (4, 5, 95), (4, 6, 94), (5, 6, 94), (6, 7, 50),
                              (1, 8, 30), (3, 11, 35), (5, 9, 36), (7, 10, 26), (11, 12, 5)],
}

#: sizes at the edges of the blossom kernel's loops: the `lane += 64` strides, the 192 entries the dual step keeps in registers
MWM_EDGE_SIZES = (63, 64, 65, 128, 129, 150, 192, 193)
_FAMILIES = DYADIC + (CONTINUOUS,)


def _classic():
    return [[(u, v, float(x)) for u, v, x in edges] for edges in MWM_CLASSIC.values()]


def _edge_sized(seed):
    """One graph of every size of MWM_EDGE_SIZES (weight families in turn, CONTINUOUS among them), a hub of 70 and one of 100
    neighbours, a star, a hub in front of a long odd cycle."""
    out = [mwm_sized(seed + t, n, n // 2 + 7 * t, _FAMILIES[t % 4]) for t, n in enumerate(MWM_EDGE_SIZES)]
    out += [mwm_sized(seed + 20, 140, 60, DYADIC[1], hub=70), mwm_sized(seed + 21, 193, 40, CONTINUOUS, hub=100),
            mwm_star(seed + 22, 130), mwm_hub_cycle(seed + 23, 152), mwm_hub_cycle(seed + 24, 200, DYADIC[1])]
    return out


def _with_empties(graphs, seed):
    """The call as it is sent: its graphs in shuffled order, then graphs without an edge at the head, in the middle and at
    the end, and a repeated edge (the other orientation, another weight) on the first graph that has an edge."""
    rng = np.random.default_rng(seed)
    graphs = [list(graphs[int(t)]) for t in rng.permutation(len(graphs))]
    k = next(g for g, e in enumerate(graphs) if e)
    u, v, x = graphs[k][0]
    graphs[k].append((v, u, x + 1.0))
    graphs[len(graphs) // 2:len(graphs) // 2] = [[], []]
    return [[]] + graphs + [[]]


_sets = {}


def forms_set(name):
    """The graph sets of tests/test_hip_matching_forms.py, built once per process and never changed:
      crowd   1,030 graphs: 2 .. 24 vertices, the classic cases, the sizes at the loops' edges, one sparse graph of 600 vertices
      three   600 graphs of 2 .. 40 vertices
      single  24 graphs of 100 .. 150 vertices and one of 300 vertices with 1,800 edges
      few     40 graphs of 63 .. 200 vertices (one graph per block)
      bins    300 graphs: the classic cases, the sizes at the loops' edges, 2 .. 40 vertices
      mixed   300 graphs of 2 .. 150 vertices"""
    if name in _sets:
        return _sets[name]
    if name == "crowd":
        graphs = [mwm_case(7000 + g, 2 + g % 23) for g in range(1026 - len(MWM_CLASSIC) - 13 - 1)]
        graphs += _classic() + _edge_sized(7100) + [mwm_sized(7200, 600, 1, DYADIC[2])]
        graphs = _with_empties(graphs, 71)
    elif name == "three":
        graphs = _with_empties([mwm_case(7300 + g, 2 + g % 39) for g in range(596)], 73)
    elif name == "single":
        graphs = [mwm_sized(7400 + g, 100 + (g * 13) % 51, 40 + 9 * g, _FAMILIES[g % 4]) for g in range(19)]
        graphs = _with_empties(graphs + [mwm_sized(7450, 300, 1501, DYADIC[2])], 74)
    elif name == "few":
        graphs = _edge_sized(7500) + _edge_sized(7540) + [mwm_sized(7580 + g, 70 + 11 * g, 30 + 20 * g, _FAMILIES[g % 4]) for g in range(10)]
        graphs = _with_empties(graphs, 75)
    elif name == "bins":
        graphs = _classic() + _edge_sized(7600) + [mwm_case(7700 + g, 2 + g % 39) for g in range(296 - len(MWM_CLASSIC) - 13)]
        graphs = _with_empties(graphs, 76)
    elif name == "mixed":
        graphs = [mwm_case(7800 + g, 2 + g % 13) for g in range(186)] + _classic()
        graphs += [mwm_sized(7900 + g, 20 + g, 10 + g % 30, _FAMILIES[g % 4]) for g in range(60)]
        graphs += [mwm_sized(8000 + g, 110 + (g * 7) % 41, 20 + 3 * g, _FAMILIES[g % 4]) for g in range(36)]
        graphs = _with_empties(graphs, 78)
    else:
        raise KeyError(name)
    _sets[name] = graphs
    return graphs


#: SQ_MWM_BIN_BYTES of the `mixed` scenario: a block of 8 KB holds all the state of a graph of up to about 12 vertices and the
#: hot part of one of up to about 100 (test_hip_matching_forms.py asserts the three forms with mwm_launch)
MIXED_BIN_BYTES = 8192

#: name -> (the one switch of the child process, the graph sets of its calls, the same setting for mwm_launch)
FORMS_SCENARIOS = {
    "nolds": ({"SQ_MWM_NOLDS": "1"}, ("few", "bins"), dict(nolds=True)),
    "hot": ({"SQ_MWM_ALL_CAP": "1"}, ("few", "bins"), dict(all_cap=1)),
    "mixed": ({"SQ_MWM_BIN_BYTES": str(MIXED_BIN_BYTES)}, ("mixed",), dict(bin_bytes=MIXED_BIN_BYTES)),
    "waves8": ({"SQ_MWM_BIN_WAVES": "8"}, ("bins",), dict(bin_waves=8)),
    "nuss64": ({"SQ_NUSS_THREADS": "64"}, (), {}),
    "nuss128": ({"SQ_NUSS_THREADS": "128"}, (), {}),
}
FORMS_SWITCHES = ("SQ_MWM_NOLDS", "SQ_MWM_ALL_CAP", "SQ_MWM_BIN_BYTES", "SQ_MWM_BIN_WAVES", "SQ_MWM_CLASSES", "SQ_NUSS_THREADS")


#: the early return (0, 1), the first cell that can exist (5), one wave, one 256-thread block, rows that stride it
NUSS_SIZES = (0, 1, 2, 4, 5, 6, 63, 64, 65, 128, 129, 256, 257, 300)


def nussinov_problem_set():
    """The Nussinov problems of tests/test_hip_matching_many.py: every size of NUSS_SIZES at four densities, four problems
    with separators, in shuffled order."""
    probs = []
    for t, n in enumerate(NUSS_SIZES):
        for d, dens in enumerate((0.0, 0.4, 1.5, 3.0)):
            if n < 5 and d > 1:
                continue                                     # no cell fits: the empty problem once, and once asked for cells
            probs.append(nussinov_case(3000 + 10 * t + d, n, int(dens * n), (DYADIC + (DYADIC[2],))[(t + d) % 4]))
    for t, n in enumerate((6, 65, 129, 257)):                # separators: BackTrack's other branch, cells of span 2 and 3
        probs.append(nussinov_case(3500 + t, n, 2 * n, DYADIC[1], seps=True))
    order = np.random.default_rng(31).permutation(len(probs))
    return [probs[int(t)] for t in order]


def nussinov_crowd_set():
    """1,034 problems for ONE call, where the kernel gets one wave per problem: 1,024 of 5 .. 24 nt, and the lengths at which a
    lane takes a second, third, fourth and fifth cell of an anti-diagonal; separators in some of both."""
    probs = [nussinov_case(8100 + g, 5 + g % 20, (5 + g % 20) * (1 + g % 3), _FAMILIES[g % 3], seps=g % 16 == 5) for g in range(1024)]
    for t, n in enumerate((63, 64, 65, 128, 129, 192, 193, 256, 257, 300)):
        probs.append(nussinov_case(8200 + t, n, 2 * n, DYADIC[1 + t % 2], seps=t in (2, 8)))
    order = np.random.default_rng(81).permutation(len(probs))
    return [probs[int(t)] for t in order]


# ------------------------------------------------------------------ python -m tests.matching_checks forms NAME
def _forms_child(name):
    """One scenario of FORMS_SCENARIOS in a process that was started with its switch (the SQ_MWM_* switches and SQ_NUSS_THREADS are
    read once per process): the pair lists of every call as one JSON line; the parent compares them with its references."""
    import json
    import os
    env, sets, _ = FORMS_SCENARIOS[name]
    assert {k: os.environ.get(k) for k in FORMS_SWITCHES} == {k: env.get(k) for k in FORMS_SWITCHES}, name
    out = {}
    if name.startswith("nuss"):
        out["nussinov"] = nussinov_many(nussinov_problem_set())
    for s in sets:
        lists, poff = mwm_many(forms_set(s))
        out[s] = dict(pairs=lists, poff=poff)
    print("FORMS " + json.dumps(out), flush=True)


if __name__ == "__main__":
    import sys
    assert len(sys.argv) == 3 and sys.argv[1] == "forms", sys.argv
    _forms_child(sys.argv[2])
