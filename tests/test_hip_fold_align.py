"""GPU tests of FoldAlignment() and its two device entries (sq_align_pair_count, sq_first_fit_dev): the alignment results that stay
on the device, against the reference's Step lines (tests/golden/text/*.txt), the CPU-built result under the OracleEngine,
Predict(alignment=True) of the same build, a plain dict count, align.Consensus and sq_align_first_fit.
All comparisons are exact."""
import ctypes
import io
import random

import numpy as np
import pytest

from tests.fold_align_checks import CASES, SMALL, check_against_golden, check_consensus_at, check_equal, check_table

pytestmark = pytest.mark.gpu

LIMITS = (0, 0.2, 0.35, 0.5, 1)


def _is_device(res):
    import torch
    L = res.L
    shapes = dict(steps=((3, L), torch.int32), stem_matrix=((L, L), torch.float64), metrics=((3, 6), torch.float64),
                  react_scores=((3,), torch.float64))
    for key, (shape, dtype) in shapes.items():
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape, key
    P = int(res.pair_count.numel())
    for key, shape in (("pair_cols", (P, 2)), ("pair_count", (P,)), ("pair_first", (P,))):
        t = getattr(res, key)
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == shape, key
    assert res.source == "device" and res.device.type == "cuda"
    if res.rows is not None:
        assert res.rows.partner.is_cuda and res.rows.source == "device" and P > 0
        assert len(res.first_fit_rounds) == 3
    else:
        assert P == 0 and len(res.first_fit_rounds) == 2
    assert all(0 <= r <= L // 2 + 1 for r in res.first_fit_rounds)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_goldens_stay_on_the_device(tag):
    from squarna_amd import FoldAlignment
    path, kw = CASES[tag]
    res = FoldAlignment(inputfile=path, **kw)
    _is_device(res)
    check_against_golden(res, tag)
    if res.rows is not None:
        check_table(res)
        check_consensus_at(res)
        host = res.cpu()
        assert host.device.type == "cpu" and host.rows.partner.device.type == "cpu"
        assert host.steps.tolist() == res.steps.tolist() and host.consensus_at(0.2) == res.consensus_at(0.2)


@pytest.mark.parametrize("tag", SMALL)
def test_equals_the_cpu_built_result(tag):
    from squarna_amd import FoldAlignment, engine as E
    from tests.oracle_engine import OracleEngine
    path, kw = CASES[tag]
    res = FoldAlignment(inputfile=path, **kw)
    with E.use_engine(OracleEngine()):
        exp = FoldAlignment(inputfile=path, **kw)
    assert exp.source == "host"
    check_equal(res, exp)


def _variant(rows, cols, seed, tmp_path):
    """An alignment in test_hip_parity6's style with a separator column and a column that is a gap in every row."""
    from tests.test_hip_parity6 import _msa_text
    lines = _msa_text(rows, cols - 2, seed).split("\n")
    out = []
    for ln in lines:
        if ln and not ln.startswith(">"):
            mid = len(ln) // 2
            ln = ln[:100] + "-" + ln[100:mid] + "&" + ln[mid:]
        out.append(ln)
    path = tmp_path / ("ali_%d_%d.afa" % (rows, cols))
    path.write_text("\n".join(out))
    return str(path)


@pytest.mark.parametrize("rows,cols", [(40, 700), (1, 333)])
def test_synthetic_alignment_equals_predict(rows, cols, tmp_path):
    """40 x 700 (and a single row): separators, an all-gap column, L not a multiple of 64 -- the three lines of
    Predict(alignment=True) from the same build, for each step3."""
    from squarna_amd import FoldAlignment, Predict
    assert cols % 64
    path = _variant(rows, cols, 77 + rows, tmp_path)
    for step3 in ("u", "i", "1", "2"):
        res = FoldAlignment(inputfile=path, step3=step3)
        _is_device(res)
        assert len(res) == rows and res.L == cols and all("&" in s for s in res.sequences)
        assert all(s[100] == "-" for s in res.sequences)
        buf = io.StringIO()
        Predict(inputfile=path, alignment=True, step3=step3, write_to=buf)
        lines = buf.getvalue().rstrip("\n").split("\n")[-3:]
        assert [res.dbn(k) for k in (1, 2, 3)] == [ln.split("\t")[0] for ln in lines], step3
        assert "Step-3(%s)" % step3 in lines[2]
        if res.rows is not None:
            check_table(res)
            assert res.steps[:, 100].tolist() == [-1] * 3 and not (res.steps == 100).any()
            if rows > 1:
                assert "(" in res.dbn(1) and "(" in res.dbn(2)


# ---- the two entries directly --------------------------------------------------------------------------------------------
def _random_rows(rng, nrow, L):
    """Per row (alignment-column pairs, gap columns): a base pair set kept with probability 0.7 per row plus random extras."""
    base, free = [], list(range(L))
    rng.shuffle(free)
    while len(free) >= 2 and len(base) < L // 3:
        v, w = sorted((free.pop(), free.pop()))
        base.append((v, w))
    rows = []
    for _ in range(nrow):
        gaps = {c for c in range(L) if rng.random() < 0.08}
        used, pairs = set(gaps), []
        for v, w in base:
            if rng.random() < 0.7 and v not in used and w not in used:
                pairs.append((v, w))
                used |= {v, w}
        for _ in range(rng.randint(0, max(1, L // 15))):
            v, w = sorted(rng.sample(range(L), 2))
            if v not in used and w not in used:
                pairs.append((v, w))
                used |= {v, w}
        rows.append((sorted(pairs), gaps))
    return rows


def _tables(rows, L, rng):
    """The pair tables of such rows in sq_result_pairs_dev's layout (gap-free coordinates; a few structure rows of other
    content behind every consensus row) and the gap maps."""
    partner, cell_off, gap_maps = [], [0], []
    for pairs, gaps in rows:
        cols = np.array([c for c in range(L) if c not in gaps], np.int32)
        short = {int(c): k for k, c in enumerate(cols)}
        row = np.full(len(cols), -1, np.int32)
        for v, w in pairs:
            row[short[v]], row[short[w]] = short[w], short[v]
        partner.append(row)
        extra = rng.randint(0, 2)
        for _ in range(extra):
            partner.append(np.roll(row, 1))                               # (never read: only row 0 counts)
        cell_off.append(cell_off[-1] + (1 + extra) * len(cols))
        gap_maps.append(cols)
    return np.concatenate(partner), np.array(cell_off, np.int64), gap_maps


def _sequential(cols, n):
    seen, res = set(), []
    for v, w in cols[:n]:
        if v not in seen and w not in seen:
            seen |= {v, w}
            res.append((v, w))
    return res


def test_count_order_and_first_fit_against_dict_and_consensus():
    import torch
    from squarna_amd import align
    from squarna_amd.dbn import DBNToPairs, PairsToDBN
    from squarna_amd.engine import HipEngine
    from squarna_amd.fold_align import _consensus_order
    eng, rng = HipEngine(), random.Random(2718)
    shapes = [(2, 30), (120, 600), (3, 64), (17, 257)] + [(rng.randint(2, 120), rng.randint(30, 600)) for _ in range(20)]
    ties_matter, most_rounds = 0, 0
    for nrow, L in shapes:
        rows = _random_rows(rng, nrow, L)
        partner, cell_off, gap_maps = _tables(rows, L, rng)
        flat, count, first = eng.align_pair_count(torch.from_numpy(partner).cuda(), torch.from_numpy(cell_off).cuda(), gap_maps, L)
        bps = {}
        for r, (pairs, _) in enumerate(rows):
            for bp in pairs:
                c, f = bps.get(bp, (0, r))
                bps[bp] = (c + 1, f)
        got = {(int(f) // L, int(f) % L): (int(c), int(r)) for f, c, r in zip(flat.tolist(), count.tolist(), first.tolist())}
        assert got == bps and int(flat.numel()) == len(bps), (nrow, L)
        order = _consensus_order(torch, flat, count, first, nrow)
        ranked = [(int(f) // L, int(f) % L) for f in flat[order].tolist()]
        assert ranked == sorted(bps, key=lambda bp: bps[bp][0], reverse=True), (nrow, L)      # (stable over the insertion order)
        structs = [PairsToDBN(pairs, L) for pairs, _ in rows]
        assert all(DBNToPairs(s) == pairs for s, (pairs, _) in zip(structs, rows))
        counts = count[order]
        by_cell_only = sorted(bps, key=lambda bp: (-bps[bp][0], bp))
        for lim in LIMITS:
            n = int((counts.double() >= lim * nrow).sum())
            part, info = eng.first_fit(flat[order][:n].contiguous(), L, 0)
            status, rounds, npairs, live = info.tolist()
            assert status == 0 and live == 0 and rounds <= L // 2 + 1
            most_rounds = max(most_rounds, rounds)
            row = part.cpu().numpy()
            v = np.flatnonzero(row > np.arange(L))
            pairs = list(zip(v.tolist(), row[v].tolist()))
            assert len(pairs) == npairs and all(row[w] == x for x, w in pairs)
            assert pairs == sorted(_sequential(ranked, n))
            exp = align.Consensus(structs, lim)
            assert PairsToDBN(list(set(pairs)), L) == exp, (nrow, L, lim)
            if nrow * L >= 4096:
                assert align._consensus_bulk(structs, lim) == exp
            ties_matter += sorted(_sequential(by_cell_only, n)) != pairs
    # the first-row order is what these cases test: ties ordered by (v, w) alone give another consensus
    assert ties_matter >= 1, "no case in which the order of equal counts matters"
    assert most_rounds >= 2


def test_matrix_cell_order_and_first_fit_against_the_host_pass():
    """Step 1's order (value descending, flat index ascending) and the first fit with minspan 4 against the host's sort and
    sq_align_first_fit, on cells with many equal values."""
    import torch
    from squarna_amd import _lib
    from squarna_amd.engine import HipEngine
    from squarna_amd.fold_align import _rank_cells
    eng, rng = HipEngine(), random.Random(31415)
    for L in (30, 64, 257, 600):
        for n in (0, 1, L, 8 * L):
            cells = rng.sample(range(L * L), n)
            idx = np.array(cells, np.int64)
            val = np.array([rng.choice((4.5, 5.0, 6.5, 9.0, 9.0, 13.0)) for _ in cells], np.float64)
            flat = _rank_cells(torch, torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda())
            sidx = np.ascontiguousarray(idx[np.lexsort((idx, -val))])
            assert flat.cpu().numpy().tolist() == sidx.tolist()
            out = np.empty(2 * (L // 2 + 1), np.int32)
            k = int(_lib.load().sq_align_first_fit(ctypes.c_void_p(sidx.ctypes.data), ctypes.c_int64(len(sidx)), L, 4,
                                                   ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(len(out) // 2)))
            exp = np.full(L, -1, np.int32)
            for v, w in out[:2 * k].reshape(-1, 2).tolist():
                exp[v], exp[w] = w, v
            part, info = eng.first_fit(flat, L, 4)
            assert part.cpu().numpy().tolist() == exp.tolist(), (L, n)
            status, rounds, npairs, live = info.tolist()
            assert (status, live, npairs) == (0, 0, k) and rounds <= L // 2 + 1


def test_chain_takes_one_launch():
    """(0,10), (10,20), ...: about one round per accepted pair, all inside the one launch."""
    import torch
    from squarna_amd.engine import HipEngine
    L = 5000
    flat = torch.tensor([v * L + v + 10 for v in range(0, L - 10, 10)], dtype=torch.int64).cuda()
    part, info = HipEngine().first_fit(flat, L, 4)
    status, rounds, npairs, live = info.tolist()
    assert (status, live) == (0, 0) and npairs == (int(flat.numel()) + 1) // 2 and npairs - 1 <= rounds <= L // 2 + 1
    row = part.cpu().tolist()
    assert all(row[v] == v + 10 and row[v + 10] == v for v in range(0, L - 10, 20))


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch
    from squarna_amd import _lib
    L = _lib.load()
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert L.sq_first_fit_dev(p, 4, 8, 0, p, p, 8, p, None) == -1          # scratch too small
    assert b"scratch" in L.sq_last_error()
    assert L.sq_first_fit_dev(p, -1, 8, 0, p, p, 1 << 20, p, None) == -1
    assert L.sq_align_pair_count(p, p, p, p, 1, 4, 0, p, 1 << 20, p, p, p, 4, p, None) == -1   # threshold below 1
    assert L.sq_align_pair_count(p, p, p, p, 1, 4, 1, p, 8, p, p, p, 4, p, None) == -1         # scratch too small
    torch.cuda.synchronize()
    assert buf.tolist() == [0] * 64


# ---- the emission stage's flush inside the loop (sq_emit.h) ------------------------------------------------------------
# The alignments above select far fewer than 768 cells per block; these inputs are dense enough that blocks flush their stage
# inside the loop, carry a partly filled stage from one row into the next, and outgrow the first call's buffers.
def _check_matrix_select(m, thr, minspan=4):
    """HipEngine.matrix_select of the numpy matrix m against numpy's own selection; returns the expected mask."""
    import torch
    from squarna_amd.engine import HipEngine
    L = m.shape[0]
    v, w = np.indices((L, L))
    mask = (w - v >= minspan) & (m >= thr)
    exp = np.flatnonzero(mask.reshape(-1))
    idx, val = HipEngine().matrix_select(torch.from_numpy(m).cuda(), thr, minspan)
    assert idx.dtype == torch.int64 and val.dtype == torch.float64 and idx.is_cuda and val.is_cuda
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert len(idx) == len(val) == len(exp)
    assert len(np.unique(idx)) == len(idx)                                   # no cell twice
    assert np.array_equal(np.sort(idx), exp)
    assert np.array_equal(val, m.reshape(-1)[idx])                           # bit for bit
    assert (val == thr).any()                                                # (>=, not >)
    return mask


def test_matrix_select_partial_ballots_flush_inside_the_loop():
    """L = 1100, one row per block, values 0..7: at threshold 4 about half of the upper cells pass (partial ballots in every
    wave; row 0 stages ~550, so its block flushes once, at the end); at threshold 2 three quarters pass and the first rows
    stage more than 768, so their blocks flush inside the loop as well."""
    L = 1100
    m = np.random.default_rng(1100).integers(0, 8, (L, L)).astype(np.float64)
    half = _check_matrix_select(m, 4.0)
    assert 0.45 < half.sum() / (np.arange(1, L - 3).sum()) < 0.55
    dense = _check_matrix_select(m, 2.0)
    assert dense[0].sum() > 768 and 0 < dense[0, -256:].sum() < 256


def test_matrix_select_every_cell_two_rows_per_block_and_the_repeat():
    """L = 2304, every cell at or above the threshold: 2,048 blocks, so blocks 0..255 take two rows and carry a partly
    filled stage from one into the next; 2,646,150 cells, so the first call's 65,536 entries are too few and the call is
    repeated with the true number."""
    L = 2304
    m = np.random.default_rng(2304).integers(4, 12, (L, L)).astype(np.float64)
    mask = _check_matrix_select(m, 4.0)
    assert mask.sum() == 2646150 > 1 << 16 and (L - 4) % 1024 and L > 2048


def _antidiagonal_records(L, recs):
    """Gap-free records of one table row each: record of `recs` entry r pairs i with (L - 1 - r) - i for i below its
    partner.  Returns (partner, cell_off, gap_maps, flat cells per record)."""
    partner = np.full((len(recs), L), -1, np.int32)
    cells = []
    for k, r in enumerate(recs):
        s = L - 1 - r
        i = np.arange((s + 1) // 2)
        partner[k, i], partner[k, s - i] = s - i, i
        cells.append(i.astype(np.int64) * L + (s - i))
    return partner.reshape(-1), np.arange(len(recs) + 1, dtype=np.int64) * L, [np.arange(L, dtype=np.int32)] * len(recs), cells


def _check_pair_count(L, recs, threshold):
    """HipEngine.align_pair_count of such records against numpy's count; returns (flat, count, first) as expected."""
    import torch
    from squarna_amd.engine import HipEngine
    partner, cell_off, gap_maps, cells = _antidiagonal_records(L, recs)
    every = np.concatenate(cells)
    owner = np.repeat(np.arange(len(recs)), [len(c) for c in cells])
    flat, at, count = np.unique(every, return_index=True, return_counts=True)     # (at: the first occurrence, records in order)
    keep = count >= threshold
    exp = (flat[keep], count[keep], owner[at][keep])
    rows = np.bincount(exp[0] // L, minlength=L)
    got = HipEngine().align_pair_count(torch.from_numpy(partner).cuda(), torch.from_numpy(cell_off).cuda(), gap_maps, L, threshold)
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32] and all(t.is_cuda for t in got)
    f, c, r = (t.cpu().numpy() for t in got)
    order = np.argsort(f, kind="stable")
    assert len(f) == len(exp[0]) and len(np.unique(f)) == len(f)
    assert np.array_equal(f[order], exp[0]) and np.array_equal(c[order], exp[1]) and np.array_equal(r[order], exp[2])
    return exp, rows


def test_pair_count_dense_rows_flush_inside_the_loop():
    """L = 2000, 900 records: 697,500 distinct column pairs, each held once; rows 0, 1 and 2 of the count table hold 900
    cells each, so their blocks flush inside the loop."""
    L = 2000
    _, _, _, cells = _antidiagonal_records(L, range(900))
    every = np.concatenate(cells)
    assert len(np.unique(every)) == len(every) == 697500                       # no pair is held twice
    assert (np.bincount(every // L)[:3] == 900).all() and 900 > 768            # rows beyond the in-loop bound
    (flat, count, first), rows = _check_pair_count(L, list(range(900)), 1)
    assert len(flat) == 697500 and (count == 1).all() and rows.max() == 900
    assert np.array_equal(first, L - 1 - (flat // L + flat % L))               # (the record whose antidiagonal holds the cell)


def test_pair_count_threshold_two_keeps_the_doubled_records():
    """The same records with every even one given twice, threshold 2: only their pairs, count 2, first = the first copy."""
    L = 2000
    recs = [r for q in range(900) for r in ([q, q] if q % 2 == 0 else [q])]
    first_copy = {r: recs.index(r) for r in range(0, 900, 2)}
    (flat, count, first), _ = _check_pair_count(L, recs, 2)
    assert len(flat) == sum((L - r) // 2 for r in range(0, 900, 2)) and (count == 2).all()
    r = L - 1 - (flat // L + flat % L)
    assert (r % 2 == 0).all() and np.array_equal(first, np.array([first_copy[int(x)] for x in r]))
