"""Shared checks of the Fold() tests (CPU: tests/test_fold_api.py, GPU: tests/test_hip_fold_api.py): a FoldResult against
an engine's SQRNdbnseq tuples and against the structure lines of the reference's output text (tests/golden/text/*.txt).
Every comparison is exact: integers, and doubles bit for bit."""
import math
import os
import struct

from squarna_amd.dbn import DBNToPairs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA = os.path.join(os.path.dirname(GOLDEN), "..", "squarna_amd", "data")


def bits(x):
    """A double's bit pattern (NaN compares equal to NaN of the same bits)."""
    return struct.pack("<d", float(x))


def same_doubles(a, b):
    return len(a) == len(b) and all(bits(x) == bits(y) for x, y in zip(a, b))


def check_against_tuples(res, tuples, keep=None, ref_scores=None):
    """res: a FoldResult (any device); tuples: per record what SQRNdbnseq returns; keep: structures kept per record."""
    res = res.cpu()
    assert len(res) == len(tuples)
    nstruct, row_off, cell_off, lengths = (t.tolist() for t in (res.nstruct, res.row_off, res.cell_off, res.lengths))
    assert row_off[0] == 0 and cell_off[0] == 0
    for r, (cons, preds, cm, bm) in enumerate(tuples):
        if keep is not None:
            preds = preds[:keep]
        seq = res.sequences[r]
        assert lengths[r] == len(seq) == len(cons)
        assert nstruct[r] == len(preds), (r, nstruct[r], len(preds))
        assert row_off[r + 1] - row_off[r] == nstruct[r] and cell_off[r + 1] - cell_off[r] == (1 + nstruct[r]) * len(seq)
        assert res.consensus(r) == cons, (r, res.consensus(r), cons)
        row0 = res.partner[cell_off[r]:cell_off[r] + len(seq)].tolist()
        assert sorted((i, j) for i, j in enumerate(row0) if j > i) == DBNToPairs(cons)
        assert all(j == -1 or row0[j] == i for i, j in enumerate(row0))
        for k, (dbn, sc, ids) in enumerate(preds):
            assert res.pairs(r, k) == DBNToPairs(dbn), (r, k)
            assert res.dbn(r, k) == dbn, (r, k, res.dbn(r, k), dbn)
            assert same_doubles(res.scores[row_off[r] + k].tolist(), sc), (r, k, res.scores[row_off[r] + k].tolist(), sc)
            assert int(res.pset_mask[row_off[r] + k]) & (2 ** 64 - 1) == sum(1 << p for p in ids), (r, k)
            assert res.paramsets(r, k) == [res.paramset_names[r][p] for p in ids]
        met = res.metrics[r].tolist()
        if any(isinstance(x, float) and math.isnan(x) for x in cm):      # no known structure
            assert all(math.isnan(x) for x in met), (r, met)
        else:
            assert same_doubles(met[:6], cm) and same_doubles(met[6:13], bm), (r, met, cm, bm)
            if ref_scores is not None and ref_scores[r] is not None:
                assert same_doubles(met[13:16], ref_scores[r]), (r, met[13:], ref_scores[r])


def golden_blocks(tag):
    """[(name, sequence, consensus, [(dbn, (total, struct, react), [paramset names])])] of a golden text."""
    with open(os.path.join(GOLDEN, "text", tag + ".txt")) as f:
        lines = f.read().split("\n")
    blocks, k = [], 0
    while k < len(lines) and lines[k]:
        assert lines[k].startswith(">"), lines[k]
        name, seq = lines[k], lines[k + 1].split("\t")[0]
        k += 2
        while lines[k] != "_" * len(seq):                               # reactivities / restraints / reference lines
            k += 1
        cons = lines[k + 1].split("\t")[0]
        assert lines[k + 2] == "=" * len(seq)
        k += 3
        structs = []
        while k < len(lines) and lines[k] and not lines[k].startswith(">"):
            f = lines[k].split("\t")
            assert f[1] == "#%d" % (len(structs) + 1)
            structs.append((f[0], tuple(float(x) for x in f[2:5]), f[5].split(",")))
            k += 1
        blocks.append((name, seq, cons, structs))
    return blocks


def check_against_golden(res, tag):
    """The structure lines the reference printed (outplim of them per record) against the FoldResult."""
    res = res.cpu()
    blocks = golden_blocks(tag)
    assert len(blocks) == len(res)
    row_off = res.row_off.tolist()
    for r, (name, seq, cons, structs) in enumerate(blocks):
        assert res.names[r] == name and res.sequences[r] == seq
        assert res.consensus(r) == cons
        assert int(res.nstruct[r]) == len(structs), (r, int(res.nstruct[r]), len(structs))
        for k, (dbn, sc, names) in enumerate(structs):
            assert res.dbn(r, k) == dbn, (r, k)
            assert same_doubles(res.scores[row_off[r] + k].tolist(), sc), (r, k, res.scores[row_off[r] + k].tolist(), sc)
            assert res.paramsets(r, k) == names, (r, k)


def check_dense_forms(res):
    """to_padded / contact_map against pairs()."""
    import torch
    host = res.cpu()
    pad = res.to_padded()
    R, K, Lmax = pad.shape
    assert pad.device == res.partner.device and pad.dtype == torch.int32
    assert R == len(res) and K == int(host.nstruct.max()) and Lmax == int(host.lengths.max())
    pad = pad.cpu()
    for r in range(R):
        n = int(host.lengths[r])
        for k in range(K):
            row = pad[r, k].tolist()
            if k >= int(host.nstruct[r]):
                assert all(v == -1 for v in row)
                continue
            assert all(v == -1 for v in row[n:])
            assert sorted((i, j) for i, j in enumerate(row[:n]) if j > i) == host.pairs(r, k)
    two = res.to_padded(2).cpu()
    assert tuple(two.shape) == (R, 2, Lmax) and torch.equal(two[:, :min(2, K)], pad[:, :min(2, K)])
    for r in range(min(R, 4)):
        for k in range(int(host.nstruct[r])):
            cm = res.contact_map(r, k)
            assert cm.dtype == torch.bool and cm.device == res.partner.device
            idx = cm.cpu().nonzero().tolist()
            prs = host.pairs(r, k)
            assert sorted(map(tuple, idx)) == sorted(prs + [(j, i) for i, j in prs])
