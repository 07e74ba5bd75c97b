"""The device pipeline of FoldAlignment() on CPU tensors (no GPU): a stand-in engine offers the device methods -- stem_matrix,
matrix_select, first_fit, fold_tensors in gap-free coordinates, align_pair_count -- with plain numpy / Python behind them and
hands its cells and pairs over in shuffled order, as the kernels do.  What is checked is everything between the kernels: the
two sort orders, the frequency prefix, the gap maps, the move of the rows' tables into alignment coordinates -- against the
result built through the host path and the reference's Step lines."""
import io
import random

import pytest

from squarna_amd import engine as E
from tests.fold_align_checks import CASES, check_against_golden, check_consensus_at, check_equal, check_table
from tests.oracle_engine import OracleEngine


class StandInEngine(OracleEngine):
    name = "stand-in"

    def __init__(self):
        self.rng = random.Random(99)

    def _shuffled(self, n):
        import torch
        order = list(range(n))
        self.rng.shuffle(order)
        return torch.tensor(order, dtype=torch.int64)

    def stem_matrix(self, records, bpweights, minlen, minbpscore, interchainonly=False):
        import torch
        from squarna_amd import align
        objs = [(None, seq, reacts, rests, None) for seq, reacts, rests in records]
        with E.use_engine(OracleEngine()):
            smat = align.SQRNdbnali(objs, None, None, None, bpweights, interchainonly, minlen, minbpscore, sink=io.StringIO())[1]
        return torch.from_numpy(smat)

    def matrix_select(self, matrix, threshold, minspan=4):
        import torch
        L = matrix.shape[0]
        v, w = torch.meshgrid(torch.arange(L), torch.arange(L), indexing="ij")
        hit = ((w - v >= minspan) & (matrix >= threshold)).reshape(-1).nonzero().reshape(-1)
        hit = hit[self._shuffled(int(hit.numel()))]
        return hit, matrix.reshape(-1)[hit]

    def first_fit(self, flat, Lcols, minspan=0):
        import torch
        partner = [-1] * Lcols
        taken = 0
        for f in flat.tolist():
            v, w = divmod(f, Lcols)
            if w > v and w - v >= minspan and partner[v] < 0 and partner[w] < 0:
                partner[v], partner[w] = w, v
                taken += 1
        return torch.tensor(partner, dtype=torch.int32), torch.tensor([0, 1 if taken else 0, taken, 0], dtype=torch.int32)

    def fold_tensors(self, records, **opts):
        from squarna_amd.fold import _oracle_tables
        keep = opts.pop("keep")
        sm = records[0][5].numpy()                                       # (the one shared matrix, a tensor in this path)
        res = self.fold_records([rec[:5] + (sm,) for rec in records], **opts)
        strip = lambda s, seq: "".join(ch for ch, q in zip(s, seq) if q not in "-.~")
        full, seqs = [], []
        for (cons, preds, cm, bm), rec in zip(res, records):
            seq = rec[0]
            short = [(strip(d, seq), sc, ids) for d, sc, ids in preds]
            full.append(((strip(cons, seq), short, cm, bm), strip(seq, seq), None))
            seqs.append(strip(seq, seq))
        tables, nstruct, lengths = _oracle_tables(full, seqs, keep)
        return dict(tables, nstruct=nstruct, lengths=lengths, source="device")

    def align_pair_count(self, partner, cell_off, gap_maps, Lcols, threshold=1):
        import torch
        bps = {}
        for r, cols in enumerate(gap_maps):
            row = partner[int(cell_off[r]):int(cell_off[r]) + len(cols)].tolist()
            for i, j in enumerate(row):
                if j > i:
                    key = int(cols[i]) * Lcols + int(cols[j])
                    c, f = bps.get(key, (0, r))
                    bps[key] = (c + 1, f)
        keys = [k for k in bps if bps[k][0] >= threshold]
        self.rng.shuffle(keys)
        return (torch.tensor(keys, dtype=torch.int64), torch.tensor([bps[k][0] for k in keys], dtype=torch.int32),
                torch.tensor([bps[k][1] for k in keys], dtype=torch.int32))


@pytest.mark.parametrize("tag", sorted(CASES))
def test_device_pipeline_on_cpu_tensors(tag):
    from squarna_amd import FoldAlignment
    path, kw = CASES[tag]
    with E.use_engine(StandInEngine()):
        res = FoldAlignment(inputfile=path, **kw)
        assert res.source == "device" and res.device.type == "cpu"
        assert len(res.first_fit_rounds) == (2 if res.rows is None else 3)
        check_against_golden(res, tag)
        if res.rows is not None:
            check_table(res)
            check_consensus_at(res)
    with E.use_engine(OracleEngine()):
        exp = FoldAlignment(inputfile=path, **kw)
    # (the stand-in's rows carry no known structure: the metrics of the rows are compared on the GPU)
    if res.rows is not None:
        res.rows.metrics = exp.rows.metrics
    check_equal(res, exp)
