"""Checks shared by the CPU and GPU tests of Entropy() (tests/test_entropy_api.py, tests/test_hip_entropy.py): the reference's
entropy mode row by row from the oracle's own building blocks, the `entropy:` values of the golden texts, and a CPU engine
whose entropy_tensors answers with them.  Not a test module."""
import contextlib
import io
import os

import numpy as np

from oracle import sqrn_oracle as O
from tests.oracle_engine import OracleEngine

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_TEXT = os.path.join(HERE, "golden", "text")
DATA = os.path.join(os.path.dirname(HERE), "squarna_amd", "data")
SEQ_INPUT = os.path.join(DATA, "examples", "seq_input.fas")
ALI_INPUT = os.path.join(DATA, "examples", "ali_input.afa")

#: absolute tolerance on every H_i and on the mean: a term |p log2 p| <= 0.531, log2 and the division a few ulp each, a sum of
#: n <= 32,768 terms in any order at most n eps H -- below 4e-11 together at the largest n
TOL = 1e-9


def reference_rows(seq, reacts, restraints, paramset, stem_matrix=None, interchainonly=False, M=1.8, B=-0.6):
    """(H per gap-free position, mean) of one record: the reference's entropy mode (SQRNdbnseq.py:1001-1037, 1076-1089,
    520-545) from the oracle's UnAlign / ParseRestraints / BPMatrix / AnnotateStems and the reference's formula in numpy,
    without the final rounding."""
    seq = seq.upper().replace("T", "U")
    restraints = restraints or "." * len(seq)
    if not reacts:
        reacts = [0.5] * len(seq)
    if isinstance(reacts, str):
        reacts = O.ProcessReacts([O.ReactDict[ch] for ch in reacts])
    shortseq, shortrest = O.UnAlign(seq, restraints)
    keep = [i for i in range(len(seq)) if seq[i] not in O.GAPS]
    shortreacts = [reacts[i] for i in keep]
    rbps, rxs, rl, rr = O.ParseRestraints(shortrest)
    n = len(shortseq)
    if n == 0:
        return np.zeros(0), float("nan")
    b, s = O.BPMatrix(shortseq, paramset["bpweights"], rxs, rl, rr, interchainonly, reacts=shortreacts,
                      bpp_power=paramset["bpp"], M=M, B=B)
    if stem_matrix is not None:
        s = s * np.asarray(stem_matrix, np.float64)[np.ix_(keep, keep)]
    sm = np.zeros((n, n))
    for st in O.AnnotateStems(b, s, rbps, [], paramset["minlen"], paramset["minbpscore"]):
        for v, w in O.stem_bps(st):
            sm[v, w] = sm[w, v] = st[3]
    H = np.zeros(n)
    for i in range(n):
        row = sm[i, :]
        if row.sum():
            probs = np.array([p for p in row / row.sum() if p])
            H[i] = sum(-(probs * np.log2(probs)))
    ent = 0
    for h in H:                                                      # (the reference's running sum, in position order)
        ent += h
    return H, ent / n


def golden_entropies(tag):
    """The value on every `entropy:` line of a golden text, in order, as the strings the reference printed."""
    with open(os.path.join(GOLDEN_TEXT, tag + ".txt")) as f:
        return [line.rstrip("\n").split("\t")[2] for line in f if "\tentropy:\t" in line]


def parsed(path):
    """The (name, sequence, reactivities, restraints, reference) records of an input file."""
    from squarna_amd.inputs import ParseInput
    with contextlib.redirect_stdout(io.StringIO()):
        return list(ParseInput(None, path, "qtrf")[0])


def paramset0(config):
    from squarna_amd.config import ParseConfig, builtin_config
    return ParseConfig(builtin_config(config))[1][0]


_memo = {}


def seq_input_reference():
    """[(H, mean)] of examples/seq_input.fas under alt's first paramset; computed once, left unchanged."""
    if "seq" not in _memo:
        ps = paramset0("alt")
        _memo["seq"] = [reference_rows(rec[1], rec[2], rec[3], ps) for rec in parsed(SEQ_INPUT)]
    return _memo["seq"]


def ali_stem_matrix():
    """The normalised step-1 matrix of examples/ali_input.afa: FoldAlignment's under the CPU engine (numpy, L x L)."""
    if "smat" not in _memo:
        from squarna_amd import FoldAlignment
        from squarna_amd import engine as E
        with E.use_engine(OracleEngine()):
            _memo["smat"] = FoldAlignment(inputfile=ALI_INPUT).stem_matrix.numpy().copy()
    return _memo["smat"]


def ali_input_reference(stem_matrix=None):
    """[(H, mean)] of the rows of examples/ali_input.afa under ali's first paramset, weighted by the stem matrix."""
    key = "ali" if stem_matrix is None else None
    if key and key in _memo:
        return _memo[key]
    ps = paramset0("ali")
    sm = ali_stem_matrix() if stem_matrix is None else stem_matrix
    out = [reference_rows(rec[1], rec[2], rec[3], ps, stem_matrix=sm) for rec in parsed(ALI_INPUT)]
    if key:
        _memo[key] = out
    return out


class EntropyOracleEngine(OracleEngine):
    """The CPU test engine with entropy_tensors: reference_rows per record, CPU tensors in the engine contract's layout."""

    def entropy_tensors(self, recs, interchainonly=False, M=1.8, B=-0.6, stem_matrix=None, bpp=None, scratch_bytes=None):
        import torch
        rows = [reference_rows(seq, reacts, restraints, ps, stem_matrix=stem_matrix, interchainonly=interchainonly, M=M, B=B)
                for seq, reacts, restraints, ps in recs]
        lengths = np.array([len(H) for H, _ in rows], np.int64)
        pos_off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(lengths, out=pos_off[1:])
        return dict(position=torch.from_numpy(np.concatenate([H for H, _ in rows] + [np.zeros(0)])), pos_off=torch.from_numpy(pos_off),
                    mean=torch.tensor([m for _, m in rows], dtype=torch.float64),
                    nstems=torch.tensor([-1] * len(rows), dtype=torch.int32), lengths=lengths)


def check_layout(res, seqs):
    """pos_off / lengths / to_padded agree; NaN exactly at the gap columns, 0.0 at the separators; mean = nan-sum / N."""
    host = res.cpu()
    lens = [len(s) for s in seqs]
    assert host.sequences == list(seqs) and len(res) == len(seqs)
    assert host.lengths.tolist() == lens and host.pos_off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert host.position.numel() == sum(lens)
    padded = host.to_padded().numpy()
    assert padded.shape == (len(seqs), max(lens))
    for r, sq in enumerate(seqs):
        row = host.row(r).numpy()
        assert np.array_equal(row, padded[r, :len(sq)], equal_nan=True) and np.isnan(padded[r, len(sq):]).all()
        gaps = np.array([ch in "-.~" for ch in sq], bool)
        assert np.array_equal(np.isnan(row), gaps), (r, sq)
        assert all(row[c] == 0.0 for c, ch in enumerate(sq) if ch in ";&"), (r, sq)
        n = int((~gaps).sum())
        if n:
            assert abs(float(host.mean[r]) - np.nansum(row) / n) <= 1e-12, r
        else:
            assert np.isnan(float(host.mean[r]))


def check_close(res, seqs, reference, tol=TOL):
    """position and mean of every record within tol of reference_rows' (H, mean)."""
    host = res.cpu()
    for r, (sq, (H, mean)) in enumerate(zip(seqs, reference)):
        keep = np.array([ch not in "-.~" for ch in sq], bool)
        got = host.row(r).numpy()[keep]
        assert got.shape == H.shape, r
        if len(H):
            assert float(np.abs(got - H).max()) <= tol, (r, float(np.abs(got - H).max()))
            assert abs(float(host.mean[r]) - mean) <= tol, (r, float(host.mean[r]), mean)
        else:
            assert np.isnan(float(host.mean[r]))
