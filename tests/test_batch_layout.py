"""The workspace layout of a batch (csrc/sq_batch.hip: plan()), Batch's descriptor and the workspace's size classes, on the CPU.

Every expected number below was recorded from the library built from commit 194bd32 (sq_batch_create as one function, the
workspace sized in plan() and laid out again in the create from a second copy of the arithmetic; the size-class rounding
inside Batch._finish_init) and is kept as a literal: the same descriptors, built through Batch._describe, sent to
sq_batch_workspace_bytes.  The total is a sum, so it pins the size of every region of the workspace, not their order.
Needs the built library (python -m squarna_amd.build), like test_host_layer.test_c_abi_exports_every_declared_symbol; no GPU."""
import os
import random

import numpy as np
import pytest

from squarna_amd import plan as P
from squarna_amd.batch import Batch
from squarna_amd.config import ParseConfig, builtin_config
from squarna_amd.inputs import ParseDefaultInput
from squarna_amd.records import Prepared

ENV = ("SQ_NO_POOL_KEPT", "SQ_KEPT_PPS", "SQ_KEPT_GB", "SQ_CTX_MIN_N", "SQ_MUL_GATHER", "SQ_OUT_CAP", "SQ_FIN_STEM_CAP",
       "SQ_LD_POW2", "SQ_NO_SHARED_BITS")
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "squarna_amd", "data", "datasets")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _psets(config):
    return ParseConfig(builtin_config(config))[1]


def _seq(n, seed, alphabet="ACGU"):
    rng = random.Random(seed)
    return "".join(rng.choice(alphabet) for _ in range(n))


def _random_records(count, n, seed=7):
    return [Prepared(_seq(n, seed + k)) for k in range(count)]


def _srtest150():
    return [Prepared(seq, reacts, restr, ref) for _, seq, reacts, restr, ref in
            ParseDefaultInput(os.path.join(DATA, "SRtest150.fas"), "qf")]


def _described(records, psets_per_record, pool_lists=False, **desc):
    """A Batch up to its descriptor: host arrays, job lists, _describe -- no workspace, no device batch."""
    b = Batch.__new__(Batch)
    nseq = b._host_arrays(records)
    b._pool_lists = pool_lists
    b._job_lists(nseq, psets_per_record if isinstance(psets_per_record[0], list) else [psets_per_record] * nseq)
    b._describe(**desc)
    return b


def _bytes(records, psets, **desc):
    return _described(records, psets, **desc).workspace_bytes()


class _DeviceMatrix:
    """What Batch._describe asks of mul_shared's matrix, at an address nobody reads (the plan compares it with NULL)."""
    is_cuda = True

    def __init__(self, L):
        import torch
        self.dtype, self.shape = torch.float64, (L, L)

    def dim(self):
        return 2

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 0x10000


# ---- workspace bytes ----------------------------------------------------------------------------------------------------

#: (config, fp32, max_structs, cand_per_nt) -> bytes for the 219 records of SRtest150
SRTEST150 = {
    ('alt', False, 0, 0): 848890112,
    ('alt', False, 0, 64): 1478035712,
    ('alt', False, 4096, 0): 848890112,
    ('alt', False, 4096, 64): 1478035712,
    ('alt', True, 0, 0): 854862080,
    ('alt', True, 0, 64): 1484007680,
    ('alt', True, 4096, 0): 854862080,
    ('alt', True, 4096, 64): 1484007680,
    ('fastest', False, 0, 0): 838934016,
    ('fastest', False, 0, 64): 1468079616,
    ('fastest', False, 4096, 0): 838934016,
    ('fastest', False, 4096, 64): 1468079616,
    ('fastest', True, 0, 0): 844905984,
    ('fastest', True, 0, 64): 1474051584,
    ('fastest', True, 4096, 0): 844905984,
    ('fastest', True, 4096, 64): 1474051584,
    ('nobpp', False, 0, 0): 896084736,
    ('nobpp', False, 0, 64): 1525230336,
    ('nobpp', False, 4096, 0): 896084736,
    ('nobpp', False, 4096, 64): 1525230336,
    ('nobpp', True, 0, 0): 925944576,
    ('nobpp', True, 0, 64): 1555090176,
    ('nobpp', True, 4096, 0): 925944576,
    ('nobpp', True, 4096, 64): 1555090176,
}


def test_srtest150_workspaces_are_the_recorded_ones():
    recs = _srtest150()
    assert len(recs) == 219
    got = {}
    for config in ("nobpp", "fastest", "alt"):
        psets = _psets(config)
        for fp32 in (True, False):
            for max_structs in (0, 4096):
                for cand in (0, 64):
                    got[(config, fp32, max_structs, cand)] = _bytes(recs, psets, fp32=fp32, max_structs=max_structs, cand_per_nt=cand)
    assert got == SRTEST150


#: environment -> (pool_lists off, pool_lists on) for twenty records of 500 nt under nobpp without fp32 matrices
POOL_LISTS_500 = {
    (): (2782956032, 2942372608),
    (('SQ_KEPT_GB', '0.05'),): (2782956032, 2845063936),
    (('SQ_KEPT_PPS', '0.5'),): (2782956032, 2816543488),
    (('SQ_NO_POOL_KEPT', '1'),): (2782956032, 2782956032),
}


@pytest.mark.parametrize("env", [(), (("SQ_NO_POOL_KEPT", "1"),), (("SQ_KEPT_PPS", "0.5"),), (("SQ_KEPT_GB", "0.05"),)])
def test_kept_list_pages_of_twenty_500_nt_records(env, monkeypatch):
    for name, value in env:
        monkeypatch.setenv(name, value)
    recs, psets = _random_records(20, 500), _psets("nobpp")
    assert tuple(_bytes(recs, psets, pool_lists=on, fp32=False) for on in (False, True)) == POOL_LISTS_500[env]


#: (length, SQ_CTX_MIN_N or None) -> bytes for four records of that length under nobpp, max_structs 4096
CONTEXT_TABLES = {
    (300, None): 1530059776,
    (300, '-1'): 1530059776,
    (300, '200'): 1550380032,
    (1000, '-1'): 5959920640,
    (1000, '1001'): 5959920640,
    (1000, None): 6030253056,
    (2000, None): 6961591552,
    (2000, '-1'): 6813394176,
}


@pytest.mark.parametrize("n,ctx_min_n", [(300, None), (1000, None), (2000, None), (300, "-1"), (1000, "-1"), (2000, "-1"),
                                         (300, "200"), (1000, "1001")])
def test_context_tables_from_800_nt(n, ctx_min_n, monkeypatch):
    if ctx_min_n is not None:
        monkeypatch.setenv("SQ_CTX_MIN_N", ctx_min_n)
    assert _bytes(_random_records(4, n), _psets("nobpp"), max_structs=4096) == CONTEXT_TABLES[(n, ctx_min_n)]


def _record_kinds():
    """name -> (records, psets, _describe arguments): what a record or a job can carry beyond its letters."""
    rng = random.Random(3)
    nobpp, bpp12 = _psets("nobpp"), _psets("def")
    seqs = [_seq(n, 40 + n) for n in (60, 90, 120)]
    floats = [Prepared(s, [round(rng.random(), 3) for _ in s]) for s in seqs]
    encoded = [Prepared(s, "".join(rng.choice("abcdefghij") for _ in s)) for s in seqs]
    mixed = [floats[0], Prepared(seqs[1]), encoded[2]]
    pairs = [Prepared(s, None, "((" + "." * (len(s) - 4) + "))") for s in seqs]
    chains = [Prepared(s[:30] + "&" + s[30:50] + ";" + s[50:]) for s in seqs]
    plain = [Prepared(s) for s in seqs]
    njobs = len(seqs) * len(nobpp)
    own = [np.zeros((len(s), len(s))) for s in seqs for _ in nobpp]
    every_third = [m if j % 3 == 0 else None for j, m in enumerate(own)]
    # (the bpp term goes to the jobs of the paramsets with bpp != 0, of either sign)
    term = [np.zeros((len(s), len(s))) if ps["bpp"] != 0 else None for s in seqs for ps in bpp12]
    cols = [np.arange(len(s), dtype=np.int32) for s in seqs]
    shared = (_DeviceMatrix(150), cols, 2.5)
    return {
        "plain": (plain, nobpp, {}),
        "float reactivities": (floats, nobpp, {}),
        "encoded reactivities": (encoded, nobpp, {}),
        "reactivities on two of three": (mixed, nobpp, {}),
        "restraint pairs": (pairs, nobpp, {}),
        "chain separators": (chains, nobpp, {"interchainonly": True}),
        "caller matrices on every job": (plain, nobpp, {"ext": [(m, m) for m in own], "fp32": False}),
        "caller matrices on every third job": (plain, nobpp, {"ext": [(m, m) if m is not None else None for m in every_third], "fp32": False}),
        "caller matrices with fp32": (plain, nobpp, {"ext": [(m, m) if m is not None else None for m in every_third]}),
        "mul on every job": (plain, nobpp, {"mul": own, "fp32": False}),
        "mul on every third job": (plain, nobpp, {"mul": every_third, "fp32": False}),
        "caller matrices and mul on other jobs": (plain, nobpp, {"ext": [(m, m) if m is not None else None for m in every_third],
                                                                 "mul": [None if m is not None else own[j] for j, m in enumerate(every_third)],
                                                                 "fp32": False}),
        "bpp term of either sign": (plain, bpp12, {"bpp": term, "fp32": False}),
        "bpp term with fp32": (plain, bpp12, {"bpp": term}),
        "shared weighting matrix": (plain, _psets("ali"), {"mul_shared": shared, "fp32": False}),
        "Hungarian": (plain, _psets("hungariannobpp"), {}),
        "Nussinov": (plain, _psets("nussinovnobpp"), {}),
        "Edmonds": (plain, _psets("edmondsnobpp"), {}),
        "one job on one nucleotide": ([Prepared("A")], _psets("alt"), {}),
        "one record of 8,000 nt": ([Prepared(_seq(8000, 11))], _psets("alt"), {"fp32": False}),
        "one record of 32,000 nt": ([Prepared(_seq(32000, 12))], _psets("fastest"), {"fp32": False, "max_structs": 64}),
    }, njobs


#: name of _record_kinds -> bytes
RECORD_KINDS = {
    'plain': 718567168,
    'float reactivities': 718571264,
    'encoded reactivities': 718571264,
    'reactivities on two of three': 718569216,
    'restraint pairs': 718567168,
    'chain separators': 727012096,
    'caller matrices on every job': 720655104,
    'caller matrices on every third job': 718687488,
    'caller matrices with fp32': 719171840,
    'mul on every job': 719611136,
    'mul on every third job': 718385152,
    'caller matrices and mul on other jobs': 719913472,
    'bpp term of either sign': 721961216,
    'bpp term with fp32': 722639616,
    'shared weighting matrix': 716807680,
    'Hungarian': 717184256,
    'Nussinov': 717509632,
    'Edmonds': 716769024,
    'one job on one nucleotide': 106737664,
    'one record of 8,000 nt': 6701665280,
    'one record of 32,000 nt': 16975832832,
}


def test_what_a_record_or_a_job_carries():
    kinds, njobs = _record_kinds()
    assert njobs == 15
    got = {name: _bytes(recs, psets, **desc) for name, (recs, psets, desc) in kinds.items()}
    assert got == RECORD_KINDS


#: bytes of the "shared weighting matrix" descriptor under SQ_MUL_GATHER=1 (per-job slices of the matrix)
SHARED_GATHERED = 717016320


def test_shared_matrix_gathered_into_slices(monkeypatch):
    monkeypatch.setenv("SQ_MUL_GATHER", "1")
    recs, psets, desc = _record_kinds()[0]["shared weighting matrix"]
    assert _bytes(recs, psets, **desc) == SHARED_GATHERED
    assert SHARED_GATHERED != RECORD_KINDS["shared weighting matrix"]


#: (switch, value) -> bytes for SRtest150 under nobpp, fp32 on for SQ_LD_POW2 and off for the rest, max_structs 4096
SWITCHES = {
    ('SQ_FIN_STEM_CAP', '100000'): 884554752,
    ('SQ_FIN_STEM_CAP', '16'): 882955008,
    ('SQ_LD_POW2', '1'): 921650176,
    ('SQ_NO_SHARED_BITS', '1'): 896084736,
    ('SQ_OUT_CAP', '100000'): 765067008,
    ('SQ_OUT_CAP', '64'): 761869056,
}


@pytest.mark.parametrize("name,value", [("SQ_OUT_CAP", "64"), ("SQ_OUT_CAP", "100000"), ("SQ_FIN_STEM_CAP", "16"),
                                        ("SQ_FIN_STEM_CAP", "100000"), ("SQ_LD_POW2", "1"), ("SQ_NO_SHARED_BITS", "1")])
def test_switches_that_size_a_region(name, value, monkeypatch):
    monkeypatch.setenv(name, value)
    recs, psets = _srtest150(), _psets("nobpp")
    assert _bytes(recs, psets, fp32=name == "SQ_LD_POW2", max_structs=4096) == SWITCHES[(name, value)]


def test_the_numbers_the_issue_of_this_split_quoted():
    assert SRTEST150[("nobpp", False, 4096, 0)] == 896084736
    assert SRTEST150[("nobpp", True, 0, 0)] == 925944576
    assert POOL_LISTS_500[()][1] == 2942372608
    assert POOL_LISTS_500[(("SQ_NO_POOL_KEPT", "1"),)][1] == 2782956032


# ---- errors of the plan -------------------------------------------------------------------------------------------------

def _refused(b):
    with pytest.raises(RuntimeError) as got:
        b.workspace_bytes()
    return str(got.value)


def test_an_empty_batch_is_refused():
    assert _refused(_described([], [_psets("alt")])) == "libsquarna_hip: empty batch (code -1)"
    no_jobs = _described([Prepared("ACGU")], [[]])
    assert no_jobs.njobs == 0 and _refused(no_jobs) == "libsquarna_hip: empty batch (code -1)"


def test_a_sequence_beyond_32000_nt_is_refused():
    assert _refused(_described([Prepared("A" * 32001)], _psets("alt"))) == "libsquarna_hip: sequence longer than 32000 nt (code -1)"


@pytest.mark.parametrize("field,value", [("job_seq", 2), ("job_seq", -1), ("job_pset", 5), ("job_pset", -1)])
def test_a_job_out_of_range_is_refused(field, value):
    b = _described([Prepared("ACGUACGU"), Prepared("GGGAAACCC")], _psets("nobpp"))
    assert b.workspace_bytes() > 0
    getattr(b, field)[3] = value                                     # (the descriptor points at the batch's arrays)
    assert _refused(b) == "libsquarna_hip: bad job (code -1)"


# ---- size classes -------------------------------------------------------------------------------------------------------

def test_workspace_size_classes():
    MB = 1 << 20
    for want, size in ((1, MB), (MB, MB), (MB + 1, 2 * MB), (16 * MB - 1, 16 * MB),                       # 1-MB steps below 16 MB
                       (16 * MB, 16 * MB), (16 * MB + 1, 24 * MB), (100 * MB, 104 * MB), (256 * MB - 1, 256 * MB),   # 8-MB steps
                       (256 * MB, 256 * MB), (256 * MB + 1, 272 * MB), (300 * MB, 304 * MB), (511 * MB, 512 * MB),   # 16 per octave
                       (512 * MB, 512 * MB), (512 * MB + 1, 544 * MB), (896084736 + 256, 905969664),
                       (6 * 1024 * MB + 1, 6400 * MB), (2942372608 + 256, 2816 * MB)):
        assert P.workspace_size_class(want) == size, want


# ---- the descriptor -------------------------------------------------------------------------------------------------------

def test_one_list_for_all_records_and_per_record_lists_describe_the_same_jobs():
    recs = [Prepared("ACGUACGU"), Prepared("GGGAAACCC"), Prepared("AU")]
    a, b, c = dict(name="a"), dict(name="b"), dict(name="c")
    for ps in (a, b, c):
        ps.update(_psets("alt")[0])
    one = [a, b, a, c]                                               # (a paramset listed twice is one paramset, by identity)
    tiled = _described(recs, one)
    listed = _described(recs, [list(one) for _ in recs])
    for got in (tiled, listed):
        assert got.job_seq.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2] and got.job_seq.dtype == np.int32
        assert got.job_pset.tolist() == [0, 1, 0, 2, 0, 1, 0, 2, 0, 1, 0, 2] and got.job_pset.dtype == np.int32
        assert got.psets_py == [a, b, c] and all(x is y for x, y in zip(got.psets_py, (a, b, c)))
        d = got.desc
        assert (d.nseq, d.njobs, d.npset, d.max_structs, d.cand_per_nt, d.batch_flags, d.interchainonly) == (3, 12, 3, 0, 0, 0, 0)
        assert [d.seq_off[k] for k in range(4)] == [0, 8, 17, 19]
        assert [d.job_seq[j] for j in range(12)] == got.job_seq.tolist() and [d.job_pset[j] for j in range(12)] == got.job_pset.tolist()
        assert not d.reacts and not d.ext_score and not d.mul_score and not d.bpp_term and not d.mul_shared and not d.mul_matrix_dev
    assert tiled.seq_jobs is None and tiled._npl == 4
    assert listed.seq_jobs == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    assert tiled.workspace_bytes() == listed.workspace_bytes()
    # lists that differ from record to record
    uneven = _described(recs, [[c], [a, c], [b, b]])
    assert uneven.job_seq.tolist() == [0, 1, 1, 2, 2] and uneven.job_pset.tolist() == [0, 1, 0, 2, 2]
    assert uneven.psets_py == [c, a, b] and uneven.seq_jobs == [[0], [1, 2], [3, 4]]
    flags = _described(recs, one, pool_lists=True, fp32=False, max_structs=77, cand_per_nt=5, interchainonly=True).desc
    assert (flags.batch_flags, flags.max_structs, flags.cand_per_nt, flags.interchainonly) == (3, 77, 5, 1)
