"""Base-pair probabilities as device tensors (sq_batch_desc.bpp_matrix_dev, Batch(bpp_dev=...), Fold(bpp=...)) on the CPU: the
workspace a descriptor with device matrices books, the refusals of the library and of the Python layer, and Fold(bpp=...)
against the provider hook on the tests' CPU engine.  Needs the built library (python -m squarna_amd.build); no GPU: the size
query compares the device pointers with NULL and nothing else, and sq_batch_create refuses the descriptors below before it
touches the workspace."""
import ctypes as C

import numpy as np
import pytest
import torch

from squarna_amd import _lib, Fold
from squarna_amd import engine as E
from squarna_amd.bpp import bpp_terms, check_bpp_matrix
from squarna_amd.records import Prepared
from tests.oracle_engine import OracleEngine
from tests.test_batch_layout import RECORD_KINDS, _described, _psets, _record_kinds, _seq


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    from tests.test_batch_layout import ENV
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


class _DeviceTensor:
    """What Batch._describe asks of a record's matrix of probabilities, at an address nobody reads."""
    is_cuda = True

    def __init__(self, n, ld=None, dtype=torch.float64, shape=None, col_stride=1, ptr=0x20000):
        self.dtype, self.shape, self._stride, self._ptr = dtype, shape or (n, n), (ld or n, col_stride), ptr

    def dim(self):
        return len(self.shape)

    def stride(self, k=None):
        return self._stride if k is None else self._stride[k]

    def data_ptr(self):
        return self._ptr


def _bytes(records, psets, **desc):
    return _described(records, psets, **desc).workspace_bytes()


# ---- workspace bytes ----------------------------------------------------------------------------------------------------

def test_device_matrices_book_what_the_host_terms_book():
    recs, psets, desc = _record_kinds()[0]["bpp term of either sign"]
    assert _bytes(recs, psets, **desc) == RECORD_KINDS["bpp term of either sign"] == 721961216
    mats = [_DeviceTensor(len(p.shortseq), ptr=0x20000 + 8 * k) for k, p in enumerate(recs)]     # (8-byte aligned, never read)
    assert _bytes(recs, psets, bpp_dev=mats, fp32=False) == 721961216
    # ... as strided views of larger tensors too (the row stride does not enter the layout)
    views = [_DeviceTensor(len(p.shortseq), ld=len(p.shortseq) + 7) for p in recs]
    assert _bytes(recs, psets, bpp_dev=views, fp32=False) == 721961216
    assert _bytes(recs, psets, bpp_dev=mats) == RECORD_KINDS["bpp term with fp32"]
    # a record without a matrix books nothing for its bpp jobs, as a NULL bpp_term entry does
    assert _bytes(recs, psets, bpp_dev=[mats[0], None, None], fp32=False) == \
        _bytes(recs, psets, bpp=[t if j < len(psets) else None for j, t in enumerate(desc["bpp"])], fp32=False)
    # no matrix at all: the descriptor of a batch without the new fields
    b = _described(recs, _psets("nobpp"), bpp_dev=[None, None, None])
    assert not b.desc.bpp_matrix_dev and not b.desc.bpp_matrix_ld and b.workspace_bytes() == RECORD_KINDS["plain"]


def test_the_descriptor_carries_pointers_and_strides():
    recs = [Prepared(_seq(n, n)) for n in (5, 1, 9)]
    mats = [_DeviceTensor(5, ld=11, ptr=0x1008), None, _DeviceTensor(9, ptr=0x2000)]
    d = _described(recs, _psets("def"), bpp_dev=mats, fp32=False).desc
    assert [d.bpp_matrix_dev[k] for k in range(3)] == [0x1008, None, 0x2000]
    assert [d.bpp_matrix_ld[k] for k in range(3)] == [11, 1, 9]
    assert C.sizeof(_lib.BatchDesc) == C.sizeof(C.c_void_p) * 2 + _lib.BatchDesc.bpp_matrix_dev.offset
    assert _lib.BatchDesc.bpp_matrix_dev.offset == _lib.BatchDesc.mul_maxabs.offset + 8       # appended behind the last old field


# ---- refusals of the library ----------------------------------------------------------------------------------------------

def _create_refused(b):
    """sq_batch_create's status and message for a descriptor it refuses at its checks (before any device work: the workspace
    is an address nobody touches)."""
    L = _lib.load()
    h = C.c_void_p()
    rc = L.sq_batch_create(C.byref(h), C.byref(b.desc), C.c_void_p(1 << 20), C.c_size_t(b.workspace_bytes()), None)
    assert rc != 0 and not h.value
    return rc, L.sq_last_error().decode()


def _pset(bpp):
    return dict(_psets("nobpp")[0], bpp=bpp)


def test_a_job_with_a_device_matrix_takes_no_other_matrix():
    rec, m = [Prepared(_seq(20, 1))], [_DeviceTensor(20)]
    z = np.zeros((20, 20))
    for extra in (dict(bpp=[z]), dict(mul=[z]), dict(ext=[(z, z)])):
        rc, msg = _create_refused(_described(rec, [_pset(0.5)], bpp_dev=m, fp32=False, **extra))
        assert rc == -4 and "bpp_matrix_dev" in msg, (extra.keys(), rc, msg)
    from tests.test_batch_layout import _DeviceMatrix
    shared = (_DeviceMatrix(20), [np.arange(20, dtype=np.int32)], 1.0)
    rc, msg = _create_refused(_described(rec, [_pset(-1.0)], bpp_dev=m, fp32=False, mul_shared=shared))
    assert rc == -4 and "bpp_matrix_dev" in msg
    # a bpp == 0 job of the same sequence is not such a job: it may carry its own matrix
    b = _described(rec, [_pset(0.5), _pset(0)], bpp_dev=m, fp32=False, mul=[None, z])
    assert b.workspace_bytes() > 0


@pytest.mark.parametrize("power", [0.25, -2.0, 0.75])
def test_other_exponents_take_the_host_term(power):
    rc, msg = _create_refused(_described([Prepared(_seq(20, 1))], [_pset(power)], bpp_dev=[_DeviceTensor(20)], fp32=False))
    assert rc == -1 and "host term" in msg and "pow" in msg


def test_a_bpp_job_without_either_source_is_still_refused():
    recs = [Prepared(_seq(20, 1)), Prepared(_seq(21, 2))]
    rc, msg = _create_refused(_described(recs, [_pset(0.5)], bpp_dev=[_DeviceTensor(20), None], fp32=False))
    assert rc == -4 and "bpp != 0 paramsets need bpp_term" in msg
    rc, msg = _create_refused(_described(recs, [_pset(0.5)], fp32=False))
    assert rc == -4 and "bpp != 0 paramsets need bpp_term" in msg


def test_a_row_stride_below_the_length_is_refused():
    b = _described([Prepared(_seq(20, 1))], [_pset(1.0)], bpp_dev=[_DeviceTensor(20)], fp32=False)
    b._bpp_ld[0] = 19
    rc, msg = _create_refused(b)
    assert rc == -1 and "bpp_matrix_ld" in msg


# ---- refusals of the Python layer -----------------------------------------------------------------------------------------

BAD = [("a CUDA tensor", torch.zeros((6, 6), dtype=torch.float64)),
       ("a CUDA tensor", np.zeros((6, 6))),
       ("float64", _DeviceTensor(6, dtype=torch.float32)),
       ("6 x 6", _DeviceTensor(7)),
       ("6 x 6", _DeviceTensor(6, shape=(6, 6, 1))),
       ("6 x 6", _DeviceTensor(6, shape=(6, 5))),
       ("column stride", _DeviceTensor(6, ld=12, col_stride=2)),
       ("row stride", _DeviceTensor(6, ld=5))]


@pytest.mark.parametrize("what,m", BAD)
def test_matrices_the_python_layer_refuses(what, m):
    with pytest.raises(ValueError, match=what):
        check_bpp_matrix(m, 6)
    rec = [Prepared("GGGAAA")]
    with pytest.raises(ValueError, match=what):
        _described(rec, [_pset(0.5)], bpp_dev=[m], fp32=False)
    # the engine refuses before it builds anything (no GPU is asked for)
    for call in ("fold_records", "fold_tensors", "fold_records_packed"):
        with pytest.raises(ValueError, match=what):
            getattr(E.HipEngine(), call)([("GGGAAA", None, None, None, [_pset(0.5)], None)], bpp=[m])


def test_the_size_is_the_gap_free_length_with_separators():
    # 9 columns, 2 gaps, one separator: ViennaRNA gets 7 symbols (SQRNdbnseq.py:343-344)
    rec = [("GG-GA&A.C", None, None, None, [_pset(0.5)], None)]
    with pytest.raises(ValueError, match="7 x 7"):
        E.HipEngine().fold_records(rec, bpp=[_DeviceTensor(9)])
    with pytest.raises(ValueError, match="7 x 7"):
        E.HipEngine().fold_records(rec, bpp=[_DeviceTensor(6)])
    with pytest.raises(ValueError, match="2 matrices for 1 records"):
        E.HipEngine().fold_records(rec, bpp=[_DeviceTensor(7), None])
    with pytest.raises(ValueError, match="1 matrices for 2 records"):
        _described([Prepared("GGGAAA"), Prepared("GGGAAA")], [_pset(0.5)], bpp_dev=[_DeviceTensor(6)], fp32=False)


def test_records_carry_their_matrix_behind_the_block_fields():
    m = _DeviceTensor(6)
    short = [("GGGAAA", None, None, None, [], None)]
    blocks = [("GGGAAA", None, None, None, [], None, "name", "", 0)]
    for recs in (short, blocks):
        (r,) = E._with_bpp(recs, [m])
        assert len(r) == 10 and r[9] is m and r[:len(recs[0])] == recs[0] and E._bpp_of(r) is m
    assert E._bpp_of(short[0]) is None


def test_bpp_terms_routes_by_source_and_exponent():
    preps = [Prepared("GGGAAACCC"), Prepared("GGGGAAACCCC")]
    host = np.triu(np.arange(81, dtype=np.float64).reshape(9, 9), 1)
    dev = _DeviceTensor(11)
    half, one, odd, none = _pset(0.5), _pset(-1.0), _pset(0.25), _pset(0)
    terms, mats = bpp_terms(preps, [[half, none, one]] * 2, given=[host, dev], device=True)
    assert mats == [None, dev]
    assert [t is None for t in terms] == [False, True, False, True, True, True]
    assert np.array_equal(terms[0], (host / host.max()) ** 0.5) and np.array_equal(terms[2], host / host.max())
    # an all-zero host matrix: "the matrix stays as it is"
    terms, mats = bpp_terms(preps[:1], [[half]], given=[np.zeros((9, 9))], device=True)
    assert terms == [None] and mats is None
    # the provider's answer takes the same road as a given matrix
    old = E.set_bpp_provider(lambda seq, reacts, M, B: dev if len(seq) == 11 else host)
    try:
        terms, mats = bpp_terms(preps, [[half, one]] * 2, device=True)
        assert mats == [None, dev] and [t is None for t in terms] == [False, False, True, True]
        assert [t is None for t in bpp_terms(preps[:1], [[half, one]])] == [False, False]         # (the form of earlier versions)
    finally:
        E.set_bpp_provider(old)
    assert bpp_terms(preps, [[none]] * 2, device=True) == (None, None) and bpp_terms(preps, [[none]] * 2) is None

    class OnDevice(_DeviceTensor):
        def detach(self):
            return self

        def cpu(self):
            return torch.from_numpy(np.triu(np.ones((11, 11)), 1))
    # another exponent: the record's matrix comes to the host once and every job of the record takes the host term
    terms, mats = bpp_terms(preps[1:], [[half, odd]], given=[OnDevice(11)], device=True)
    assert mats is None and np.array_equal(terms[0], np.triu(np.ones((11, 11)), 1)) and np.array_equal(terms[1], terms[0])


# ---- Fold(bpp=...) on the CPU engine --------------------------------------------------------------------------------------

def _probabilities(seq):
    n = len(seq)
    rng = np.random.default_rng(n * 7919 + sum(map(ord, seq)))
    return np.triu(rng.random((n, n)) ** 3, 4)


class _ProviderEngine(OracleEngine):
    """The CPU oracle taking its probabilities from the product's provider hook, as the GPU engine does."""

    def fold_records(self, records, **opts):
        from oracle import sqrn_oracle as O
        from squarna_amd import bpp as B
        old, O.BPP_SOURCE = O.BPP_SOURCE, lambda seq, reacts, M, Bq: B._bpp_provider(seq, reacts, M, Bq)
        try:
            return super().fold_records(records, **opts)
        finally:
            O.BPP_SOURCE = old


def _same(a, b):
    assert a.source == b.source == "host"
    for key in ("partner", "scores", "pset_mask", "row_off", "cell_off", "nstruct", "lengths"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert torch.equal(torch.nan_to_num(a.metrics, nan=-7.0), torch.nan_to_num(b.metrics, nan=-7.0))


def test_fold_bpp_on_the_cpu_engine_equals_the_provider():
    seqs = ["GGGAAACCCUUAGGCAUCGAUGCCUA", "GCGCAAAAGCGCUUUUGCGC", "GGAUC-CGA&UCGGAUCC", "ACGUACGUAC"]
    short = [Prepared(s).shortseq for s in seqs]
    mats = [_probabilities(s) for s in short]
    mats[3] = np.zeros((10, 10))                                     # (max == 0: the matrix stays as it is)
    table = dict(zip(short, mats))
    calls = []

    def provider(seq, reacts, M, B):
        calls.append(seq)
        m = table[seq]
        return m if m.max() > 0 else None
    with E.use_engine(_ProviderEngine()):
        old = E.set_bpp_provider(provider)
        try:
            exp = Fold(records=seqs, configfile="def")
        finally:
            E.set_bpp_provider(old)
        assert calls
        got = Fold(records=seqs, configfile="def", bpp=mats)
        _same(got, exp)
        Lmax = max(len(s) for s in short)
        cube = torch.zeros((len(seqs), Lmax, Lmax), dtype=torch.float64)
        for k, m in enumerate(mats):
            cube[k, :len(m), :len(m)] = torch.from_numpy(m)
        before = cube.clone()
        _same(Fold(records=seqs, configfile="def", bpp=cube), exp)
        assert torch.equal(cube, before)
        # probabilities change the answer (the comparison above is not one of two defaults)
        flat = Fold(records=seqs, configfile="def", bpp=[np.triu(np.ones((len(s), len(s))), 4) for s in short])
        assert not torch.equal(flat.scores, exp.scores)
        # a record without a matrix keeps the provider
        old = E.set_bpp_provider(provider)
        try:
            _same(Fold(records=seqs, configfile="def", bpp=[mats[0], None, mats[2], None]), exp)
        finally:
            E.set_bpp_provider(old)
        for bad, what in (([mats[0]], "1 matrices for 4 records"), (mats[:3] + [np.zeros((9, 9))], "10 x 10"),
                          (cube[:, :5, :5], "Lmax"), (mats[:3] + [torch.zeros((10, 10), dtype=torch.int32)], "dtype")):
            with pytest.raises(ValueError, match=what):
                Fold(records=seqs, configfile="def", bpp=bad)
