"""GPU: base-pair probabilities handed over as device tensors (sq_bpp_dev.hip, sq_batch_desc.bpp_matrix_dev,
Batch(bpp_dev=...), HipEngine.fold_*(bpp=...), Fold(bpp=...), a provider that returns CUDA tensors).

Exact equality throughout: the device forms (bppm / max) ** |bpp| with the two IEEE operations numpy performs for
|bpp| 1 and 0.5 (a division; a correctly rounded square root), so every term, every packed record and every table is
compared bit for bit with the host-term path of the same matrices.

The oracle's answers for the 400-nt record of the fold parity test are recorded (tests/golden/bpp_dev_400.json.gz, written by
tests/golden/gen_bpp_dev_golden.py: the CPU oracle takes 40 s for them); the four short records are folded by the oracle here."""
import gzip
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5


def conf(name):
    from squarna_amd.config import ParseConfig, builtin_config
    return ParseConfig(builtin_config(name))


def fake_bpp(seq, reacts=None, M=1.8, B=-0.6):
    """The synthetic probabilities of test_hip_parity.test_bpp_term_matches_oracle."""
    n = len(seq)
    rng = np.random.default_rng(n * 7919 + sum(map(ord, seq)))
    return np.triu(rng.random((n, n)) ** 3, 1)


def parity_sequences():
    """The four records of test_bpp_term_matches_oracle and one of 400 nt."""
    rng = np.random.default_rng(5)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in (40, 77, 120, 33)]
    return seqs + ["".join(np.random.default_rng(400).choice(list("ACGU"), 400))]


def _cuda(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64)).cuda()


def _sparse_cube(seq, seed):
    """Probabilities of fake_rna's form: u ** 3 on 60 % of the pairable cells with j >= i + 4, zero elsewhere."""
    n = len(seq)
    rng = np.random.default_rng(seed)
    u, keep = rng.random((n, n)), rng.random((n, n)) < 0.6
    pairs = {"GC", "CG", "AU", "UA", "GU", "UG"}
    ok = np.array([[j >= i + 4 and seq[i] + seq[j] in pairs for j in range(n)] for i in range(n)], bool).reshape(n, n)
    return np.where(ok & keep, u ** 3, 0.0)


def _same_fold(got, exp, tag):
    assert got[0] == exp[0], (tag, "consensus", got[0], exp[0])
    assert len(got[1]) == len(exp[1]), (tag, len(got[1]), len(exp[1]))
    for g, e in zip(got[1], exp[1]):
        assert g[0] == e[0], (tag, g, e)
        assert all(abs(a - b) <= TOL for a, b in zip(g[1], e[1])), (tag, g, e)
        assert list(g[2]) == list(e[2]), (tag, g, e)
    for g, e in zip(list(got[2]) + list(got[3]), list(exp[2]) + list(exp[3])):
        if e == "nan":
            assert g != g, tag
        else:
            assert abs(g - e) <= TOL, (tag, got[2], got[3], exp[2], exp[3])


class _NoProvider:
    """The provider hook must not be asked when every record brings its matrix."""

    def __enter__(self):
        from squarna_amd import engine as E

        def refuse(*a):
            raise AssertionError("the host provider was asked for a record that carries its matrix")
        self.old = E.set_bpp_provider(refuse)

    def __exit__(self, *a):
        from squarna_amd import engine as E
        E.set_bpp_provider(self.old)


# ---- 1. the bits of the terms -------------------------------------------------------------------------------------------
def test_term_bits_equal_the_host_terms():
    import torch
    from squarna_amd.engine import Batch, Prepared, bpp_terms
    sizes = (1, 5, 33, 64, 65, 130, 257)                              # odd N^2; below, at and across a wave; across the chunk
    rng = np.random.default_rng(17)
    seqs = ["".join(rng.choice(list("ACGU"), n)) for n in sizes]
    base = conf("nobpp")[1][0]
    psets = [dict(base, bpp=p) for p in (0.5, -0.5, 1.0, -1.0, 0)]
    host = [_sparse_cube(s, 100 + k) for k, s in enumerate(seqs)]
    host[0] = np.array([[0.7]])
    host[1][:] = host[1] * 0.5
    host[1][0, 0] = 0.9                                               # the maximum in the first element
    host[2][:] = host[2] * 0.5
    host[2][32, 32] = 0.8                                             # ... and in the last
    host[3][:] = 0.0                                                  # all zero: the matrix stays as it is
    host[4] = host[4] * 1e-30                                         # beside one whose maximum is 1.0: a maximum that leaks shows
    host[5][7, 90] = 1.0
    assert host[4].max() < 1e-30 and host[5].max() == 1.0 and host[6].max() < 1.0
    dev = [_cuda(m) for m in host]
    big = torch.full((141, 143), 5.0, dtype=torch.float64, device="cuda")     # a corner view with an odd row stride
    big[:130, :130] = dev[5]
    dev[5] = big[:130, :130]
    assert dev[5].stride() == (143, 1) and not dev[5].is_contiguous()
    flat = torch.full((257 * 257 + 1,), 9.0, dtype=torch.float64, device="cuda")   # a base 8 but not 16 bytes aligned
    flat[1:] = dev[6].reshape(-1)
    dev[6] = flat[1:].view(257, 257)
    assert dev[6].data_ptr() % 16 == 8
    before = [t.clone() for t in (big, flat)] + [t.clone() for t in dev[:5]]
    preps = [Prepared(s) for s in seqs]
    terms = bpp_terms(preps, [psets] * len(seqs), given=host)
    assert [t is None for t in terms[15:20]] == [True] * 5 and sum(t is not None for t in terms) == 4 * 6
    with Batch(preps, [psets] * len(seqs), bpp=terms) as hb, Batch(preps, [psets] * len(seqs), bpp_dev=dev) as db:
        assert hb.njobs == db.njobs == 35
        hb.fill()
        db.fill()
        for j in range(35):
            (hbool, hscore), (dbool, dscore) = hb.bpmatrix(j), db.bpmatrix(j)
            assert np.array_equal(hbool, dbool), j
            bad = np.flatnonzero(hscore.view(np.uint64).reshape(-1) != dscore.view(np.uint64).reshape(-1))
            assert bad.size == 0, (j, sizes[j // 5], psets[j % 5]["bpp"], bad[:5], hscore.reshape(-1)[bad[:5]], dscore.reshape(-1)[bad[:5]])
        # the added term is visible as it is where bpboolmatrix is 0: numpy's own bits, without the fill in between
        n = 130
        _, sc = db.bpmatrix(5 * 5 + 1)                                # N = 130, bpp = -0.5
        bl, _ = db.bpmatrix(5 * 5 + 4)
        exp = np.sqrt(host[5] / host[5].max())
        assert np.array_equal(sc[bl == 0].view(np.uint64), exp[bl == 0].view(np.uint64)) and (bl == 0).sum() > n * n // 2
    after = [big, flat] + dev[:5]
    assert all(torch.equal(a, b) for a, b in zip(after, before))      # the caller's tensors are only read


# ---- 2. whole folds: device path == host-provider path == oracle ---------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_400():
    with gzip.open(os.path.join(GOLDEN, "bpp_dev_400.json.gz"), "rb") as f:
        g = json.load(f)
    assert g["seq"] == parity_sequences()[-1] and g["config"] == "def"
    return g["folds"]


@pytest.mark.parametrize("poollim", [1000, 1])
def test_fold_parity_with_the_host_provider_and_the_oracle(poollim, oracle_400, monkeypatch):
    from squarna_amd import engine as E
    from oracle import sqrn_oracle as O
    made = []

    class Recorded(E.Batch):                                          # which road the matrices took into each batch
        def __init__(self, *a, **kw):
            made.append((sum(t is not None for t in kw.get("bpp") or []), sum(m is not None for m in kw.get("bpp_dev") or [])))
            super().__init__(*a, **kw)
    monkeypatch.setattr(E, "Batch", Recorded)
    names, psets = conf("def")
    seqs = parity_sequences()
    recs = [(s, None, None, None, psets, None) for s in seqs]
    dev = [_cuda(fake_bpp(s)) for s in seqs]
    before = [t.clone() for t in dev]
    eng = E.HipEngine()
    old = E.set_bpp_provider(fake_bpp)
    try:
        host_packed = [bytes(x) for x in eng.fold_records_packed(recs, poollim=poollim)]
    finally:
        E.set_bpp_provider(old)
    with _NoProvider():
        dev_packed = [bytes(x) for x in eng.fold_records_packed(recs, bpp=dev, poollim=poollim)]
        got = eng.fold_records(recs, bpp=dev, poollim=poollim)
    assert dev_packed == host_packed
    assert made == [(5 * 7, 0), (0, 5), (0, 5)]                       # (def.conf: 7 of 12 paramsets with bpp != 0)
    assert all(a.equal(b) for a, b in zip(dev, before))
    old_src, O.BPP_SOURCE = O.BPP_SOURCE, fake_bpp
    try:
        for s, g in zip(seqs[:4], got):
            exp = O.SQRNdbnseq(s, None, None, None, psets, poollim=poollim)
            _same_fold(g, [exp[0], [[d, list(sc), list(p)] for d, sc, p in exp[1]], ["nan"] * 6, ["nan"] * 7], s)
    finally:
        O.BPP_SOURCE = old_src
    cons, preds = oracle_400[str(poollim)]
    _same_fold(got[4], [cons, preds, ["nan"] * 6, ["nan"] * 7], "400 nt")


# ---- 3. the reference's own tuples (tests/golden/bpp.json: the real reference over tests/fake_rna.py) ---------------------
def test_reference_pin_through_device_matrices(fake_rna):
    import torch
    from squarna_amd import engine as E
    from squarna_amd.bpp import vienna_bpp
    names, psets = conf("def")
    with open(os.path.join(GOLDEN, "bpp.json")) as f:
        cases = json.load(f)["fold"]
    recs, mats, groups, zeros = [], [], {}, 0
    for k, c in enumerate(cases):
        p = E.Prepared(c["seq"], c["reacts"], c["restraints"])
        n = len(p.shortseq)
        m = vienna_bpp(p.shortseq, p.shortreacts if p.shortreacts is not None else [0.5] * n)
        if m is None:                                                  # the lengths with len % 11 == 7: all zero, rescaled or not
            assert n % 11 == 7
            m = np.zeros((n, n))
            zeros += 1
        recs.append((c["seq"], c["reacts"], c["restraints"], None, psets, None))
        mats.append(_cuda(m))
        groups.setdefault(json.dumps(c["kw"], sort_keys=True), []).append(k)
    assert zeros >= 2 and len(groups) == 2 and len(cases) >= 20
    eng = E.HipEngine()
    with _NoProvider():
        for key, idx in groups.items():
            kw = json.loads(key)
            if "rankby" in kw:
                kw["rankby"] = tuple(kw["rankby"])
            if "priority" in kw:
                kw["priority"] = set(kw["priority"])
            out = eng.fold_records([recs[k] for k in idx], bpp=[mats[k] for k in idx], **kw)
            for k, o in zip(idx, out):
                _same_fold(o, cases[k]["out"], (cases[k]["tag"], cases[k]["kw"]))
    assert torch.cuda.is_available()


# ---- 4. the public interface ----------------------------------------------------------------------------------------------
def _tables_equal(a, b):
    import torch
    for key in ("partner", "scores", "pset_mask", "row_off", "cell_off", "nstruct", "lengths"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert torch.equal(torch.nan_to_num(a.metrics, nan=-7.0), torch.nan_to_num(b.metrics, nan=-7.0))


def test_fold_api_and_a_provider_that_returns_device_tensors():
    import torch
    from squarna_amd import Fold, Predict
    from squarna_amd import engine as E
    seqs = parity_sequences()[:4] + ["GGGAUC-CGAAAG&CUUUCGGAUCCC"]
    short = [E.Prepared(s).shortseq for s in seqs]
    host = {s: fake_bpp(s) for s in short}
    dev = [_cuda(host[s]) for s in short]
    before = [t.clone() for t in dev]
    old = E.set_bpp_provider(lambda seq, reacts, M, B: host[seq])
    try:
        exp = Fold(records=seqs, configfile="def")
        buf = io.StringIO()
        Predict(inputseq=seqs[1], configfile="def", write_to=buf)
        exp_text = buf.getvalue()
    finally:
        E.set_bpp_provider(old)
    with _NoProvider():
        got = Fold(records=seqs, configfile="def", bpp=dev)
        assert got.source == "device"
        _tables_equal(got, exp)
        Lmax = max(len(s) for s in short)
        cube = torch.full((len(seqs), Lmax, Lmax), 3.0, dtype=torch.float64, device="cuda")     # (what lies beyond a corner is not read)
        for k, t in enumerate(dev):
            cube[k, :t.shape[0], :t.shape[1]] = t
        cube0 = cube.clone()
        _tables_equal(Fold(records=seqs, configfile="def", bpp=cube), exp)
        assert torch.equal(cube, cube0)
        # host matrices are uploaded once per record; fp32 ones are widened on the device (exactly representable values here)
        _tables_equal(Fold(records=seqs, configfile="def", bpp=[host[s] for s in short]), exp)
        half = [torch.from_numpy(np.triu(np.round(host[s] * 256) / 256, 1)).float() for s in short]
        _tables_equal(Fold(records=seqs, configfile="def", bpp=[t.cuda() for t in half]),
                      Fold(records=seqs, configfile="def", bpp=[t.double() for t in half]))
    assert all(torch.equal(a, b) for a, b in zip(dev, before))
    # a provider that answers with CUDA tensors: Predict's text is the numpy provider's
    by_seq = dict(zip(short, dev))
    old = E.set_bpp_provider(lambda seq, reacts, M, B: by_seq[seq])
    try:
        buf = io.StringIO()
        Predict(inputseq=seqs[1], configfile="def", write_to=buf)
        assert buf.getvalue() == exp_text and "\n" in exp_text
        _tables_equal(Fold(records=seqs, configfile="def"), exp)
    finally:
        E.set_bpp_provider(old)
    assert all(torch.equal(a, b) for a, b in zip(dev, before))
