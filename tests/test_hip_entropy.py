"""GPU tests of Entropy() / HipEngine.entropy_tensors / sq_entropy_rows: the row entropies of the stem matrix formed on the
device, against the reference's formula over the oracle's stems (tests/entropy_checks.reference_rows) within the derived
tolerance, the rounded strings of the golden texts, and bit for bit against itself: alone, in a batch, in other chunks, twice."""
import numpy as np
import pytest

from tests import entropy_checks as EC

pytestmark = pytest.mark.gpu

LENGTHS = (1, 4, 5, 16, 63, 64, 65, 127, 129, 300)


def _is_device(res):
    import torch
    assert res.source == "device"
    for key in ("lengths", "pos_off", "position", "mean", "nstems"):
        t = getattr(res, key)
        assert isinstance(t, torch.Tensor) and t.is_cuda, key
    assert res.position.dtype == torch.float64 and res.mean.dtype == torch.float64 and res.nstems.dtype == torch.int32
    assert res.lengths.dtype == torch.int64 and res.pos_off.dtype == torch.int64


def _same_bits(a, b):
    import torch
    a, b = a.cpu(), b.cpu()
    assert a.sequences == b.sequences
    for key in ("lengths", "pos_off", "nstems"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    for key in ("position", "mean"):                                 # (bit patterns: NaN at the gap columns compares equal)
        assert torch.equal(getattr(a, key).view(torch.int64), getattr(b, key).view(torch.int64)), key


def mixed_records():
    """Random records on every length boundary of the kernels (one wave's 64 columns, a block's 4 rows), gap columns,
    separators, a restraint line, reactivities, a dense GC repeat and a record without a stem."""
    rng = np.random.RandomState(20240607)
    rnd = lambda n: "".join(rng.choice(list("ACGU"), n))
    recs = [(">n%d" % n, rnd(n), None, None, None) for n in LENGTHS]
    gapped = list(rnd(70))
    for c in (0, 7, 8, 33, 69):
        gapped[c] = "-"
    recs.append((">gaps", "".join(gapped), None, None, None))
    recs.append((">seps", rnd(30) + ";" + rnd(25) + "&" + rnd(20), None, None, None))
    hp = "GGGGCUCAAAAGAGCCCCAUUGCGAAAGCAAU"
    recs.append((">restraints", hp, None, "((((" + "." * 10 + "))))" + "_" * 4 + "." * 10, None))
    recs.append((">reacts", rnd(90), [float(x) for x in rng.uniform(0, 1, 90).round(2)], None, None))
    recs.append((">gc_repeat", "GC" * 100, None, None, None))
    recs.append((">no_stem", "A" * 30, None, None, None))
    return recs


@pytest.fixture(scope="module")
def mixed():
    """(records, Entropy of them in one call, reference_rows of each): computed once, left unchanged."""
    from squarna_amd import Entropy
    recs = mixed_records()
    ps = EC.paramset0("alt")
    ref = [EC.reference_rows(rec[1], rec[2], rec[3], ps) for rec in recs]
    return recs, Entropy(records=recs, configfile="alt"), ref


def test_goldens_on_the_device():
    from squarna_amd import Entropy
    res = Entropy(inputfile=EC.SEQ_INPUT, configfile="alt")
    _is_device(res)
    assert [res.text(r) for r in range(len(res))] == EC.golden_entropies("seq_input_entropy")
    EC.check_layout(res, res.sequences)
    EC.check_close(res, res.sequences, EC.seq_input_reference())
    assert (res.nstems.cpu().numpy() >= 0).all()


def test_lengths_around_every_boundary_in_one_call(mixed):
    from squarna_amd import Entropy
    recs, res, ref = mixed
    _is_device(res)
    seqs = [rec[1] for rec in recs]
    EC.check_layout(res, seqs)
    EC.check_close(res, seqs, ref)
    nst = res.nstems.cpu().tolist()
    assert nst[0] == nst[1] == 0 and nst[-1] == 0 and nst[-2] > 0
    assert float(res.mean[0]) == 0.0 and float(res.mean[1]) == 0.0 and float(res.mean[-1]) == 0.0
    assert float(res.mean[-2]) > 1.0                                 # (the GC repeat: dense rows)
    import torch
    host = res.cpu()
    for r, rec in enumerate(recs):                                   # alone: other offsets, another batch -- the same bits
        one = Entropy(records=[rec], configfile="alt").cpu()
        assert one.row(0).view(torch.int64).tolist() == host.row(r).view(torch.int64).tolist(), rec[0]
        assert one.mean.view(torch.int64).tolist() == host.mean[r:r + 1].view(torch.int64).tolist(), rec[0]
        assert int(one.nstems[0]) == nst[r]


@pytest.mark.parametrize("budget", [300 * 300 * 8 + 4096, 65536])
def test_chunks_give_the_same_bits(mixed, monkeypatch, budget):
    """A scratch budget that holds the 300-nt record alone (three chunks or more), and one smaller than several records (a
    record larger than the budget gets a chunk of its own)."""
    from squarna_amd import Entropy
    from squarna_amd.batch import Batch
    from squarna_amd.engine import HipEngine
    recs, whole, _ = mixed
    inner, rows, calls = HipEngine.entropy_tensors, Batch.entropy_rows, []

    def small(self, *a, **kw):
        kw["scratch_bytes"] = budget
        return inner(self, *a, **kw)

    def counted(self, jobs, *a):
        calls.append(len(jobs))
        return rows(self, jobs, *a)
    monkeypatch.setattr(HipEngine, "entropy_tensors", small)
    monkeypatch.setattr(Batch, "entropy_rows", counted)
    res = Entropy(records=recs, configfile="alt")
    assert len(calls) >= 3 and sum(calls) == len(recs)
    _same_bits(res, whole)


def test_one_long_record():
    """1,100 nt: past a 1,024-thread block, 18 strides of a wave over a row, 275 blocks of rows."""
    from squarna_amd import Entropy
    rng = np.random.RandomState(11)
    seq = "".join(rng.choice(list("ACGU"), 1100))
    res = Entropy(records=[seq], configfile="alt")
    _is_device(res)
    EC.check_layout(res, [seq])
    EC.check_close(res, [seq], [EC.reference_rows(seq, None, None, EC.paramset0("alt"))])


def test_alignment_weights_stay_on_the_device(monkeypatch):
    import torch
    from squarna_amd import Entropy, FoldAlignment
    from squarna_amd.engine import HipEngine
    m = FoldAlignment(inputfile=EC.ALI_INPUT).stem_matrix
    assert m.is_cuda and m.dtype == torch.float64
    before = m.clone()
    seen, inner = [], HipEngine.entropy_tensors

    def spy(self, recs, *a, **kw):
        sm = kw.get("stem_matrix")
        seen.append((sm.data_ptr(), sm.is_cuda))
        return inner(self, recs, *a, **kw)
    monkeypatch.setattr(HipEngine, "entropy_tensors", spy)
    res = Entropy(inputfile=EC.ALI_INPUT, configfile="ali", stem_matrix=m)
    assert seen == [(m.data_ptr(), True)] and torch.equal(m, before)
    _is_device(res)
    assert [res.text(r) for r in range(len(res))] == EC.golden_entropies("ali_input_a_entropy")
    EC.check_layout(res, res.sequences)
    EC.check_close(res, res.sequences, EC.ali_input_reference(m.cpu().numpy()))


def test_run_to_run(mixed):
    from squarna_amd import Entropy
    recs, first, _ = mixed
    _same_bits(Entropy(records=recs, configfile="alt"), first)
