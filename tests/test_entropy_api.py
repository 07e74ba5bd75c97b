"""CPU tests of Entropy() / EntropyResult (no GPU): the helper the GPU tests compare against IS the reference (its rounded means
are the `entropy:` values of the golden texts), the public function through a CPU engine that answers with that helper, and
the validation of its arguments."""
import numpy as np
import pytest

from squarna_amd import engine as E
from tests import entropy_checks as EC
from tests.oracle_engine import OracleEngine


def entropy(**kw):
    from squarna_amd import Entropy
    with E.use_engine(EC.EntropyOracleEngine()):
        return Entropy(**kw)


def test_helper_gives_the_golden_values_of_seq_input():
    want = EC.golden_entropies("seq_input_entropy")
    got = [str(round(mean, 3)) for _, mean in EC.seq_input_reference()]
    assert len(want) == 17 and got == want


def test_helper_gives_the_golden_values_of_the_alignment():
    want = EC.golden_entropies("ali_input_a_entropy")
    got = [str(round(mean, 3)) for _, mean in EC.ali_input_reference()]
    assert len(want) == 33 and got == want


def test_entropy_of_seq_input():
    res = entropy(inputfile=EC.SEQ_INPUT, configfile="alt")
    recs = EC.parsed(EC.SEQ_INPUT)
    assert res.source == "host" and res.device.type == "cpu"
    assert [res.text(r) for r in range(len(res))] == EC.golden_entropies("seq_input_entropy")
    assert res.names == [rec[0] for rec in recs] and res.paramset_names == [res.paramset_names[0]] * 17
    seqs = [rec[1] for rec in recs]
    assert any(ch in "-.~" for sq in seqs for ch in sq) and any(ch in ";&" for sq in seqs for ch in sq)
    EC.check_layout(res, seqs)
    EC.check_close(res, seqs, EC.seq_input_reference(), tol=0.0)
    import torch
    assert res.position.dtype == torch.float64 and res.mean.dtype == torch.float64 and res.nstems.dtype == torch.int32
    assert res.lengths.dtype == torch.int64 and res.pos_off.dtype == torch.int64


def test_entropy_of_the_alignment_rows_with_the_stem_matrix():
    import torch
    sm = EC.ali_stem_matrix()
    want = EC.golden_entropies("ali_input_a_entropy")
    for given in (sm, torch.from_numpy(sm.copy())):
        res = entropy(inputfile=EC.ALI_INPUT, configfile="ali", stem_matrix=given)
        assert [res.text(r) for r in range(len(res))] == want
    EC.check_layout(res, res.sequences)
    EC.check_close(res, res.sequences, EC.ali_input_reference(), tol=0.0)


def test_records_and_inputseq_forms():
    recs = EC.parsed(EC.SEQ_INPUT)[:5]
    a = entropy(records=[tuple(rec) for rec in recs], configfile="alt")
    assert [a.text(r) for r in range(5)] == EC.golden_entropies("seq_input_entropy")[:5]
    plain = [rec[1] for rec in recs if not rec[2] and not rec[3]][:2]
    assert plain
    b = entropy(records=plain, c="alt")
    assert b.names == [">record1", ">record2"][:len(plain)] and b.sequences == plain
    for r, sq in enumerate(plain):
        c = entropy(inputseq=sq, config="alt")
        d = entropy(s=sq, configfile="alt")
        assert len(c) == 1 and c.sequences == [sq]
        assert torch_equal(c.position, b.row(r)) and torch_equal(d.position, b.row(r))


def torch_equal(a, b):
    return np.array_equal(a.numpy(), b.numpy(), equal_nan=True)


def test_paramset_by_name_and_by_index():
    from squarna_amd.config import ParseConfig, builtin_config
    names, psets = ParseConfig(builtin_config("nobpp"))
    assert len(names) >= 2
    seqs = ["GGGGAAAACCCCUUUUGGGGAAAACCCC", "GCGCGCAAAAGCGCGCUUUAGCGC"]
    for k in (0, len(names) - 1):
        a = entropy(records=seqs, configfile="nobpp", paramset=k)
        b = entropy(records=seqs, configfile="nobpp", paramset=names[k])
        assert a.paramset_names == b.paramset_names == [names[k]] * 2
        assert torch_equal(a.position, b.position) and torch_equal(a.mean, b.mean)
        EC.check_close(a, seqs, [EC.reference_rows(sq, None, None, psets[k]) for sq in seqs], tol=0.0)


def test_edge_records():
    """Fewer than 5 positions: no stem, rows and mean 0.0; no gap-free position: no finite row, mean NaN."""
    seqs = ["A", "GC-C", "----", "GG-GAAA-CCC"]
    res = entropy(records=seqs, configfile="alt")
    EC.check_layout(res, seqs)
    assert res.row(0).tolist() == [0.0] and float(res.mean[0]) == 0.0 and float(res.mean[1]) == 0.0
    assert np.isnan(res.row(2).numpy()).all() and np.isnan(float(res.mean[2])) and res.text(2) == "nan"
    assert np.isnan(res.cpu().to_padded().numpy()[0, 1:]).all()


def test_validation():
    seqs = ["GGGGAAAACCCC", "GGGGAAAACCCCA"]
    with pytest.raises(ValueError, match="Unknown paramset"):
        entropy(records=seqs, configfile="alt", paramset="nosuchset")
    for bad in (99, -1, 1.5, True):
        with pytest.raises(ValueError, match="Unknown paramset"):
            entropy(records=seqs, configfile="alt", paramset=bad)
    with pytest.raises(ValueError, match="stem_matrix: shape"):
        entropy(records=seqs[:1], configfile="alt", stem_matrix=np.ones((12, 11)))
    with pytest.raises(ValueError, match="stem_matrix: shape"):
        entropy(records=seqs[:1], configfile="alt", stem_matrix=np.ones(12))
    with pytest.raises(ValueError, match="stem_matrix: dtype"):
        entropy(records=seqs[:1], configfile="alt", stem_matrix=np.ones((12, 12), np.float32))
    with pytest.raises(ValueError, match="every record needs 12"):
        entropy(records=seqs, configfile="alt", stem_matrix=np.ones((12, 12)))
    with pytest.raises(ValueError, match="every record needs 14"):
        entropy(records=seqs[:1], configfile="alt", stem_matrix=np.ones((14, 14)))


def test_an_engine_without_entropy_tensors_is_refused():
    from squarna_amd import Entropy
    with E.use_engine(OracleEngine()):
        with pytest.raises(RuntimeError, match="entropy_tensors"):
            Entropy(records=["GGGGAAAACCCC"], configfile="alt")


def test_the_keywords_of_fold_raise_as_fold_does():
    from squarna_amd import Fold
    cases = [dict(inputfile="/no/such/file"), dict(records=["GGGAAACCC"], fileformat="pdf"),
             dict(records=["GGGAAACCC"], configfile="/no/such.conf"), dict(records=["GGGAAACCC"], inputformat="rt"),
             dict(records=["GGGAAACCC"], M="x"), dict(records=["GGGAAACCC"], B="y"), dict(records=[]),
             dict(records=[("a", "GGGAAACCC")])]
    for kw in cases:
        errors = []
        for fn in (Fold, entropy):
            with pytest.raises((AssertionError, ValueError)) as err:
                if fn is Fold:
                    with E.use_engine(OracleEngine()):
                        Fold(**kw)
                else:
                    entropy(**kw)
            errors.append((err.type, str(err.value)))
        assert errors[0] == errors[1], kw


def test_entropy_prints_nothing(capsys):
    entropy(inputfile=EC.SEQ_INPUT, configfile="alt")
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""
