"""CPU tests of RowIdentity() / IdentityResult (no GPU): the numpy path under the test-only OracleEngine against the naive
reference of tests/identity_checks.py.  Integer comparisons are exact; identity() is one IEEE division of two exact integers
and is compared with Python's own quotient with ==."""
import pytest

from squarna_amd import engine as E
from tests.identity_checks import DENOMINATORS, as_lists, chain_rows, check_result, family_rows, mixed_rows, naive
from tests.oracle_engine import OracleEngine

ALI = "examples/ali_input.afa"


def identity(**kw):
    from squarna_amd import RowIdentity
    with E.use_engine(OracleEngine()):
        return RowIdentity(**kw)


def check(res, rows, denominator, T, matrix=True):
    import torch
    R = len(rows)
    assert res.source == "host" and res.device.type == "cpu" and (res.R, res.L, len(res)) == (R, len(rows[0]), R)
    assert (res.threshold_bp, res.denominator, res.sequences) == (T, denominator, rows)
    for key in ("len", "bases", "neighbours"):
        assert getattr(res, key).dtype == torch.int32 and tuple(getattr(res, key).shape) == (R,), key
    assert res.keep.dtype == torch.bool and tuple(res.keep.shape) == (R,)
    if matrix:
        assert res.same.dtype == res.both.dtype == torch.int32 and tuple(res.same.shape) == tuple(res.both.shape) == (R, R)
    else:
        assert res.same is None and res.both is None
    check_result(as_lists(res), naive(rows, denominator, T, matrix), (R, denominator, T))


@pytest.mark.parametrize("R,L", [(1, 30), (2, 9), (11, 30), (65, 70), (129, 40)])
def test_the_numpy_path_against_the_naive_reference(R, L):
    rows = mixed_rows(R * 1000 + L, R, L)
    for k, denominator in enumerate(DENOMINATORS):
        for T, threshold in ((0, 0), (8000, 0.8), (9700, 0.97), (10000, 1.0))[k % 2::2] + ((7000, 0.7),):
            check(identity(sequences=rows, threshold=threshold, denominator=denominator), rows, denominator, T)
    res = identity(sequences=rows)
    assert (res.threshold_bp, res.denominator) == (8000, "shorter") and res.names == [">record%d" % (k + 1) for k in range(R)]


def test_keyword_errors():
    rows = ["ACGU", "ACGA"]
    for kw in (dict(threshold=1.5), dict(threshold=-0.1), dict(threshold="high"), dict(threshold=None), dict(denominator="longer"),
               dict(denominator=0), dict(matrix="yes"), dict(matrix=1.5), dict(names=["one"])):
        with pytest.raises(ValueError, match="RowIdentity"):
            identity(sequences=rows, **kw)
    with pytest.raises(ValueError, match="RowIdentity"):
        identity()
    with pytest.raises(ValueError, match="RowIdentity"):
        identity(sequences=rows, inputfile=ALI)
    with pytest.raises(AssertionError):
        identity(sequences=["ACGU", "ACG"])


def test_the_three_input_forms():
    from squarna_amd import FoldAlignment
    with E.use_engine(OracleEngine()):
        ali = FoldAlignment(inputfile=ALI, step3="1")
    from_file, from_ali = identity(inputfile=ALI), identity(alignment=ali)
    from_seqs = identity(sequences=ali.sequences, names=ali.names)
    for res in (from_file, from_ali, from_seqs):
        assert res.names == ali.names and res.sequences == ali.sequences
        check(res, ali.sequences, "shorter", 8000)


def test_filtered_rows_feed_covariation():
    from squarna_amd import Covariation
    rows = family_rows(5, 40, 30, families=4, rate=0.08)
    res = identity(sequences=rows, names=["r%d" % k for k in range(40)], threshold=0.8)
    names, seqs = res.filtered()
    kept = [k for k, keep in enumerate(naive(rows, "shorter", 8000)["keep"]) if keep]
    assert res.kept().tolist() == kept and 1 < len(kept) < 40
    assert names == ["r%d" % k for k in kept] and seqs == [rows[k] for k in kept]
    with E.use_engine(OracleEngine()):
        cov, direct = Covariation(sequences=seqs, names=names), Covariation(sequences=[rows[k] for k in kept])
    assert cov.R == len(kept) and cov.names == names and cov.cov.tolist() == direct.cov.tolist() and cov.pair_cols.tolist() == direct.pair_cols.tolist()


def test_derived_values():
    import torch
    rows = mixed_rows(9, 30, 25)
    for denominator in DENOMINATORS:
        res = identity(sequences=rows, threshold=0.7, denominator=denominator)
        exp = naive(rows, denominator, 7000)
        assert res.weights().dtype == torch.float64 and res.weights().tolist() == [1 / n for n in exp["neighbours"]]
        assert res.neff().item() == torch.tensor([1 / n for n in exp["neighbours"]], dtype=torch.float64).sum().item()
        L = len(rows[0])
        den = lambda a, b: (min(exp["len"][a], exp["len"][b]) if denominator == "shorter" else exp["both"][a][b] if denominator == "aligned" else L)
        ident = [[exp["same"][a][b] / den(a, b) if den(a, b) else 0.0 for b in range(30)] for a in range(30)]
        assert res.identity().dtype == torch.float64 and res.identity().tolist() == ident
        rec = res.identity_of(3, 17)
        assert rec == dict(same=exp["same"][3][17], both=exp["both"][3][17], len_a=exp["len"][3], len_b=exp["len"][17], den=den(3, 17),
                           identity=ident[3][17], neighbours=den(3, 17) > 0 and exp["same"][3][17] * 10000 >= 7000 * den(3, 17))
        assert res.identity_of(5, 5)["neighbours"] is False
        best, where = res.nearest()
        others = [[ident[a][b] for b in range(30) if b != a] for a in range(30)]
        assert best.tolist() == [max(o) for o in others]
        assert where.tolist() == [min(b for b in range(30) if b != a and ident[a][b] == max(others[a])) for a in range(30)]
        mean = res.mean_identity().item()
        assert abs(mean - sum(ident[a][b] for a in range(30) for b in range(a + 1, 30)) / 435) <= 1e-12   # (435 sums of numbers <= 1)
    one = identity(sequences=["ACGU-N"])
    assert one.nearest()[0].tolist() == [0.0] and one.nearest()[1].tolist() == [-1] and one.mean_identity().item() == 0.0
    assert one.neighbours.tolist() == [1] and one.keep.tolist() == [True] and one.neff().item() == 1.0


def test_neighbours_at_the_threshold_are_the_neighbours():
    rows = mixed_rows(21, 66, 40)
    for denominator in DENOMINATORS:
        res = identity(sequences=rows, threshold=0.75, denominator=denominator)
        assert res.neighbours_at(0.75).dtype == res.neighbours.dtype and res.neighbours_at(0.75).tolist() == res.neighbours.tolist()
        for T in (0, 5000, 10000):
            assert res.neighbours_at(T / 10000).tolist() == naive(rows, denominator, T)["neighbours"], (denominator, T)
    with pytest.raises(ValueError, match="neighbours_at"):
        res.neighbours_at(2)


def test_cpu_and_the_matrix_less_result():
    rows = mixed_rows(4, 20, 33)
    full, bare = identity(sequences=rows, matrix=True), identity(sequences=rows, matrix=False)
    check(full, rows, "shorter", 8000)
    check(bare, rows, "shorter", 8000, matrix=False)
    for res in (full, bare):
        host = res.cpu()
        assert host is not res and as_lists(host) == as_lists(res) and (host.names, host.R, host.source) == (res.names, res.R, res.source)
    assert bare.weights().tolist() == full.weights().tolist() and bare.filtered() == full.filtered()
    for call in (bare.identity, bare.nearest, bare.mean_identity, lambda: bare.identity_of(0, 1), lambda: bare.neighbours_at(0.5)):
        with pytest.raises(ValueError, match="matrix=True"):
            call()


def test_matrix_defaults_to_the_row_count():
    from squarna_amd import row_identity as RI
    assert RI.MATRIX_ROWS == 4096
    few, many = ["ACGU"] * 3, ["ACGU"] * 5
    old = RI.MATRIX_ROWS
    try:
        RI.MATRIX_ROWS = 4                                                   # (the rule, not 4097 rows)
        assert identity(sequences=few).same is not None and identity(sequences=many).same is None
        assert identity(sequences=many, matrix=True).same is not None and identity(sequences=few, matrix=False).same is None
    finally:
        RI.MATRIX_ROWS = old


def test_the_filter_chain_keeps_the_even_rows():
    rows = chain_rows(130)
    for denominator in ("shorter", "aligned"):
        res = identity(sequences=rows, threshold=0.5, denominator=denominator)
        assert res.keep.tolist() == [k % 2 == 0 for k in range(130)] and res.neighbours.tolist() == [2] + [3] * 128 + [2]
