"""GPU: the pairing predicate "may i pair with j" (SQRNdbnseq.py:286-304) on every kernel that states it, against the oracle.

The bit words a fold scans come from sq_bits_masks_kernel (letter masks: the default), from sq_bits_direct_kernel (cell by
cell: interchainonly batches, SQ_BITS_NOMASKS, mask tables beyond LDS) or from the presence of a value in the fp32 matrix
that sq_fill_kernel wrote (sq_bits_kernel, after sq_bpmatrix_fill).  No entry returns the words, so each route is read back
through AnnotateStems of the empty structure with minlen = 1 and no score threshold (tests/bits_checks.py): the stems --
(i, j, len) exactly and in the reference's order, bpscore within test_hip_parity's bar -- are the matrix cell for cell on the
visited diagonals.  All records go into one batch (mixed n, bits_off and nw per job; two pair tables, so two matrices per
record) and into a second one reversed; the 4,097-nt record (the fill kernel's generic path, the direct kernel's grid stride
over 129 x 33 tiles) is compared stems against stems at minlen = 3 in a batch of its own.

The VALUES of the fp32 matrix are not pinned here: no entry of the C ABI returns them and the library reads only their
presence."""
import os
import subprocess
import sys

import pytest

from tests import bits_checks as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = 2 * 2 * len(B.RECORDS)
#: the child process of test_cell_by_cell_without_the_chain_test gets twice the 5.4 s the same route -- both batches and the
#: long record, the process's first GPU call and the oracle's share included -- took in-process on an MI355X (the child
#: itself, interpreter start and imports included, took 3.7 s)
CHILD_TIMEOUT = 11


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("SQ_BITS_NOMASKS", "SQ_BITS_DIRECT", "SQ_NO_SHARED_BITS"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def golden():
    return B.load_golden()["stems"]


def test_default_route_letter_masks():
    """Batch(fp32=False): sq_bits_masks_kernel."""
    assert B.check_route() == JOBS


def test_default_route_long_record():
    assert B.check_route(big=True) == 2


def test_chain_test(golden):
    """interchainonly: sq_bits_direct_kernel with the chain test (:301), separators on word boundaries, tiles with s0 > 0; four
    records also against the reference's own stems (tests/golden/interchain.json)."""
    assert B.check_route(interchainonly=True, golden=golden) == JOBS


def test_chain_test_long_record():
    """129 x 33 tiles on a grid of 2,048 blocks: the direct kernel's stride loop."""
    nw, ntile = B.tiles_of(len(B.BIG[0]))
    assert nw * ntile > 2048
    assert B.check_route(interchainonly=True, big=True) == 2


def test_cell_by_cell_without_the_chain_test():
    """SQ_BITS_NOMASKS=1 is read once per process (sq_tuning), so the route runs in a fresh child: sq_bits_direct_kernel for
    batches without the chain test, the long record included."""
    env = dict(os.environ, SQ_BITS_NOMASKS="1")
    r = subprocess.run([sys.executable, "-m", "tests.bits_checks", "nomasks"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and "%d jobs, 0 mismatches" % (JOBS + 2) in r.stdout, (r.stdout + r.stderr)[-2000:]


@pytest.mark.parametrize("interchainonly", [False, True], ids=["all", "chain_test"])
def test_fp32_fill_then_bits_from_presence(interchainonly, golden):
    """Batch(fp32=True), sq_bpmatrix_fill, then the stems: sq_fill_kernel on its LDS fast path (no reactivities, no chain
    test) and its LDS per-cell path (the records with reactivities; every record under the chain test), sq_bits_kernel."""
    assert B.check_route(interchainonly, fp32=True, fill=True, golden=golden) == JOBS


@pytest.mark.parametrize("interchainonly", [False, True], ids=["all", "chain_test"])
def test_fp32_fill_long_record(interchainonly):
    """n > SQ_FILL_LDS_N: sq_fill_kernel's generic path (every input from global memory), then sq_bits_kernel."""
    assert B.check_route(interchainonly, fp32=True, fill=True, big=True) == 2


@pytest.mark.parametrize("interchainonly", [False, True], ids=["all", "chain_test"])
def test_fp32_fill_long_and_short_records_in_one_batch(interchainonly):
    """sq_fill_kernel picks its path per job: beside the 4,097-nt record (generic path) records of 33-300 nt stage their
    inputs in LDS, whose room the launch has to size by them and not by the longest sequence of the batch (it asked for none
    when that sequence was beyond SQ_FILL_LDS_N: the staging stores of the shorter jobs had no LDS behind them)."""
    assert B.check_route(interchainonly, fp32=True, fill=True, big="mixed") == 10


@pytest.mark.parametrize("interchainonly", [False, True], ids=["all", "chain_test"])
def test_fp32_fill_with_derived_bits(interchainonly, monkeypatch, golden):
    """SQ_BITS_DIRECT=1 (read when the batch is created): sq_bpmatrix_fill writes the fp32 matrix and derives the bit words
    from the inputs -- sq_bits_masks_kernel, or sq_bits_direct_kernel under the chain test -- instead of from the matrix."""
    monkeypatch.setenv("SQ_BITS_DIRECT", "1")
    assert B.check_route(interchainonly, fp32=True, fill=True, golden=golden) == JOBS
    assert B.check_route(interchainonly, fp32=True, fill=True, big=True) == 2
