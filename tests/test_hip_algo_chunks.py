"""sq_run_algo in more than one chunk: when the candidate arena does not hold the matching scratch of all jobs, the driver
builds, launches and collects chunk after chunk (algo_build from k0 > 0) -- a path no fold of the suite's batches reaches."""
import random

import pytest

from tests.test_hip_parity import conf, prep

pytestmark = pytest.mark.gpu

# Arena of a batch of 150-nt records created with cand_per_nt 1: max(max_structs x 1,835, 11,266) records of 32 bytes (the
# estimate of the runs of a 150-nt record at minlen 2; the floor of the dense read-back).  A 150-nt job takes 475,136 bytes of
# scratch under Nussinov, 186,368 under Hungarian and 60-150 KB under Edmonds:
#   E, H  max_structs  7: 411 KB -- at most six Edmonds, at most two Hungarian jobs per chunk
#   N     max_structs 19: 1.1 MB -- two Nussinov jobs per chunk
MAX_STRUCTS = {"E": 7, "H": 7, "N": 19}


def _builds(capfd):
    return sum(line.startswith("[sq_algos] build algo") for line in capfd.readouterr().err.split("\n"))


@pytest.mark.parametrize("algo", "EHN")
def test_runalgo_in_several_chunks_equals_one_chunk(algo, monkeypatch, capfd):
    from squarna_amd.engine import Batch
    names, psets = conf("nobpp")
    p = dict(zip(names, psets))["def" + algo]
    rng = random.Random(150)
    seqs = ["".join(rng.choice("ACGU") for _ in range(150)) for _ in range(10)]
    monkeypatch.setenv("SQ_TIMING", "1")
    monkeypatch.setenv("SQ_NO_DEVICE_ALGOS", "1")
    jobs = list(range(len(seqs)))
    capfd.readouterr()
    with Batch([prep(s) for s in seqs], [[p]] * len(seqs)) as b:
        one = b.run_algo(jobs, algo)
    assert _builds(capfd) == 1
    with Batch([prep(s) for s in seqs], [[p]] * len(seqs), max_structs=MAX_STRUCTS[algo], cand_per_nt=1) as b:
        got = b.run_algo(jobs, algo)
    assert _builds(capfd) >= 2
    assert got == one and sum(len(g) for g in got) > len(seqs)
