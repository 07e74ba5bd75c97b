"""The low-complexity fold fixture, tests/golden/lowcomplex.json (written by tests/golden/gen_lowcomplex_golden.py from the
reference): repeats, G/C blocks, two- and three-letter alphabets and a stem-free sequence, placed on the kernels' switch
points.  One place for the digest of a fold and the comparison, shared by the generator, the oracle test and the GPU
tests."""
import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOP = 25          # structures stored in full per case (scores, paramsets); the rest only through the digest
TOL = 1e-5


def digest(structs):
    """sha256 over the whole ordered list of (dbn, paramsets) of one fold's structures."""
    body = json.dumps([[s[0], [int(p) for p in s[2]]] for s in structs], separators=(",", ":"))
    return hashlib.sha256(body.encode()).hexdigest()


def load():
    with open(os.path.join(GOLDEN, "lowcomplex.json")) as f:
        return json.load(f)


def fold_kwargs(case):
    return dict(case["kw"])


def check(got, case, tag=None):
    """One fold's (consensus, structures, ...) against a fixture case: consensus and every dbn exactly, the number of
    structures, the first TOP scores within TOL and their paramsets, and the digest of the whole list."""
    tag = tag or case["tag"]
    structs = list(got[1])
    assert got[0] == case["cons"], (tag, "consensus", got[0], case["cons"])
    assert len(structs) == case["nstruct"], (tag, "structures", len(structs), case["nstruct"])
    for k, (g, e) in enumerate(zip(structs, case["top"])):
        assert g[0] == e[0], (tag, k, g[0], e[0])
        assert len(g[1]) == len(e[1]) and all(abs(a - b) <= TOL for a, b in zip(g[1], e[1])), (tag, k, list(g[1]), e[1])
        assert [int(p) for p in g[2]] == e[2], (tag, k, list(g[2]), e[2])
    assert digest(structs) == case["digest"], (tag, "digest")
