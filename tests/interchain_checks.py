"""The multi-chain fold records of tests/test_hip_interchain.py, shared with tests/golden/gen_interchain_golden.py and
tests/test_oracle_golden.py: two and three chains ('&', ';') with three planted 12-nt reverse complements between chains, so
that a fold under interchainonly has stems to choose from (a random one is nearly empty).  Fixed by their seeds; a case has the
form of tests/lowcomplex.py's fixture cases (seq, reacts, restraints, config, kw), so that its check() and
test_hip_lowcomplex's _fold_one take it as it is."""
import functools
import random

PLANT = 12
SLOTS = (2, 15, 28)              # offsets of a chain's three 12-nt slots: a chain has at least 40 nt
POOLLIM = {"nobpp": 100, "greedynobpp": 5, "500nobpp": 1000, "fastest": 1}


def revcomp(seq):
    return "".join({"A": "U", "C": "G", "G": "C", "U": "A"}[ch] for ch in reversed(seq))


def fold_record(n, nchains, seed):
    """n characters, separators included: chains of about equal length, chain 0's slots 0 and 1 (and slot 2, or chain 1's slot
    0 when there are three chains) reverse-complemented into slots of other chains."""
    rng = random.Random(seed)
    seq = [rng.choice("ACGU") for _ in range(n)]
    seps = [n * (k + 1) // nchains for k in range(nchains - 1)]
    starts = [0] + [p + 1 for p in seps]
    ends = seps + [n]
    assert all(e - s >= SLOTS[-1] + PLANT for s, e in zip(starts, ends)), (n, nchains)
    last = nchains - 1
    plants = [((0, 0), (last, 2)), ((0, 1), (1, 1)), ((1, 0) if nchains > 2 else (0, 2), (last, 0))]
    for (ca, sa), (cb, sb) in plants:
        a, b = starts[ca] + SLOTS[sa], starts[cb] + SLOTS[sb]
        seq[b:b + PLANT] = revcomp("".join(seq[a:a + PLANT]))
    for k, p in enumerate(seps):
        seq[p] = "&;"[k % 2]
    return "".join(seq)


def _case(n, nchains, config, seed):
    return dict(tag="%d-%dchains" % (n, nchains), seq=fold_record(n, nchains, seed), reacts=None, restraints=None, config=config,
                kw=dict(poollim=POOLLIM[config]))


CHAINS = {96: 2, 130: 3, 256: 2, 257: 3, 300: 2, 600: 3, 1024: 2, 1025: 3}
#: (the seeds of the two shortest records are the first of 7096, 8096, ... / 7130, 8130, ... whose fold under either
#: configuration changes with the chain test: a case folds differently with interchainonly on and off)
SEED = {n: {96: 8096, 130: 9130}.get(n, 7000 + n) for n in CHAINS}
#: up to 256 nt: the scan form of the pool round kernel
SCAN = [_case(n, CHAINS[n], c, SEED[n]) for n in (96, 130, 256) for c in ("nobpp", "greedynobpp")]
#: 257-1,024 nt: the list form (E / H / N on interchain stem sets under 500nobpp)
LIST = [_case(n, CHAINS[n], c, SEED[n]) for n in (257, 300, 600) for c in ("nobpp", "greedynobpp")] + [_case(300, 2, "500nobpp", SEED[300])]
#: pools of width one: the persistent round kernel
ONE = [_case(n, CHAINS[n], "fastest", SEED[n]) for n in (300, 1024, 1025)]
#: beyond 1,024 nt with a pool: the launched kernels
LAUNCHED = [_case(1025, 3, "greedynobpp", SEED[1025])]
CASES = SCAN + LIST + ONE + LAUNCHED
#: the folds tests/golden/interchain.json holds from the reference itself (interchainonly on)
GOLDEN_FOLDS = (("130-3chains", "nobpp"), ("257-3chains", "greedynobpp"), ("300-2chains", "fastest"), ("300-2chains", "500nobpp"))


def case_id(c):
    return "%s-%s" % (c["tag"], c["config"])


def find(tag, config):
    return [c for c in CASES if c["tag"] == tag and c["config"] == config][0]


@functools.lru_cache(maxsize=None)
def oracle_fold(cid, interchainonly):
    """The oracle's fold of the case, in the list form test_hip_parity's _same_fold compares with; computed once."""
    from oracle import sqrn_oracle as O
    from squarna_amd.config import ParseConfig, builtin_config
    c = [c for c in CASES if case_id(c) == cid][0]
    names, psets = ParseConfig(builtin_config(c["config"]))
    out = O.SQRNdbnseq(c["seq"], None, None, None, psets, interchainonly=interchainonly, **c["kw"])
    return [out[0], [[d, list(s), list(p)] for d, s, p in out[1]], ["nan"] * 6, ["nan"] * 7]


def chain_of(seq):
    """Chain number of every position as BPMatrix counts them (SQRNdbnseq.py:264-271; separators keep 0)."""
    out, cur = [], 0
    for ch in seq:
        cur += ch in "&;"
        out.append(0 if ch in "&;" else cur)
    return out


def record_form(case, out):
    """A fold's tuple as a tests.lowcomplex.check fixture case."""
    from tests.lowcomplex import TOP, digest
    structs = [[d, [float(x) for x in sc], [int(p) for p in ps]] for d, sc, ps in out[1]]
    return dict(case, cons=out[0], nstruct=len(structs), top=structs[:TOP], digest=digest(structs))
