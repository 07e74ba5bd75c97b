"""The engine's sub-batch planner, its capacity retry, the sizing arithmetic and the Python switches, on the CPU through stubs.

Every expected number below was recorded from the behaviour of commit adce493 (engine.py as one module: the closures of
HipEngine._fold_in_sub_batches, the retry loop inside HipEngine._fold_groups, the two copies of the sizing formulas, the inline
os.environ reads) and is kept as a literal: the tests that go through HipEngine pass on that commit unchanged, the ones on
plan.SubBatchPlan / plan.slot_bytes / plan.default_structs / switches repeat the same cases on the units."""
import random

import pytest

from squarna_amd import _lib, engine as E, plan as P, switches as S

PS = {"suboptmin": .9, "suboptmax": .99, "algorithms": "G", "minlen": 2.0, "bpweights": 1}
PSETS = [PS]
ENV = ("SQ_NO_POOL_KEPT", "SQ_KEPT_PPS", "SQ_MUL_GATHER", "SQ_DENSE_GB", "SQ_ENGINE_SUBLANES", "SQ_ENGINE_LANES",
       "SQ_NO_DETACH", "SQ_NO_PACKED_ROWS")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _records(lengths, matrix=False):
    return [("A" * n, None, None, None, PSETS) + ((object(),) if matrix else ()) for n in lengths]


def _slots(records, poollim=1000):
    return E.pool_slots_wanted_many([len(r[0]) for r in records], [r[4] for r in records], poollim).tolist()


def _three_hundred():
    rng = random.Random(1)
    recs = _records([rng.randint(250, 520) for _ in range(300)])
    return recs, _slots(recs)


# ---- the plan, through HipEngine._fold_in_sub_batches with _fold_groups replaced --------------------------------------------

def _plan_through_engine(records, per_rec, cap, script, eng=None, raise_at=None, **opts):
    """(engine, [(records of the sub-batch, its slots hint, batches in flight)]) of one _fold_in_sub_batches call whose folds
    answer (driver, peak) from `script`; raise_at: the fold of that call (1-based) raises instead."""
    eng = eng or E.HipEngine()
    calls, answers = [], iter(script)

    def fold_groups(groups, hints, o, info=None, inflight=1):
        calls.append((len(groups[0]), hints[0], inflight))
        if len(calls) == raise_at:
            raise raise_at_error
        info["driver"], info["peak"] = next(answers)
        return [[("r", len(calls))] * len(groups[0])], [[None] * len(groups[0])]
    eng._fold_groups = fold_groups
    opts.setdefault("poollim", 1000)
    out = eng._fold_in_sub_batches(records, per_rec, cap, opts)
    assert len(out) == len(records) and None not in out
    return eng, calls


raise_at_error = RuntimeError("the fold of a sub-batch failed")


def _plan_alone(per_rec, cap, script, scale=1.0, dense=None, dense_cap=32e9):
    """The same walk on plan.SubBatchPlan without any engine: ([(records, hint)], plan)."""
    plan = P.SubBatchPlan(per_rec, dense or [0.0] * len(per_rec), cap, dense_cap, 1, scale)
    calls, answers = [], iter(script)
    while True:
        job = plan.take()
        if job is None:
            return calls, plan
        lo, hi, hint = job
        calls.append((hi - lo, hint))
        plan.report(lo, hi, *next(answers))


def test_first_sub_batch_scales_the_rest_and_the_memo_sizes_the_next_call():
    recs, per = _three_hundred()
    script = [(2, 900), (2, 800)] + [(3, 0)] * 8
    eng, calls = _plan_through_engine(recs, per, 60000, script)
    assert calls == [(45, 58836, 1), (255, 10563, 1)]
    assert list(eng._pool_scale.values()) == [0.030593514174994903]
    assert (eng.last_fold_driver, eng.last_fold_peak) == (2, 900)
    assert eng.last_ref_scores == [None] * 300
    eng, calls = _plan_through_engine(recs, per, 60000, script, eng=eng)           # the memo is warm
    assert calls == [(300, 12363, 1)]
    assert list(eng._pool_scale.values()) == [0.004454243780762121]
    # another pool limit is another key
    _plan_through_engine(recs, per, 60000, script, eng=eng, poollim=999)
    assert len(eng._pool_scale) == 2

    calls, plan = _plan_alone(per, 60000, script)
    assert calls == [(45, 58836), (255, 10563)] and plan.scale == 0.030593514174994903
    assert (plan.driver, plan.peak) == (2, 900)
    calls, plan = _plan_alone(per, 60000, script, scale=plan.scale)
    assert calls == [(300, 12363)] and plan.scale == 0.004454243780762121


def test_host_loop_fallback_widens_the_scale_by_four_up_to_one():
    recs, per = _three_hundred()
    script = [(2, 900), (3, 0)]
    eng, calls = _plan_through_engine(recs, per, 60000, script)
    assert calls == [(45, 58836, 1), (255, 10563, 1)]
    assert list(eng._pool_scale.values()) == [0.12237405669997961]            # 4 x 0.0305935...
    assert (eng.last_fold_driver, eng.last_fold_peak) == (3, 900)
    always3 = [(3, 0)] * 7
    eng, calls = _plan_through_engine(recs, per, 60000, always3)
    assert calls == [(45, 58836, 1), (41, 58015, 1), (44, 58138, 1), (42, 58588, 1), (43, 56892, 1), (42, 56908, 1), (43, 56732, 1)]
    assert list(eng._pool_scale.values()) == [1.0]                            # (never above the estimate itself)
    assert (eng.last_fold_driver, eng.last_fold_peak) == (3, 0)

    calls, plan = _plan_alone(per, 60000, script)
    assert calls == [(45, 58836), (255, 10563)] and plan.scale == 0.12237405669997961
    calls, plan = _plan_alone(per, 60000, always3)
    assert [c[0] for c in calls] == [45, 41, 44, 42, 43, 42, 43] and plan.scale == 1.0
    plan = P.SubBatchPlan(per, [0.0] * len(per), 60000, 32e9, 1, 0.1)
    scales = []
    for _ in range(3):
        plan.report(0, 1, 3, 0)
        scales.append(plan.scale)
    assert scales == [0.4, 1.0, 1.0]                                          # (not 1.6)


def test_a_first_sub_batch_without_a_peak_leaves_the_scale():
    recs, per = _three_hundred()
    script = [(2, 0), (2, 700), (2, 5)]
    eng, calls = _plan_through_engine(recs, per, 60000, script)
    assert calls == [(45, 58836, 1), (41, 58015, 1), (214, 6933, 1)]          # the second one is the first that counts
    assert list(eng._pool_scale.values()) == [0.024131690080151685]
    assert (eng.last_fold_driver, eng.last_fold_peak) == (2, 700)

    calls, plan = _plan_alone(per, 60000, script)
    assert calls == [(45, 58836), (41, 58015), (214, 6933)] and plan.scale == 0.024131690080151685


def test_dense_matrices_cut_sub_batches_of_equal_weight(monkeypatch):
    recs = _records([200 + 20 * (k % 7) for k in range(40)], matrix=True)
    per = _slots(recs)
    monkeypatch.setenv("SQ_DENSE_GB", "0.01")
    eng, calls = _plan_through_engine(recs, per, 10 ** 9, [(2, 0)] * 9)
    assert calls == DENSE_CALLS
    assert list(eng._pool_scale.values()) == [1.0]
    monkeypatch.setenv("SQ_DENSE_GB", "32")
    assert _plan_through_engine(recs, per, 10 ** 9, [(2, 0)])[1] == [(40, sum(c[1] for c in DENSE_CALLS), 1)]

    dense = [12.0 * len(r[0]) ** 2 for r in recs]
    calls, _ = _plan_alone(per, 10 ** 9, [(2, 0)] * 9, dense=dense, dense_cap=0.01e9)
    assert calls == [c[:2] for c in DENSE_CALLS]


DENSE_CALLS = [(12, 8146, 1), (11, 8403, 1), (11, 8481, 1), (6, 4188, 1)]


def test_a_record_beyond_the_cap_is_a_sub_batch_of_its_own():
    recs = _records([100, 900, 100, 100])
    per = _slots(recs)
    assert per == [40, 1512, 40, 40]
    eng, calls = _plan_through_engine(recs, per, 1000, [(2, 0)] * 3)
    assert calls == [(1, 40, 1), (1, 1512, 1), (2, 80, 1)]
    assert _plan_alone(per, 1000, [(2, 0)] * 3)[0] == [(1, 40), (1, 1512), (2, 80)]


def test_the_error_of_a_sub_batch_is_raised_as_it_is_and_ends_the_walk():
    recs, per = _three_hundred()
    eng = E.HipEngine()
    with pytest.raises(RuntimeError) as got:
        _plan_through_engine(recs, per, 60000, [(2, 0)] * 9, eng=eng, raise_at=2)
    assert got.value is raise_at_error
    assert eng._pool_scale and eng.last_ref_scores is None                    # (one report came in; no result went out)

    plan = P.SubBatchPlan(per, [0.0] * len(per), 60000, 32e9, 1, 1.0)
    assert plan.take() == (0, 45, 58836)
    plan.fail(raise_at_error)
    plan.fail(ValueError("a later one"))
    assert plan.take() is None and plan.error is raise_at_error


def test_text_blocks_keep_the_sub_batches_on_one_lane(monkeypatch):
    recs, per = _three_hundred()
    monkeypatch.setenv("SQ_ENGINE_SUBLANES", "2")
    eng, calls = _plan_through_engine(recs, per, 60000, [(2, 900), (2, 800)], _blocks={"psnames": []})
    assert calls == [(45, 58836, 1), (255, 10563, 1)]                         # (two lanes: half the slots each, inflight 2)
    plan = P.SubBatchPlan(per, [0.0] * len(per), 60000, 32e9, 2, 1.0)
    assert plan.take() == (0, 24, 29393)


# ---- the capacity retry, through HipEngine._fold_groups with _make_batch / _fits_device replaced ------------------------------

class _FakeBatch:
    nseq = 2
    fold_driver = 2
    fold_peak_structs = 77

    def __init__(self, log, grow, answer):
        self.log, self.grow, self.answer, self.closed = log, grow, answer, False
        log.append(("make", grow))

    def fold(self, **opts):
        assert not self.closed
        self.log.append(("fold", self.grow))
        if self.answer is not None:
            raise self.answer

    def close(self):
        if not self.closed:
            self.log.append(("close", self.grow))
        self.closed = True

    def results_all(self):
        return [(("cons", self.grow), None)] * self.nseq


def _retry(answers, fits=True):
    """(engine, log, batches) of one _fold_groups call whose k-th batch answers its fold with answers[k] (None: it holds)."""
    eng, log, made = E.HipEngine(), [], []

    def make_batch(records, slots_hint, opts, grow=(1, 1)):
        made.append(_FakeBatch(log, grow, answers[len(made)]))
        return made[-1], {}

    def fits_device(records, slots_hint, opts, grow):
        log.append(("fits?", grow))
        return fits
    eng._make_batch, eng._fits_device = make_batch, fits_device
    return eng, log, made


def _cap(kind):
    return _lib.CapacityError("capacity %d" % kind, kind)


def test_an_outgrown_batch_is_closed_and_made_again_four_times_as_large():
    eng, log, made = _retry([_cap(_lib.CAP_CANDIDATES), _cap(_lib.CAP_STRUCTS), None])
    outs, refs = eng._fold_groups([_records([30, 40])], [None], {})
    assert outs == [[("cons", (4, 4))] * 2] and refs == [[None, None]]
    assert log == [("make", (1, 1)), ("fold", (1, 1)), ("fits?", (4, 1)), ("close", (1, 1)),
                   ("make", (4, 1)), ("fold", (4, 1)), ("fits?", (4, 4)), ("close", (4, 1)),
                   ("make", (4, 4)), ("fold", (4, 4)), ("close", (4, 4))]
    assert eng.capacity_retries == 2
    assert (eng.last_fold_driver, eng.last_fold_peak) == (2, 77)
    assert all(b.closed for b in made)


def test_an_output_overflow_grows_the_candidate_room():
    eng, log, made = _retry([_cap(_lib.CAP_OUTPUT), None])
    eng._fold_groups([_records([30, 40])], [None], {})
    assert [g for what, g in log if what == "make"] == [(1, 1), (4, 1)]
    assert eng.capacity_retries == 1 and all(b.closed for b in made)


@pytest.mark.parametrize("kind", [_lib.CAP_FIXED, 0, 99])
def test_a_capacity_nothing_can_grow_is_raised_at_once(kind):
    err = _cap(kind)
    eng, log, made = _retry([err, None])
    with pytest.raises(_lib.CapacityError) as got:
        eng._fold_groups([_records([30, 40])], [None], {})
    assert got.value is err
    assert log == [("make", (1, 1)), ("fold", (1, 1)), ("close", (1, 1))]
    assert eng.capacity_retries == 0 and all(b.closed for b in made)


def test_a_grown_batch_that_would_not_fit_raises_the_original_error():
    err = _cap(_lib.CAP_STRUCTS)
    eng, log, made = _retry([err, None], fits=False)
    with pytest.raises(_lib.CapacityError) as got:
        eng._fold_groups([_records([30, 40])], [None], {})
    assert got.value is err
    assert log == [("make", (1, 1)), ("fold", (1, 1)), ("fits?", (1, 4)), ("close", (1, 1))]
    assert eng.capacity_retries == 0 and all(b.closed for b in made)


def test_the_eighth_failure_is_raised():
    errs = [_cap(_lib.CAP_CANDIDATES) for _ in range(9)]
    eng, log, made = _retry(errs)
    with pytest.raises(_lib.CapacityError) as got:
        eng._fold_groups([_records([30, 40])], [None], {})
    assert got.value is errs[7]
    assert [g for what, g in log if what == "make"] == [(4 ** k, 1) for k in range(8)]
    assert eng.capacity_retries == 7 and len(made) == 8 and all(b.closed for b in made)


def test_another_error_of_the_fold_closes_the_batch():
    err = ValueError("not a capacity")
    eng, log, made = _retry([err])
    with pytest.raises(ValueError) as got:
        eng._fold_groups([_records([30, 40])], [None], {})
    assert got.value is err and all(b.closed for b in made)


# ---- the sizing arithmetic ---------------------------------------------------------------------------------------------

#: environment -> per length n: (n, kept-list bytes per slot, pool_slot_cap(n) without a GPU, the least free device memory at
#: which HipEngine._fits_device lets each of _FITS_CASES grow)
_FITS_CASES = [  # (jobs, HipEngine(max_structs), HipEngine(cand_per_nt), poollim, grow)
    (3, 0, 0, 1000, (1, 1)), (3000, 0, 0, 1000, (4, 1)), (100000, 0, 0, 1, (4, 4)), (10, 5000, 100, 1000, (1, 16))]
_SIZES = {
    (): [
        (100, 0, 389884, [62619648, 10006656000, 343081484288, 1200640000]),
        (256, 0, 201528, [122683392, 25506816000, 868657135616, 2338816000]),
        (257, 14344, 100256, [240279552, 25949568000, 871950712832, 4635392000]),
        (500, 38920, 44834, [535461888, 50684736000, 1690711359488, 10346240000]),
        (1024, 156674, 13989, [1701855232, 105575472000, 3456106496000, 33009984000]),
        (1025, 0, 59642, [418471936, 101913792000, 3459400073216, 7943680000]),
        (3000, 0, 21218, [1179189248, 298150656000, 10113398079488, 22359040000])],
    (("SQ_NO_POOL_KEPT", "1"),): [
        (100, 0, 389884, [62619648, 10006656000, 343081484288, 1200640000]),
        (256, 0, 201528, [122683392, 25506816000, 868657135616, 2338816000]),
        (257, 0, 201414, [122773504, 25605312000, 871950712832, 2340352000]),
        (500, 0, 114789, [216629248, 49750656000, 1690711359488, 4119040000]),
        (1024, 0, 59652, [418381824, 101815296000, 3456106496000, 7942144000]),
        (1025, 0, 59642, [418471936, 101913792000, 3459400073216, 7943680000]),
        (3000, 0, 21218, [1179189248, 298150656000, 10113398079488, 22359040000])],
    (("SQ_KEPT_PPS", "2.5"),): [
        (100, 0, 389884, [62619648, 10006656000, 343081484288, 1200640000]),
        (256, 0, 201528, [122683392, 25506816000, 868657135616, 2338816000]),
        (257, 32776, 60931, [391274496, 26391936000, 871950712832, 7584512000]),
        (500, 32776, 49606, [485130240, 50537280000, 1690711359488, 9363200000]),
        (1024, 32776, 35447, [686882816, 102601920000, 3456106496000, 13186304000]),
        (1025, 0, 59642, [418471936, 101913792000, 3459400073216, 7943680000]),
        (3000, 0, 21218, [1179189248, 298150656000, 10113398079488, 22359040000])],
}


@pytest.mark.parametrize("env", sorted(_SIZES))
def test_slot_bytes_and_the_fit_of_a_grown_batch_are_the_recorded_ones(env, monkeypatch):
    for name, value in env:
        monkeypatch.setenv(name, value)
    free = [0]
    monkeypatch.setattr(E, "_free_device_bytes", lambda: free[0])
    for n, kept, cap, needs in _SIZES[env]:
        assert E._kept_bytes_per_slot(n) == kept, n
        assert E.pool_slot_cap(n) == cap, n                                   # (no GPU here: a sixth of 16 GB)
        plain = 8 * (n + 34) + 72 * (n // 2 + 1) + 2600
        assert P.slot_bytes(n, False) == plain and P.slot_bytes(n, True) == plain + kept and P.slot_bytes(n) == plain + kept
        for (njobs, max_structs, cand, poollim, grow), need in zip(_FITS_CASES, needs):
            eng = E.HipEngine(max_structs=max_structs, cand_per_nt=cand)
            recs = [("A" * n, None, None, None, [PS] * njobs)]
            free[0] = need
            assert eng._fits_device(recs, None, {"poollim": poollim}, grow), (n, njobs, grow)
            free[0] = need - 1
            assert not eng._fits_device(recs, None, {"poollim": poollim}, grow), (n, njobs, grow)


def test_default_structure_slots():
    for njobs, want in ((0, 4096), (1024, 4096), (1025, 4100), (3000, 12000), (65536, 262144), (10 ** 6, 262144)):
        assert P.default_structs(njobs, 0) == want
        assert P.default_structs(njobs, 5000) == 5000


# ---- the switches -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,read", [("SQ_NO_POOL_KEPT", "no_pool_kept"), ("SQ_MUL_GATHER", "mul_gather"),
                                       ("SQ_NO_DETACH", "no_detach"), ("SQ_NO_PACKED_ROWS", "no_packed_rows")])
def test_presence_switches_are_on_whatever_their_value(name, read, monkeypatch):
    read = getattr(S, read)
    assert read() is False
    monkeypatch.setenv(name, "1")
    assert read() is True
    monkeypatch.setenv(name, "0")                                             # ("X" in os.environ: set is on)
    assert read() is True
    monkeypatch.delenv(name)
    assert read() is False                                                    # (read at every call)


def test_valued_switches_keep_their_defaults_and_clamps(monkeypatch):
    assert S.kept_pps() is None and S.dense_gb() == 32.0 and S.engine_sublanes() == 1 and S.engine_lanes() == 1
    for name in ("SQ_KEPT_PPS", "SQ_DENSE_GB", "SQ_ENGINE_SUBLANES", "SQ_ENGINE_LANES"):
        monkeypatch.setenv(name, "1")
    assert (S.kept_pps(), S.dense_gb(), S.engine_sublanes(), S.engine_lanes()) == (1.0, 1.0, 1, 1)
    monkeypatch.setenv("SQ_KEPT_PPS", "0.1")                                  # (no floor on the Python side)
    monkeypatch.setenv("SQ_DENSE_GB", "0.5")
    monkeypatch.setenv("SQ_ENGINE_SUBLANES", "0")                             # max(1, ...)
    monkeypatch.setenv("SQ_ENGINE_LANES", "0")                                # (as it is)
    assert (S.kept_pps(), S.dense_gb(), S.engine_sublanes(), S.engine_lanes()) == (0.1, 0.5, 1, 0)
    monkeypatch.setenv("SQ_ENGINE_SUBLANES", "2")
    monkeypatch.setenv("SQ_ENGINE_LANES", "2")
    assert (S.engine_sublanes(), S.engine_lanes()) == (2, 2)
    assert E._kept_bytes_per_slot(500) == int(2 * (0.1 * 6144 + 1028))
    monkeypatch.delenv("SQ_KEPT_PPS")
    assert S.kept_pps() is None and E._kept_bytes_per_slot(500) == 38920
