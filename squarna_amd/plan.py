"""How many structure slots a batch gets, what a slot costs, and how an input too big for the device pools is cut into
sub-batches.  Arithmetic only: torch is touched inside the two functions that ask the device for its free memory."""
import threading

import numpy as np

from . import switches


def _free_device_bytes():
    """Free device memory as a new workspace sees it: what the driver reports plus what torch's caching allocator holds without
    using it (the workspaces of earlier batches: a call that sized its batches by the driver's figure alone got smaller ones
    than the call before it, whose workspace it could have had back)."""
    import torch
    return int(torch.cuda.mem_get_info()[0]) + max(0, int(torch.cuda.memory_reserved()) - int(torch.cuda.memory_allocated()))


def _kept_bytes_per_slot(maxn):
    """Bytes per structure slot of the lists a pool's structures hand to their children (SQ_BATCH_POOL_LISTS, sequences of
    257-1,024 nt): SQ_KEPT_PPS pages of 6 KB per generation (default 3 at 500 nt, growing with the square of the length), a row
    of 256 page numbers, a count."""
    # (the library takes SQ_KEPT_PPS as "else at least 0.25", csrc/sq_switches.h; this estimate takes any value as it is)
    if not 256 < maxn <= 1024 or switches.no_pool_kept():
        return 0
    pps = switches.kept_pps()
    if pps is None:
        pps = max(1.0, 3.0 * (maxn / 500.0) ** 2)
    return int(2 * (pps * 6144 + 1028))


def slot_bytes(n, pool_lists=True):
    """Device bytes of one structure slot of a batch of sequences up to n nt: ~56 bytes per nucleotide of the device pools
    (sq_pool.hip), and with pool_lists the pages of the kept lists."""
    return 8 * (n + 34) + 72 * (n // 2 + 1) + 2600 + (_kept_bytes_per_slot(n) if pool_lists else 0)


def default_structs(njobs, max_structs=0):
    """Structure slots of a batch of njobs (sequence, paramset) jobs unless the caller fixed them: the device-side pools /
    chained rounds hold every structure of a round at once, so the default grows with the number of jobs."""
    return max_structs if max_structs else max(4096, min(4 * njobs, 262144))


def workspace_size_class(want):
    """Bytes of the workspace tensor of a batch that needs `want` bytes: the next multiple of the size class's step."""
    # (sizes in coarse steps: batches of a stream differ by a few records, and torch's caching allocator only hands a cached
    # block back for a request it nearly fits -- every new size was a hipMalloc, the occasional one with a device-wide
    # free of cached blocks in front: 40-190 ms steps in the stream leg)
    # (sixteen size classes per octave from 256 MB on: the 6 GB workspaces of a stream's batches -- 12 SRtest150 sets each --
    # differ by a few per cent, which in 64 MB steps was a new size every other step: torch's reserved memory grew from 95
    # to 173 GB over fourteen steps of the pipelined stream, and a step paid hundreds of ms for the device-wide free)
    step = (1 << (want.bit_length() - 5)) if want >= (256 << 20) else (8 << 20) if want >= (16 << 20) else (1 << 20)
    return (want + step - 1) // step * step


#: candidate records per nucleotide a structure gets at least (32 bytes each) when a fold is repeated with more room
MIN_CAND_PER_NT = 32


def pool_slot_cap(maxn, want=None):
    """Most structure slots a batch of sequences up to maxn nt should get: a slot of the device pools (sq_pool.hip) costs
    ~56 bytes per nucleotide; all slots stay within a sixth of the free device memory (at most 2 Mi).
    want: the slots the caller is about to ask for -- when the driver's figure alone grants them, the allocator's idle blocks are
    not counted (torch.cuda.memory_reserved() walks the allocator's statistics: 0.25 ms of a 5-ms Predict() on SRtest150)."""
    import torch
    per_slot = slot_bytes(maxn)
    if not torch.cuda.is_available():
        return int(max(4096, min((16 << 30) // 6 // per_slot, 2 << 20)))
    cap = int(max(4096, min(int(torch.cuda.mem_get_info()[0]) // 6 // per_slot, 2 << 20)))
    if want is not None and want <= cap:
        return cap
    return int(max(4096, min(_free_device_bytes() // 6 // per_slot, 2 << 20)))


def pool_slots_wanted(ngreedy, poollim, n=None):
    """Structure slots for `ngreedy` greedy jobs of an n-nt sequence under pools wider than 1: the device pools hold a
    whole generation of every job's pool.  A pool overshoots poollim before the stopper (SQRNdbnseq.py:1147) holds it (it
    grows by a factor of 1.5 to 3.5 per round), and a short sequence never fills it: measured on random sequences the
    generations peak at ~1.75e-5 n^3 structures per job (6 at 20-120 nt, 485 at 300 nt) until poollim bounds them (130
    at 1000 nt under poollim 100).  Twice that, and at least 16."""
    p = min(int(poollim), 1024)
    per_job = min(3 * p, p + 512)
    if n is not None:
        per_job = min(per_job, max(16, int(4e-5 * float(n) ** 3)))
    return int(ngreedy) * per_job


def _shared_weights(records):
    """The records are an alignment's rows weighted by ONE device matrix (alignment step 2)."""
    sm0 = records[0][5] if records and len(records[0]) > 5 else None
    return sm0 is not None and hasattr(sm0, "is_cuda") and sm0.is_cuda and all(len(r) > 5 and r[5] is sm0 for r in records)


def pool_slots_wanted_many(lengths, psets_per_record, poollim, rarely_branch=False):
    """pool_slots_wanted for every record of a batch (numpy array): the greedy-job count per distinct paramset list is
    counted once (the records of an input usually share one list), the per-length part is vectorised.
    rarely_branch: the rows of an alignment under paramsets whose range factor is 1.0 -- their pools branch only at exact
    ties that share a base (SQRNdbnseq.py:769-789), the weights of a stem matrix make those rare, and the library folds such
    jobs as chains first (sq_fold.hip): sixteen slots per job (a fold that outgrows them is repeated by the host loop)."""
    if rarely_branch and all(ps["suboptmin"] == 1.0 and ps["suboptmax"] == 1.0 for pl in {id(p): p for p in psets_per_record}.values()
                             for ps in pl if "G" in ps["algorithms"]):
        return np.array([16 * sum(1 for ps in pl if "G" in ps["algorithms"]) for pl in psets_per_record], np.int64)
    ng_of, ng = {}, np.empty(len(psets_per_record), np.int64)
    for k, pl in enumerate(psets_per_record):
        v = ng_of.get(id(pl))
        if v is None:
            v = ng_of[id(pl)] = sum(1 for ps in pl if "G" in ps["algorithms"])
        ng[k] = v
    p = min(int(poollim), 1024)
    n = np.asarray(lengths, np.float64)
    per_job = np.minimum(min(3 * p, p + 512), np.maximum(16, (4e-5 * n ** 3).astype(np.int64)))
    return ng * per_job


class SubBatchPlan:
    """Cuts records into consecutive sub-batches sized to the device-pool slots (`cap`; per_rec: the slots every record's pools
    may want) and to the dense per-job matrices a sub-batch may hold (dense: bytes per record).  What the pools of the first
    sub-batch really reached scales the estimate for the rest (a fold weighted by an alignment's stem matrix keeps one or two
    structures per job).  take() and report() may be called from `lanes` threads, each with its share of the slots."""

    def __init__(self, per_rec, dense, cap, dense_cap, lanes=1, scale=1.0):
        self.per_rec, self.per_arr, self.dense, self.scale = per_rec, np.asarray(per_rec, np.float64), dense, scale
        if sum(dense) > dense_cap:
            # sub-batches of equal weight (a last one of a few records would run its rounds on a mostly empty chip)
            dense_cap = sum(dense) / np.ceil(sum(dense) / dense_cap) + max(dense)
        self.dense_cap = dense_cap
        self.cap = cap // lanes if lanes > 1 else cap
        self.lo, self.first, self.error, self.driver, self.peak, self.reported = 0, True, None, 0, 0, False
        self.lock = threading.Lock()

    def take(self):
        """(lo, hi, slots hint) of the next sub-batch; None when no record is left or a sub-batch has failed."""
        with self.lock:
            n, lo, per, arr = len(self.per_rec), self.lo, self.per_rec, self.per_arr
            if self.error is not None or lo >= n:
                return None
            # (sub-batches of equal weight: what is left goes into as few batches as the slots allow, each with the same share --
            # a full one and a remainder of a fifth left the remainder its own wait for the Edmonds graphs on a mostly empty chip)
            left = float(np.maximum(16.0, arr[lo:] * self.scale).sum())
            cap = self.cap
            if left > cap:
                cap = min(cap, left / np.ceil(left / cap) + float(arr[lo:].max()) * self.scale + 16.0)
            hi, g, gb = lo, 0.0, 0.0
            while hi < n and (hi == lo or (g + max(16.0, per[hi] * self.scale) <= cap and gb + self.dense[hi] <= self.dense_cap)):
                g += max(16.0, per[hi] * self.scale)
                gb += self.dense[hi]
                hi += 1
            self.lo = hi
            return lo, hi, int(g)

    def report(self, lo, hi, driver, peak):
        """What the fold of records lo..hi reached: its driver (2 device pools, 3 device pools repeated by the host loop) and
        the most structures a round of it held."""
        with self.lock:
            self.driver, self.peak, self.reported = max(self.driver, driver), max(self.peak, peak), True
            if self.first and peak > 0 and driver == 2:
                self.scale = min(self.scale, max(2.0 * peak / max(sum(self.per_rec[lo:hi]), 1), 1e-4))
                self.first = False
            elif driver == 3:
                self.scale = min(1.0, self.scale * 4)

    def fail(self, error):
        """A sub-batch raised: the first error is kept, no further sub-batch is handed out."""
        with self.lock:
            if self.error is None:
                self.error = error
