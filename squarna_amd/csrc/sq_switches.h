// sq_switches.h -- the library's SQ_* environment switches (INTEGRATION.md section 5 documents each).  sq_switches.cpp is
// the only place that reads them, at one of three moments:
//   * per fold (SqFoldSwitches, sq_read_fold_switches at the start of every sq_fold): diagnostics and test hooks, none
//     changes results; tests flip them between two folds of one process;
//   * per batch (SqBatchSwitches, sq_read_batch_switches at sq_batch_workspace_bytes / sq_batch_create): switches that size
//     or shape a batch;
//   * once per process (SqTuning, sq_tuning() at its first call): tuning knobs of the launch shapes and the host's threads.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct SqFoldSwitches {
    bool timing = false;              // SQ_TIMING: phase timings on stderr
    bool pool_debug = false;          // SQ_POOL_DEBUG: pool sizes per round (with SQ_TIMING)
    bool no_chain = false;            // SQ_NO_CHAIN: poollim = 1 folds driven round by round from the host
    bool no_rounds = false;           // SQ_NO_ROUNDS: the launched rounds instead of the persistent round kernel
    bool no_pool = false;             // SQ_NO_POOL: pools booked on the host
    bool no_opt_chain = false;        // SQ_NO_OPT_CHAIN: pools with a range factor of 1.0 go to the device pools at once (no optimistic chains)
    bool no_fly_bits = false;         // SQ_NO_FLY_BITS: the bit matrices are always written (the round kernel's scan reads them)
    bool no_defer_wait = false;       // SQ_NO_DEFER_WAIT: the host waits for the round kernel before it enqueues the device tail
    bool no_pool_round = false;       // SQ_NO_POOL_ROUND: state / scan / score / choose / extend kernels instead of sq_pool_round_kernel
    int pool_round_nsurv = 0;         // SQ_POOL_ROUND_NSURV: survivors sq_pool_round_kernel keeps in LDS (0: by length)
    int pool_slots = 0;               // SQ_POOL_SLOTS: structure slots the device pools may use (0: max_structs)
    int pool_root = 0;                // SQ_POOL_ROOT: pools on sequences of 257-1,024 nt run the one-wave round kernel over root lists
    bool no_pool_kept = false;        // SQ_NO_POOL_KEPT: ... not over the lists their parents left (sq_device.h: SqKept)
    int pool_ahead = 3;               // SQ_POOL_AHEAD: rounds of the device pools a batch alone enqueues ahead of the host (0: none)
    int pool_chunk = 0;               // SQ_POOL_CHUNK: structures per chunk of a generation (0: what the arena holds)
    bool no_score_bound = false;      // SQ_NO_SCORE_BOUND: ScoreStems on every survivor of :492
    bool no_score_context = false;    // SQ_NO_SCORE_CONTEXT: the strand walk instead of the context tables (launched rounds)
    bool no_device_algos = false;     // SQ_NO_DEVICE_ALGOS: RunAlgo's edge lists and filters on the host
    bool no_edges_lds = false;        // SQ_NO_EDGES_LDS: the edges kernel ranks its stems in global memory (the form for lists beyond LDS)
    bool no_device_tail = false;      // SQ_NO_DEVICE_TAIL: the ranking tail on the host
    bool algo_sync = false;           // SQ_ALGO_SYNC: matching kernels on the batch stream
    int lsap_classes = 0;             // SQ_LSAP_CLASSES: size classes of the Hungarian / Nussinov launches (0: 3 crowded, else 1)
    bool mwm_dump = false;            // SQ_MWM_DUMP: the blossom graphs' sizes and LDS plan on stderr
    bool mwm_posthoc = false;         // SQ_MWM_POSTHOC: verification of streamed Edmonds results
    int rounds_tlds = 0;              // SQ_ROUNDS_TLDS: stems the persistent round kernel's LDS lists hold for pools that may branch (0: by the launch)
    int wave_walk_min = 192;          // SQ_WAVE_WALK_MIN: strands from which a wave takes over the last walks of a score step (<= 0: never)
    int wave_walk_lanes = 12;         // SQ_WAVE_WALK_LANES: ... once at most this many lanes are still walking
    bool no_early_walk = false;       // SQ_NO_EARLY_WALK: ScoreStems' walk never ends early at the order factor's bound
    int score_pool_threads = 128;     // SQ_SCORE_POOL_THREADS: score-kernel threads per structure of the pools' big generations beyond 200 nt
};
void sq_read_fold_switches(SqFoldSwitches &sw);

struct SqBatchSwitches {
    bool ld_pow2 = false;             // SQ_LD_POW2: fp32 row pitch without the odd-multiple-of-128-bytes padding
    bool mul_gather = false;          // SQ_MUL_GATHER: the rows of an alignment get their slices of the shared matrix materialised
    int out_cap = 0;                  // SQ_OUT_CAP: stems one round may emit (0: by the arena; else at least 64)
    int ctx_min_n = 800;              // SQ_CTX_MIN_N: longest sequence from which the batch carries the context tables (< 0: never)
    bool no_pool_kept = false;        // SQ_NO_POOL_KEPT: no pages are reserved for the pools' kept lists
    double kept_pps = 0;              // SQ_KEPT_PPS: pages of the kept lists per slot and generation (0: by length; else at least 0.25)
    double kept_gb = 48.0;            // SQ_KEPT_GB: upper limit of the kept lists' pages in all (at least 0.01)
    int fin_stem_cap = 0;             // SQ_FIN_STEM_CAP: caps the stem room of the log of final structures (0: none; else at least 16)
    bool no_shared_bits = false;      // SQ_NO_SHARED_BITS: every job gets its own diagonal bit matrix
    bool bits_direct = false;         // SQ_BITS_DIRECT: sq_bpmatrix_fill still writes the fp32 matrix (sq_fill_kernel) but takes the bit words from the O(N) inputs --
                                      // sq_bits_masks_kernel, or sq_bits_direct_kernel as below -- instead of from the matrix (sq_bits_kernel)
    int host_threads = 0;             // SQ_HOST_THREADS: size of the batch's worker pool (0: by the CPUs)
};
void sq_read_batch_switches(SqBatchSwitches &sw);

struct SqTuning {
    int cpus = 0;                     // SQ_CPUS: CPUs the process may use (0: affinity mask and cgroup quota)
    int relax = -1;                   // SQ_RELAX: wait loops spin (0) or sleep (1) (-1: by the batches in flight)
    bool pinned_trace = false;        // SQ_PINNED_TRACE: the pinned-buffer cache's trips to the driver on stderr
    int pinned_cache_mb = 6144;       // SQ_PINNED_CACHE_MB: idle pinned host buffers the cache keeps (at least 0)
    int fold_lanes = 2;               // SQ_FOLD_LANES: lanes of round buffers of a big host-driven fold
    int lane_min_jobs = 512;          // SQ_LANE_MIN_JOBS: greedy jobs from which a fold drives two lanes
    size_t grow_par = 1024;           // SQ_GROW_PAR: rounds with at least this many structures grow their pools on the worker pool
    int rounds_threads = 0;           // SQ_ROUNDS_THREADS: threads per block of the persistent round kernel (0: by the launch; else 64 .. SQ_ROUNDS_THREADS in waves)
    int fly_min_n = 0;                // SQ_FLY_MIN_N: shortest longest-sequence from which the round kernel forms its bit words itself
    uint32_t chain_depth = 3;         // SQ_CHAIN_DEPTH: chained rounds enqueued ahead of the device (at least 1)
    int pool_extend_waves = 1;        // SQ_POOL_EXTEND_WAVES: waves sharing a parent's children in the extend kernel on a crowded chip (1 .. 16)
    int fill_per = 0;                 // SQ_FILL_PER: 16-byte stores per thread of sq_fill_kernel's fast path (<= 0: by the launch)
    bool bits_nomasks = false;        // SQ_BITS_NOMASKS: sq_bits_direct_kernel (cell by cell) for every batch of the process in place of sq_bits_masks_kernel
                                      // (without the switch: interchainonly batches and mask tables beyond 60 KB of LDS)
    bool no_state_scan_fuse = false;  // SQ_NO_STATE_SCAN_FUSE: state and scan kernel as two launches on a crowded chip
    int state_short_threads = 64;     // SQ_STATE_SHORT_THREADS: state-kernel threads for sequences up to 200 nt on a crowded chip (64 .. 256 in waves)
    bool state_short_set = false;     // ... given with another value than 64 (then the state and scan kernels are not fused)
    int scan_short_waves = 1;         // SQ_SCAN_SHORT_WAVES: scan-kernel waves per structure for sequences up to 200 nt on a crowded chip (at least 1)
    bool scan_short_set = false;      // ... given with another value than 1 (then the state and scan kernels are not fused)
    bool no_state_copy = false;       // SQ_NO_STATE_COPY: per-structure / per-job records read from the pinned tables, not from device copies
    int score_nr_lim = 4096;          // SQ_SCORE_NR_LIM: longest sequence whose reactivities the score kernel stages in LDS
    size_t score_state_lim = 24 * 1024;   // SQ_SCORE_STATE_LIM: LDS bytes up to which it stages the partner / prefix arrays too
    int score_threads = 0;            // SQ_SCORE_THREADS: threads of a score block (0: by the launch)
    int score_parts = 0;              // SQ_SCORE_PARTS: blocks per structure of the score kernel (0: by the launch)
    int score_target = 512;           // SQ_SCORE_TARGET: blocks the score kernel's launch aims at
    int score_short_threads = 64;     // SQ_SCORE_SHORT_THREADS: score-kernel threads for sequences up to 200 nt on a crowded chip
    int pool_short_nsurv = 384;       // SQ_POOL_SHORT_NSURV: survivors the pools' choose kernel sorts in LDS up to 200 nt (64 .. 1,024)
    bool align_sequential = false;    // SQ_ALIGN_SEQUENTIAL: alignment step 1 adds one sequence per launch
    int side_streams = 0;             // SQ_SIDE_STREAMS: side streams of the matching kernels (0: by the batches in flight)
    int mwm_classes = 0;              // SQ_MWM_CLASSES: LDS size classes of one-graph blossom launches (0: by the launch; else at least 1)
    bool mwm_verify = false;          // SQ_MWM_VERIFY: every Edmonds job re-run on the host and compared
    bool no_algo_raw = false;         // SQ_NO_ALGO_RAW: E / H batches that need the host libm take the host-driven RunAlgo
    int mwm_bin_waves = 0;            // SQ_MWM_BIN_WAVES: graphs per blossom block (0: by the launch)
    long mwm_bin_bytes = 0;           // SQ_MWM_BIN_BYTES: LDS per blossom block (0: by the launch)
    long mwm_all_cap = 0;             // SQ_MWM_ALL_CAP: largest graph that keeps all its state in LDS (0: by the launch)
    bool mwm_nolds = false;           // SQ_MWM_NOLDS: blossom state in global memory for every graph
    int nuss_threads = 0;             // SQ_NUSS_THREADS: threads per block of the Nussinov kernel (0: by the launch; else 64 .. 256 in waves)
};
const SqTuning &sq_tuning();
