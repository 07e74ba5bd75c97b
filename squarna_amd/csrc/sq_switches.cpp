// sq_switches.cpp -- every read of an SQ_* environment variable (sq_switches.h: the three moments).
#include "sq_host_int.h"

namespace {
bool on(const char *name) { return getenv(name) != nullptr; }
int num(const char *name, int lo, int hi, int dflt)
{
    const char *e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : dflt;
}
int raw(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
long raw_l(const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; }
// threads in whole waves: the value rounded down to a multiple of 64, within [lo, hi]
int waves(const char *name, int lo, int hi, int dflt)
{
    const char *e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e) / 64 * 64)) : dflt;
}
}  // namespace

// SQ_CPUACC: read when the library is loaded (every CpuScope tests it)
bool g_cpuacc_on = getenv("SQ_CPUACC") != nullptr;

void sq_read_fold_switches(SqFoldSwitches &sw)
{
    sw.timing = on("SQ_TIMING"); sw.pool_debug = on("SQ_POOL_DEBUG");
    sw.no_chain = on("SQ_NO_CHAIN"); sw.no_rounds = on("SQ_NO_ROUNDS"); sw.no_pool = on("SQ_NO_POOL");
    sw.no_opt_chain = on("SQ_NO_OPT_CHAIN"); sw.no_fly_bits = on("SQ_NO_FLY_BITS"); sw.no_defer_wait = on("SQ_NO_DEFER_WAIT");
    sw.no_pool_round = on("SQ_NO_POOL_ROUND");
    sw.pool_round_nsurv = num("SQ_POOL_ROUND_NSURV", 16, 2048, 0);
    sw.pool_root = num("SQ_POOL_ROOT", 0, 1, 0);
    sw.no_pool_kept = on("SQ_NO_POOL_KEPT");
    sw.pool_ahead = num("SQ_POOL_AHEAD", 0, SQ_POOL_HDR_RING - 2, 3);
    sw.pool_slots = num("SQ_POOL_SLOTS", 1, 0x7fffffff, 0); sw.pool_chunk = num("SQ_POOL_CHUNK", 1, 0x7fffffff, 0);
    sw.no_score_bound = on("SQ_NO_SCORE_BOUND"); sw.no_score_context = on("SQ_NO_SCORE_CONTEXT");
    sw.no_edges_lds = on("SQ_NO_EDGES_LDS");
    sw.no_device_algos = on("SQ_NO_DEVICE_ALGOS"); sw.no_device_tail = on("SQ_NO_DEVICE_TAIL");
    sw.algo_sync = on("SQ_ALGO_SYNC"); sw.lsap_classes = num("SQ_LSAP_CLASSES", 1, 64, 0);
    sw.mwm_dump = on("SQ_MWM_DUMP"); sw.mwm_posthoc = on("SQ_MWM_POSTHOC");
    sw.rounds_tlds = num("SQ_ROUNDS_TLDS", 1, 0x7fffffff, 0);
    sw.wave_walk_min = raw("SQ_WAVE_WALK_MIN", 192); sw.wave_walk_lanes = raw("SQ_WAVE_WALK_LANES", 12);
    sw.no_early_walk = on("SQ_NO_EARLY_WALK");
    sw.score_pool_threads = waves("SQ_SCORE_POOL_THREADS", 64, 1024, 128);
}

void sq_read_batch_switches(SqBatchSwitches &sw)
{
    sw.ld_pow2 = on("SQ_LD_POW2"); sw.mul_gather = on("SQ_MUL_GATHER");
    sw.out_cap = num("SQ_OUT_CAP", 64, 0x7fffffff, 0);
    sw.ctx_min_n = raw("SQ_CTX_MIN_N", 800);
    sw.no_pool_kept = on("SQ_NO_POOL_KEPT");
    sw.kept_pps = getenv("SQ_KEPT_PPS") ? std::max(0.25, atof(getenv("SQ_KEPT_PPS"))) : 0.0;
    sw.kept_gb = getenv("SQ_KEPT_GB") ? std::max(0.01, atof(getenv("SQ_KEPT_GB"))) : 48.0;
    sw.fin_stem_cap = num("SQ_FIN_STEM_CAP", 16, 0x7fffffff, 0);
    sw.no_shared_bits = on("SQ_NO_SHARED_BITS"); sw.bits_direct = on("SQ_BITS_DIRECT");
    sw.host_threads = num("SQ_HOST_THREADS", 1, 0x7fffffff, 0);
}

const SqTuning &sq_tuning()
{
    static const SqTuning t = [] {
        SqTuning t;
        t.cpus = num("SQ_CPUS", 1, 0x7fffffff, 0);
        t.relax = raw("SQ_RELAX", -1);
        t.pinned_trace = on("SQ_PINNED_TRACE"); t.pinned_cache_mb = num("SQ_PINNED_CACHE_MB", 0, 0x7fffffff, 6144);
        t.fold_lanes = raw("SQ_FOLD_LANES", 2); t.lane_min_jobs = raw("SQ_LANE_MIN_JOBS", 512);
        t.grow_par = getenv("SQ_GROW_PAR") ? (size_t)atol(getenv("SQ_GROW_PAR")) : 1024;
        t.rounds_threads = waves("SQ_ROUNDS_THREADS", 64, SQ_ROUNDS_THREADS, 0);
        t.fly_min_n = raw("SQ_FLY_MIN_N", 0);
        t.chain_depth = (uint32_t)num("SQ_CHAIN_DEPTH", 1, 0x7fffffff, 3);
        t.pool_extend_waves = num("SQ_POOL_EXTEND_WAVES", 1, 16, 1);
        t.fill_per = raw("SQ_FILL_PER", 0);
        t.bits_nomasks = on("SQ_BITS_NOMASKS");
        t.no_state_scan_fuse = on("SQ_NO_STATE_SCAN_FUSE");
        t.state_short_threads = waves("SQ_STATE_SHORT_THREADS", 64, 256, 64);
        t.state_short_set = raw("SQ_STATE_SHORT_THREADS", 64) != 64;
        t.scan_short_waves = num("SQ_SCAN_SHORT_WAVES", 1, 0x7fffffff, 1);
        t.scan_short_set = raw("SQ_SCAN_SHORT_WAVES", 1) != 1;
        t.no_state_copy = on("SQ_NO_STATE_COPY");
        t.score_nr_lim = raw("SQ_SCORE_NR_LIM", 4096);
        t.score_state_lim = getenv("SQ_SCORE_STATE_LIM") ? (size_t)atol(getenv("SQ_SCORE_STATE_LIM")) : 24 * 1024;
        t.score_threads = raw("SQ_SCORE_THREADS", 0); t.score_parts = raw("SQ_SCORE_PARTS", 0);
        t.score_target = raw("SQ_SCORE_TARGET", 512); t.score_short_threads = raw("SQ_SCORE_SHORT_THREADS", 64);
        t.pool_short_nsurv = num("SQ_POOL_SHORT_NSURV", 64, 1024, 384);
        t.align_sequential = on("SQ_ALIGN_SEQUENTIAL");
        t.side_streams = raw("SQ_SIDE_STREAMS", 0);
        t.mwm_classes = num("SQ_MWM_CLASSES", 1, 0x7fffffff, 0);
        t.mwm_verify = on("SQ_MWM_VERIFY"); t.no_algo_raw = on("SQ_NO_ALGO_RAW");
        t.mwm_bin_waves = raw("SQ_MWM_BIN_WAVES", 0);
        t.mwm_bin_bytes = raw_l("SQ_MWM_BIN_BYTES", 0); t.mwm_all_cap = raw_l("SQ_MWM_ALL_CAP", 0);
        t.mwm_nolds = on("SQ_MWM_NOLDS");
        t.nuss_threads = waves("SQ_NUSS_THREADS", 64, 256, 0);
        return t;
    }();
    return t;
}
