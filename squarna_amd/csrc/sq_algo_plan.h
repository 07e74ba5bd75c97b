// sq_algo_plan.h -- the plan of one chunk of matching work (Edmonds / Hungarian / Nussinov jobs that share a device region, a
// pinned staging buffer and a sequence of launches): what a job needs, which jobs fit the region, the layouts of region and
// staging buffer ("the plan of a matching chunk"), the order and size classes of the launches, the blossom kernel's
// LDS bins.  Host only: no HIP, no environment -- sq_algos.hip, sq_graph.hip and sq_launch_matching allocate, copy and launch
// by it, and tests/native/algo_plan_host.cpp compiles it with a plain C++ compiler.
#pragma once
#include <algorithm>
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../include/squarna_hip.h"
#include "sq_match.h"
#include "sq_blossom.h"

// The switches the plan honours, handed in by the caller; 0 / false: decided by the launch.
struct SqAlgoKnobs {              // SQ_MWM_CLASSES, SQ_LSAP_CLASSES, SQ_MWM_BIN_WAVES, SQ_MWM_BIN_BYTES, SQ_MWM_ALL_CAP, SQ_MWM_NOLDS, SQ_NUSS_THREADS
    int mwm_classes = 0, lsap_classes = 0, mwm_bin_waves = 0;
    long mwm_bin_bytes = 0, mwm_all_cap = 0;
    bool mwm_nolds = false;
    int nuss_threads = 0;
};
SqAlgoKnobs sq_algo_knobs(int lsap_classes);     // sq_match.hip: from sq_tuning() and the fold's SQ_LSAP_CLASSES

static inline size_t sq_up256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline size_t sq_mwm_scratch_bytes(int n, int nedges) { return SqBlossom::scratch_bytes(n, nedges); }
static inline size_t sq_blossom_hdr() { return (sizeof(SqBlossom) + 15) & ~(size_t)15; }   // the algorithm object in front of a graph's LDS slice

// ---- size of a job: n = sequence length (Hungarian, Nussinov) or graph vertices (Edmonds), ncell = cells of its stems = edges ----
struct SqAlgoJobSize {
    int n = 0;
    size_t ncell = 0, need = 0, nout = 0;   // need: global scratch, a multiple of 256; nout: result ints -- mates + first-assignment ranks
};                                           // + (passes, events) | col4row | pairs
static inline SqAlgoJobSize sq_algo_job_size(int algo, int n, size_t ncell)
{
    SqAlgoJobSize B;
    B.n = n; B.ncell = ncell;
    if (algo == SQ_ALGO_E) { B.need = sq_mwm_scratch_bytes(n, (int)ncell); B.nout = 2 * (size_t)n + 2; }
    else if (algo == SQ_ALGO_H) { B.need = sq_lsap_scratch_bytes(n); B.nout = (size_t)n; }
    else { B.need = sq_nussinov_scratch_bytes(n); B.nout = 2 * ((size_t)n + 4); }
    B.need = sq_up256(B.need);
    return B;
}

// ---- the region of a chunk: [jobs][edges][out ints][counts]([vid2pos][stats][finish records])[scratch], every part on a
// 256-byte boundary; the parts in brackets exist in the device form only (RunAlgo on the device, sq_algos_dev.hip) ----
struct SqAlgoCarve { size_t o_jobs = 0, o_edges = 0, o_out = 0, o_cnt = 0, o_vid = 0, o_stat = 0, o_aj = 0, o_scr = 0, bytes = 0; };
static inline SqAlgoCarve sq_algo_carve(size_t nj, size_t nedges, size_t outints, size_t vids, size_t scratch, bool dev)
{
    SqAlgoCarve c;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = sq_up256(o + bytes); return at; };
    c.o_jobs = take(nj * sizeof(SqMatchJob));
    c.o_edges = take(nedges * sizeof(SqMatchEdge) + 16);
    c.o_out = take(outints * 4 + 16);
    c.o_cnt = take(nj * 4 + 16);
    if (dev) { c.o_vid = take(vids * 4 + 16); c.o_stat = take(sizeof(SqAlgoStat)); c.o_aj = take(nj * sizeof(SqAlgoJob) + 16); }
    c.o_scr = take(0);
    c.bytes = o + scratch;
    return c;
}

// The chunk cut admits a job while this CONSERVATIVE ESTIMATE of the region's fixed part (with that job) plus the scratch fits
// the region.  It bounds sq_algo_carve: the four host-form parts round up by at most 255 bytes each and three of them carry 16
// bytes of slack (4 x 255 + 48 = 1,068 <= 4,096); the device form adds vids x 4 + 16, 256 for the 64 bytes of statistics and
// nj records + 16, rounded up (16 + 255 + 256 + 16 + 255 = 798 <= 1,024), and counts the candidate's n as vertices under every
// algorithm.  The constants are part of which job ends a chunk.
static inline size_t sq_algo_cut_estimate(size_t nj, size_t nedges, size_t outints, size_t vids_n, bool dev)
{
    return nj * sizeof(SqMatchJob) + nedges * sizeof(SqMatchEdge) + (outints + nj) * 4 + 4096 +
           (dev ? vids_n * 4 + 1024 + nj * sizeof(SqAlgoJob) : 0);
}

// ---- the pinned staging buffer of a chunk: [jobs][edges][results][counts][completion word]([job flags][bin heads])
// ([job table in list order][finish records][statistics]); Edmonds alone has the flags and bin heads, the device form alone the
// tail -- and no edges, which its kernel writes into the region.  SQ_PLAN_NONE: the part does not exist. ----
static const size_t SQ_PLAN_NONE = ~(size_t)0;
struct SqAlgoStage {
    size_t jobs = 0, edges = 0, out = 0, cnt = 0, flag = 0, job_flags = SQ_PLAN_NONE, bin_head = SQ_PLAN_NONE;
    size_t p_mj = SQ_PLAN_NONE, p_aj = SQ_PLAN_NONE, h_stats = SQ_PLAN_NONE, bytes = 0;
};
static inline SqAlgoStage sq_algo_stage(int algo, size_t nj, size_t nedges, size_t outints, bool dev)
{
    SqAlgoStage s;
    size_t o = sq_up256(nj * sizeof(SqMatchJob));
    s.edges = o; o += dev ? 0 : sq_up256(nedges * sizeof(SqMatchEdge));
    s.out = o; o += sq_up256(outints * 4);
    s.cnt = o; o += sq_up256(nj * 4);
    s.flag = o; o += 256;
    if (algo == SQ_ALGO_E) { s.job_flags = o; o += sq_up256(nj * 4); s.bin_head = o; o += sq_up256(nj * 4); }
    if (dev) {
        s.p_mj = o; o += sq_up256(nj * sizeof(SqMatchJob));
        s.p_aj = o; o += sq_up256(nj * sizeof(SqAlgoJob));
        s.h_stats = o; o += 256;
    }
    s.bytes = o;
    return s;
}

// ---- crowd predicates ----
// the chip is crowded for a chunk's short kernels: batches in flight, or thousands of jobs
// (a batch of 1,314 jobs alone: 7.1 ms without the Hungarian classes, 8.5 with)
static inline bool sq_algo_crowded(int inflight, size_t njobs) { return inflight > 1 || njobs >= 4096; }
// A blossom launch (or the launches in flight together) with more graphs than the chip has room for at one graph per CU is a
// throughput problem: every graph keeps only the hot part of its state in LDS (~4 KB; the rest in its global scratch,
// +14 % time per graph) and a block holds four of them in 40 KB, so that ALL graphs are resident at once -- the kernel
// then lasts as long as its slowest graph -- and the scoring kernels of the greedy rounds still find LDS on every CU.
// Measured on 24 SRtest150 sets in one batch (4,296 graphs): 11.5 ms with 150 KB bins, 6.6 ms this way.
// ... and so is a launch of hundreds of LARGE graphs (hot part beyond a crowd's 40 KB bin: 500 vertices and 17,000 edges take
// 50 KB) beside the rounds of the same batch's pools: 822 such graphs fill the LDS of every CU for 75 ms, during which the
// round kernel does not run (round 6: 1,000 records of 500 nt under pools of a thousand 313 -> 278 ms with the graphs' state
// in global memory; at 700 records the same either way, at 500 and fewer the longer Edmonds kernel is what the fold waits for)
static inline bool sq_mwm_crowd(const SqMatchJob *jobs, int nj, int inflight)
{
    size_t hot_max = 0;
    for (int q = 0; q < nj; q++) hot_max = std::max(hot_max, SqBlossom::hot_bytes(jobs[q].n, jobs[q].nedges, 2));
    return (long long)nj * std::max(1, inflight) >= 1024 || (nj >= 768 && hot_max + 16 + sq_blossom_hdr() > 40 * 1024);
}
// Threads of a Nussinov block: an anti-diagonal of the DP has at most n cells, no more waves than that keeps busy (the block
// holds its wave slots through the single-threaded BackTrack too); on a crowded chip ONE wave per job -- a block of three waves
// holds three wave slots through every barrier-separated diagonal, and wave slots are what a crowded chip runs out of (a lane
// then takes up to three cells of a diagonal).  The crowd rule is borrowed from the blossom plan, hot-part sizes included.
static inline int sq_nussinov_threads(const SqMatchJob *jobs, int nj, int maxn, int inflight, const SqAlgoKnobs &kn)
{
    if (kn.nuss_threads) return kn.nuss_threads;
    return sq_mwm_crowd(jobs, nj, inflight) ? 64 : std::max(64, std::min(256, (maxn + 63) / 64 * 64));
}

// ---- the dynamic LDS of one Hungarian launch ----
// Every block of a launch gets the same LDS, and every job must find room in it: the largest n and the largest m may belong
// to different jobs.  need: the most a job wants for form a (sq_lsap.h); lds: what the launch gets -- that, or when it is
// beyond a block's share of a CU, room for the vectors of the largest job alone (forms b, c).  Each job then takes the form
// sq_lsap_form(n, m, lds) gives it.
static const size_t SQ_LSAP_LDS_CAP = 150 * 1024;
struct SqLsapLds { size_t need = 0, lds = 0; };
static inline SqLsapLds sq_lsap_launch_lds(const SqMatchJob *h_jobs, int nj)
{
    SqLsapLds P;
    int maxn = 0;
    for (int q = 0; q < nj; q++) {
        P.need = std::max(P.need, sq_lsap_lds_bytes(h_jobs[q].n, h_jobs[q].nedges));
        maxn = std::max(maxn, (int)h_jobs[q].n);
    }
    P.lds = P.need <= SQ_LSAP_LDS_CAP ? P.need : std::min(sq_lsap_vec_bytes(maxn) + 64, SQ_LSAP_LDS_CAP);
    return P;
}

// ---- launch order and size classes ----
// what a job's place in the launch order is decided by: the dynamic LDS it needs (Nussinov: the waves of its block)
static inline size_t sq_algo_lds_need(int algo, int n, int nedges)
{
    if (algo == SQ_ALGO_E) return SqBlossom::scratch_bytes(n, nedges, 1) + (((size_t)nedges * sizeof(SqMatchEdge) + 15) & ~(size_t)15) + 64;
    if (algo == SQ_ALGO_H) return sq_lsap_lds_bytes(n, nedges);
    return (size_t)std::max(1, (n + 63) / 64);
}
// Two classes for Edmonds folded alone (one-graph blocks, the critical class on its own stream; with batches in flight one
// launch, the graphs packed into multi-wave blocks -- sq_mwm_plan), one for Hungarian / Nussinov: classes that FOLLOW each other
// on a stream each last as long as their slowest job, so more of them lengthen the chain on the short kernels' stream past the
// end of Edmonds' class 0 (traced: 4 + 4 classes end at 9.3 ms, one batch alone, instead of 7.2 ms).  With the chip crowded
// three: every block of a Hungarian launch gets the LDS of the launch's LARGEST job (62 KB at 150 nt: two one-wave blocks per
// CU, and LDS the scoring kernels of the other batches do not get) -- three classes give most jobs a quarter of that; Nussinov
// gets blocks of 64 / 128 / 192 threads instead of 192 for every job.
static inline int sq_algo_max_classes(int algo, int inflight, size_t nq, const SqAlgoKnobs &kn)
{
    if (algo == SQ_ALGO_E) return kn.mwm_classes ? kn.mwm_classes : (inflight < 2 ? 2 : 1);
    return kn.lsap_classes ? kn.lsap_classes : (sq_algo_crowded(inflight, nq) ? 3 : 1);
}

struct SqAlgoClass { int start, count; };         // rows [start, start + count) of the sorted table: one launch

// ---- the plan of a chunk ----
struct SqAlgoPlan {
    std::vector<SqMatchJob> mj;                  // the admitted jobs in list order (pos_off: the caller's)
    size_t nedges = 0, vids = 0;                 // vids: graph vertices of all Edmonds jobs
    size_t outints = 0, scratch = 0;
    SqAlgoCarve carve;                           // carve.bytes: device bytes used from the region's base
    SqAlgoStage stage;
    // Edmonds / Hungarian: the kernel's job table is sorted by LDS need (largest first) and launched in size classes,
    // every class with the dynamic LDS of ITS largest job.  A launch-wide LDS size gives each of the 219 SRtest150
    // graphs the 130 KB of the largest one: one block per CU, so two batches in flight already hold every CU's LDS and
    // the 56 KB blocks of the scoring kernel of ALL batches wait for a blossom block to finish (traced on MI355X with 8
    // batches in flight: sq_score_kernel 31 -> 137 us, sq_bps_kernel 33 -> 783 us per launch, profiles/r02j_*).
    std::vector<size_t> need;                    // sq_algo_lds_need per job
    std::vector<int> sorted_pos;                 // job q of mj -> row of the sorted table
    std::vector<SqMatchJob> sorted;              // the sorted table (pad: the job's index -- the Nussinov kernel files its pair count under it)
    std::vector<SqAlgoClass> classes;
};

// Jobs jb[0, nj) in order, as many as fit region_bytes: the cut, the two layouts, the launch order and its classes.
static inline void sq_algo_plan_chunk(int algo, const SqAlgoJobSize *jb, size_t nj, size_t region_bytes, bool dev, int inflight,
                                      const SqAlgoKnobs &kn, SqAlgoPlan &P)
{
    std::vector<SqMatchJob> &mj = P.mj;
    mj.clear();
    size_t scratch = 0, outints = 0, nedges = 0, vids = 0;
    for (size_t k = 0; k < nj; k++) {
        const SqAlgoJobSize &B = jb[k];
        const size_t fixed = sq_algo_cut_estimate(mj.size() + 1, nedges + B.ncell, outints + B.nout, vids + (size_t)B.n, dev);
        if (fixed + scratch + B.need > region_bytes) break;
        SqMatchJob m = SqMatchJob();
        m.n = B.n; m.nedges = (int32_t)B.ncell;
        m.edge_off = (int64_t)nedges; m.pos_off = 0;
        m.scratch_off = (int64_t)scratch; scratch += B.need;
        m.out_off = (int64_t)(algo == SQ_ALGO_N ? outints / 2 : outints); outints += B.nout;
        nedges += B.ncell;
        if (algo == SQ_ALGO_E) vids += (size_t)B.n;
        mj.push_back(m);
    }
    const size_t nq = mj.size();
    P.outints = outints; P.scratch = scratch; P.nedges = nedges; P.vids = vids;
    P.carve = sq_algo_carve(nq, nedges, outints, vids, scratch, dev);
    assert(nq == 0 || P.carve.bytes <= region_bytes);       // (sq_algo_cut_estimate)
    P.stage = sq_algo_stage(algo, nq, nedges, outints, dev);
    P.need.resize(nq); P.sorted.resize(nq); P.sorted_pos.resize(nq); P.classes.clear();
    if (!nq) return;
    for (size_t q = 0; q < nq; q++) P.need[q] = sq_algo_lds_need(algo, mj[q].n, mj[q].nedges);
    std::vector<int> ord(nq);
    for (size_t q = 0; q < nq; q++) ord[q] = (int)q;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return P.need[x] > P.need[y]; });
    for (size_t r = 0; r < nq; r++) { P.sorted[r] = mj[ord[r]]; P.sorted[r].pad = ord[r]; P.sorted_pos[ord[r]] = (int)r; }
    // a new class starts where twice as many blocks would fit a CU (and the current one has a few jobs)
    const int max_classes = sq_algo_max_classes(algo, inflight, nq, kn);
    size_t cur = std::min<size_t>(P.need[ord[0]], 150 * 1024);
    P.classes.push_back({0, 0});
    for (size_t r = 0; r < nq; r++) {
        SqAlgoClass &c = P.classes.back();
        if (c.count >= 4 && P.need[ord[r]] * 2 <= cur && (int)P.classes.size() < max_classes) {
            P.classes.push_back({(int)r, 1});
            cur = P.need[ord[r]];
        } else c.count++;
    }
}

// ---- the LDS bins of one blossom launch ----
// Packs the blossom graphs of one launch into bins (blocks) by LDS need, first fit in decreasing order.
//   * a graph gets its whole state + edge list in LDS when that is at most `all_cap`, else only the hot part (the rest in
//     its global scratch), else just the algorithm object (global-memory run);
//   * a bin holds at most `waves` graphs and `cap` bytes; with one batch in flight every graph has its own block (spread
//     over the CUs: latency), with several the bins fill up so that all batches' graphs are resident together and the
//     scoring kernels still find LDS (throughput): waves = ceil(graphs x inflight / 256), cap 150 KB -> 96 KB, all_cap
//     150 KB -> 48 KB from three batches in flight on; a crowd (sq_mwm_crowd): 4 waves, 40 KB, hot parts only.
//     SQ_MWM_BIN_WAVES / SQ_MWM_BIN_BYTES / SQ_MWM_ALL_CAP override.
// Writes lds_off / lds_bytes / next of jobs_rw (the table the kernel reads) and bin_head[0..nbins).
struct SqMwmPlan { int nbins = 0, waves = 1; size_t lds = 0, cap = 0; bool all_in_lds = true; };
static inline SqMwmPlan sq_mwm_plan(const SqMatchJob *h_jobs, SqMatchJob *jobs_rw, int nj, int32_t *bin_head, int inflight,
                                    const SqAlgoKnobs &kn, bool dump)
{
    SqMwmPlan P;
    const size_t hdr = sq_blossom_hdr();
    const bool many = inflight >= 3;
    const bool crowd = sq_mwm_crowd(h_jobs, nj, inflight);
    size_t cap = kn.mwm_bin_bytes > 0 ? (size_t)kn.mwm_bin_bytes : (crowd ? 40 * 1024 : many ? 96 * 1024 : 150 * 1024);
    cap = std::min<size_t>(cap, 150 * 1024);
    const size_t all_cap = kn.mwm_all_cap > 0 ? (size_t)kn.mwm_all_cap : (crowd ? 1 : many ? 48 * 1024 : 150 * 1024);
    int waves = kn.mwm_bin_waves > 0 ? kn.mwm_bin_waves : (crowd ? 4 : (int)(((long long)nj * std::max(1, inflight) + 255) / 256));
    waves = std::max(1, std::min(waves, 8));
    std::vector<size_t> need(nj);
    for (int q = 0; q < nj; q++) {
        const int n = h_jobs[q].n, m = h_jobs[q].nedges;
        const size_t full = SqBlossom::scratch_bytes(n, m, 1) + (((size_t)m * sizeof(SqMatchEdge) + 15) & ~(size_t)15) + 16;
        const size_t hot = SqBlossom::hot_bytes(n, m, 2) + 16;
        size_t take = hdr;
        if (n > 0 && !kn.mwm_nolds) {
            if (hdr + full <= std::min(all_cap, cap)) take = hdr + full;
            else if (hdr + hot <= cap) take = hdr + hot;
        }
        if (n > 0 && take != hdr + full) P.all_in_lds = false;
        need[q] = (take + 15) & ~(size_t)15;
    }
    std::vector<int> ord(nj);
    for (int q = 0; q < nj; q++) ord[q] = q;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return need[x] > need[y]; });
    std::vector<size_t> used; std::vector<int> cnt, tail;
    size_t lds = 0, first_open = 0;                      // bins before first_open are full (by count)
    for (int r = 0; r < nj; r++) {
        const int q = ord[r];
        size_t k = first_open;
        while (k < used.size() && (cnt[k] >= waves || used[k] + need[q] > cap)) k++;
        if (k == used.size()) { used.push_back(0); cnt.push_back(0); tail.push_back(-1); bin_head[k] = q; P.nbins++; }
        else jobs_rw[tail[k]].next = q;
        jobs_rw[q].lds_off = (int32_t)used[k]; jobs_rw[q].lds_bytes = (int32_t)need[q]; jobs_rw[q].next = -1;
        used[k] += need[q]; cnt[k]++; tail[k] = q;
        lds = std::max(lds, used[k]);
        while (first_open < used.size() && cnt[first_open] >= waves) first_open++;
    }
    P.waves = waves; P.cap = cap; P.lds = sq_up256(lds);
    if (dump) {
        size_t tot = 0; int nfull = 0;
        for (int q = 0; q < nj; q++) { tot += need[q]; nfull += need[q] > hdr + SqBlossom::hot_bytes(h_jobs[q].n, h_jobs[q].nedges, 2) + 32; }
        fprintf(stderr, "[mwm plan] %d graphs (inflight %d): %d bins of <= %d waves, %zu B of LDS per block, %zu B needed in all, %d graphs fully in LDS\n",
                nj, inflight, P.nbins, waves, P.lds, tot, nfull);
    }
    return P;
}
