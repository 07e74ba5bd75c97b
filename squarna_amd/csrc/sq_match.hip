// sq_match.hip -- a-8 / a-9 / Nussinov on device: the matching step of RunAlgo
// (SQRNdbnseq.py:548-595) for the paramsets whose `algorithms` are H, E or N.
//
//   sq_lsap_kernel      Hungarian (SQRNalgos.py:113-135): scipy's linear_sum_assignment restated
//                       in sq_lsap.h, one wave per job.
//   sq_nussinov_kernel  Nussinov DP + BackTrack (SQRNalgos.py:6-93) in sq_nussinov.h: the DP by
//                       columns, one block per job, fp64, first-best-k tie rule.
//   sq_mwm_kernel       Edmonds (SQRNalgos.py:96-110): networkx 3.4.2 max_weight_matching
//                       restated in sq_blossom.h, one thread per job.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include "sq_match.h"
#include "sq_switches.h"
#include "sq_hostflag.h"
#include <vector>
#include <algorithm>
#include "sq_blossom.h"
#include "sq_algo_plan.h"

// ------------------------------------------------------------------------------------
// LSAP: one wave per job, the algorithm and the layout of the job's state in sq_lsap.h
// ------------------------------------------------------------------------------------
// the wave's barriers; with the vectors in global scratch (form c) lane 0's stores are released to the whole wave before the
// next step's cross-lane reads, not left to same-wave store-to-load ordering through L1
struct SqLsapBlockSync {
    __device__ void operator()() const { __syncthreads(); }
    __device__ void after_lane0(bool glob) const
    {
        if (glob) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        if (glob) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};

extern "C" __global__ __launch_bounds__(64) void sq_lsap_kernel(const SqMatchJob *jobs, const SqMatchEdge *edges,
                                                                char *scratch, int32_t *col4row_out, int lds_bytes)
{
    extern __shared__ __attribute__((aligned(16))) char lsap_lds[];
    const SqMatchJob jb = jobs[blockIdx.x];
    const int n = jb.n, m = jb.nedges, lane = threadIdx.x;
    if (n <= 0) return;
    const SqLsapForm form = sq_lsap_form(n, m, (size_t)lds_bytes);
    const SqLsapLayout L = sq_lsap_carve(scratch + jb.scratch_off, lsap_lds, form, n, m);
    sq_lsap_run<64>(L, form, n, m, edges + jb.edge_off, lane, SqLsapBlockSync(), SqCoopWave());
    for (int q = lane; q < n; q += 64) col4row_out[jb.out_off + q] = L.col4row[q];
}

// ------------------------------------------------------------------------------------
// Nussinov (SQRNalgos.py:44-93): one block per job, the algorithm and the layout of the job's scratch in sq_nussinov.h
// out: pairs (k, j) appended to pairs_out[out_off..], count in count_out[job]
// ------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void sq_nussinov_kernel(const SqMatchJob *jobs, const SqMatchEdge *edges,
                                                                     const uint8_t *codes, char *scratch,
                                                                     int32_t *pairs_out, int32_t *count_out, int by_pad)
{
    const SqMatchJob jb = jobs[blockIdx.x];
    const int n = jb.n, tid = threadIdx.x, nthr = blockDim.x;   // 64 .. 256 threads: the launch's longest sequence rounded up to waves
    // (by_pad: the rows are a slice of a table sorted by size, row.pad = the job's index, under which its count is filed)
    int32_t *const my_count = count_out + (by_pad ? jb.pad : (int)blockIdx.x);
    // (n == 1: the column DP writes no cell, BackTrack would read K[0, 0] from reused scratch; the reference returns no pairs)
    if (n < 2) { if (tid == 0) *my_count = 0; return; }
    sq_nussinov_run(sq_nuss_carve(scratch + jb.scratch_off, n, jb.nedges), n, jb.nedges, edges + jb.edge_off, codes + jb.pos_off,
                    pairs_out + 2 * (size_t)jb.out_off, my_count, tid, nthr, [] { __syncthreads(); }, SqCoopWave());
}

// ------------------------------------------------------------------------------------
// Edmonds: one thread per job runs the restated networkx blossom algorithm (sq_blossom.h)
// ------------------------------------------------------------------------------------
// One WAVE per graph, several graphs per block ("bin"): the host packs the graphs of a launch into bins by the LDS
// each one needs (sq_mwm_plan), the block's dynamic LDS is the bin capacity and every wave works in its own slice
// [lds_off, lds_off + lds_bytes) of it.  A launch-wide LDS size for one-graph blocks gives every graph the LDS of the
// largest one (SRtest150: 219 graphs, 8 MB of state in total, 29 MB when each gets 133 KB), and the LDS a blossom block
// holds is LDS the scoring kernels of the batches in flight cannot get.
// The waves of a bin never synchronise with each other: the "barrier" of the algorithm is a wave-local fence.
// job_flags (pinned host memory, may be null): job_flags[row] = stamp once the job's mates are in host memory, so the
// host can filter and rank a sequence while the larger graphs are still being matched.
// mate_out: per job 2n + 2 ints -- mate[0..n), the rank of every vertex's first mate assignment (SqBlossom::mord), then
// the run's scan passes and lane-0 events (measurement: the critical path of the kernel is passes x cycles per pass)
// one graph on one wave: bl (the algorithm object) and wlds (lds_bytes of state room) are the wave's LDS, sync its barrier
template <class Sync>
__device__ __forceinline__ void sq_mwm_one(SqBlossom &bl, char *lds_base, char *wlds, size_t lds_bytes, const SqMatchJob *jp, int row,
                                           const SqMatchEdge *edges, char *scratch, int32_t *mate_out, uint32_t *job_flags,
                                           uint32_t stamp, int lane, Sync wsync)
{
    // The job's flag tells the host that its result block in pinned memory is complete.  A system-scope fence between the
    // data stores and the flag store is NOT enough on this platform: both are posted writes on the way to host memory and
    // the later one was seen to overtake the earlier ones (about one job in 10^5: the collector read a result block that
    // was still arriving -- found by tools/fuzz_options.py, shown by SQ_MWM_POSTHOC=1).  A READ from the same memory
    // cannot pass the posted writes ahead of it, so every lane reads back a word of the block before the flag goes out.
    auto publish = [&]() {
        if (job_flags) {
            const int nw = jp->n > 0 ? 2 * jp->n + 2 : 2;
            sq_host_write_flush(mate_out + jp->out_off + (lane < nw ? nw - 1 - lane : 0));
        }
        // (without per-job flags nobody reads the mates before the kernel has ended -- the finish kernel or the flag kernel
        // behind it on the stream: no fence here; a system-scope fence per graph writes the L2 back, thousands of times a launch)
        wsync();
        if (job_flags && lane == 0) job_flags[row] = stamp;
    };
    const int n = jp->n, m = jp->nedges;
    if (n <= 0) { if (lane == 0) { mate_out[jp->out_off] = 0; mate_out[jp->out_off + 1] = 0; } publish(); return; }
    // The algorithm is a long chain of dependent loads: keep its state in LDS -- all of it with the edge list when
    // the slice holds that (tight capacities), else only the hot part (what every scan pass touches; blossom structure
    // and adjacency stay in global memory); on a capacity overflow rerun the job in global memory.
#ifdef SQ_MWM_PROF
    const long long _c0 = clock64(), _w0 = wall_clock64();
#endif
    const size_t ebytes = ((size_t)m * sizeof(SqMatchEdge) + 15) & ~(size_t)15;
    char *gscratch = scratch + jp->scratch_off;
    const bool all_lds = SqBlossom::scratch_bytes(n, m, 1) + ebytes + 16 <= lds_bytes;
    const bool hot_lds = !all_lds && SqBlossom::hot_bytes(n, m, 2) + 16 <= lds_bytes;
    if (all_lds) {
        SqMatchEdge *le = reinterpret_cast<SqMatchEdge *>(wlds);
        for (int e = lane; e < m; e += 64) le[e] = edges[jp->edge_off + e];
        wsync();
#ifdef SQ_MWM_PROF
        const long long _w1 = wall_clock64();
#endif
        if (lane == 0) { bl.init(n, m, le, wlds + ebytes, 1, false); bl.origin = lds_base; }
        wsync();
#ifdef SQ_MWM_PROF
        const long long _w2 = wall_clock64();
#endif
        bl.template build_csr<1>(lane, 64, wsync, SqCoopWave());
#ifdef SQ_MWM_PROF
        const long long _w3 = wall_clock64();
#endif
        bl.template run<1>(lane, 64, wsync, SqCoopWave(), lds_base);
#ifdef SQ_MWM_PROF
        if (lane == 0 && n >= 140) printf("mwm outside: edge load %.0f us, init %.0f, csr %.0f, run %.0f\n", (_w1 - _w0) * 0.01, (_w2 - _w1) * 0.01, (_w3 - _w2) * 0.01, (wall_clock64() - _w3) * 0.01);
#endif
    } else if (hot_lds) {
        if (lane == 0) {
            char *cold = gscratch;
            bl.init(n, m, edges + jp->edge_off, wlds, 2, false, cold, cold + ((SqBlossom::cold_bytes(n, m, 2) + 15) & ~(size_t)15));
            bl.origin = lds_base;
        }
        wsync();
        bl.template build_csr<2>(lane, 64, wsync, SqCoopWave());
        bl.template run<2>(lane, 64, wsync, SqCoopWave(), lds_base);
    }
    if (all_lds || hot_lds) {
        wsync();
        if (!bl.error) {
            for (int q = lane; q < n; q += 64) { mate_out[jp->out_off + q] = bl.mate[q]; mate_out[jp->out_off + n + q] = bl.mord[q]; }
            if (lane == 0) { mate_out[jp->out_off + 2 * n] = bl.stat_pass; mate_out[jp->out_off + 2 * n + 1] = bl.stat_event; }
#ifdef SQ_MWM_PROF
            if (lane == 0 && n >= 140) {
                const long long dc = clock64() - _c0, dw = wall_clock64() - _w0;
                printf("mwm clock: %lld shader cycles in %.0f us -> %.0f MHz\n", dc, dw * 0.01, (double)dc / (dw * 0.01));
            }
#endif
            publish();
            return;
        }
        wsync();
    }
    if (lane == 0) bl.init(n, m, edges + jp->edge_off, gscratch, 0, false);
    wsync();
    bl.template build_csr<0>(lane, 64, wsync, SqCoopWave());
    // lane 0 runs the order-dependent part; all 64 lanes share the O(n) sweeps of every substage
    bl.template run<0>(lane, 64, wsync, SqCoopWave(), nullptr);
    wsync();
    for (int q = lane; q < n; q += 64) { mate_out[jp->out_off + q] = bl.error ? -2 : bl.mate[q]; mate_out[jp->out_off + n + q] = bl.mord[q]; }
    if (lane == 0) { mate_out[jp->out_off + 2 * n] = bl.stat_pass; mate_out[jp->out_off + 2 * n + 1] = bl.stat_event; }
    publish();
}

// several graphs per block (one per wave), each in its slice of the block's dynamic LDS
// (second launch bound: four waves per SIMD, i.e. at most 128 VGPRs -- the compiler otherwise takes the 248 a 512-thread block
// may have and two graphs per SIMD fill the register file; 24 SRtest150 sets in one batch: Edmonds 16.9 -> 13.0 ms)
extern "C" __global__ __launch_bounds__(512, 4) void sq_mwm_kernel(const SqMatchJob *jobs, const int32_t *bin_head,
                                                                const SqMatchEdge *edges, char *scratch, int32_t *mate_out,
                                                                uint32_t *job_flags, uint32_t stamp)
{
    extern __shared__ __attribute__((aligned(16))) char mwm_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int row = bin_head[blockIdx.x];
    for (int k = 0; k < wave && row >= 0; k++) row = jobs[row].next;
    if (row < 0) return;                                  // this bin holds fewer graphs than the block has waves
    // all lanes of a wave run in lockstep; the fence keeps the compiler (and the memory pipeline) from moving accesses
    // of one lane across the point where another lane's data is needed
    auto wsync = [] { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); };
    const SqMatchJob *jp = jobs + row;
    // the wave's slice: the algorithm object (shared by the lanes), then the state
    const size_t hdr = (sizeof(SqBlossom) + 15) & ~(size_t)15;
    SqBlossom &bl = *reinterpret_cast<SqBlossom *>(mwm_lds + jp->lds_off);
    const size_t lds_bytes = (size_t)jp->lds_bytes > hdr ? (size_t)jp->lds_bytes - hdr : 0;
    sq_mwm_one(bl, mwm_lds, mwm_lds + jp->lds_off + hdr, lds_bytes, jp, row, edges, scratch, mate_out, job_flags, stamp, lane, wsync);
}

// one graph per block (one batch alone: every graph on its own CU): the algorithm object at a fixed LDS address, the
// block barrier as the wave's barrier; the block's dynamic LDS is the graph's (rows = blocks)
extern "C" __global__ __launch_bounds__(64) void sq_mwm_single_kernel(const SqMatchJob *jobs, const SqMatchEdge *edges, char *scratch,
                                                                     int32_t *mate_out, int lds_bytes, uint32_t *job_flags,
                                                                     uint32_t stamp)
{
    __shared__ SqBlossom bl;
    extern __shared__ __attribute__((aligned(16))) char mwm_lds[];
    sq_mwm_one(bl, mwm_lds, mwm_lds, (size_t)lds_bytes, jobs + blockIdx.x, (int)blockIdx.x, edges, scratch, mate_out, job_flags, stamp,
               (int)threadIdx.x, [] { __syncthreads(); });
}

extern "C" __global__ void sq_flag_kernel(uint32_t *flag, uint32_t value)
{
    sq_host_write_flush(flag);                           // (the results in pinned memory: earlier kernels)
    *flag = value;
}

// the switches the plan of a chunk honours (sq_algo_plan.h reads no environment itself)
SqAlgoKnobs sq_algo_knobs(int lsap_classes)
{
    const SqTuning &tu = sq_tuning();
    SqAlgoKnobs kn;
    kn.mwm_classes = tu.mwm_classes; kn.lsap_classes = lsap_classes;
    kn.mwm_bin_waves = tu.mwm_bin_waves; kn.mwm_bin_bytes = tu.mwm_bin_bytes; kn.mwm_all_cap = tu.mwm_all_cap;
    kn.mwm_nolds = tu.mwm_nolds; kn.nuss_threads = tu.nuss_threads;
    return kn;
}

// Launch configuration of the three matching kernels (dynamic LDS sized for the largest job of the launch), shared
// by the fold path (sq_algos.hip) and the graph-level C entries (sq_graph.hip).  jobs / edges: what the kernels read
// (pinned host or device memory); h_jobs: the same table on the host; dev_edges: device room for the edge list, used
// only when some blossom job has to run in global memory.  Asynchronous on st.
// The blossom graphs of one launch are packed into bins (blocks) by LDS need: sq_mwm_plan (sq_algo_plan.h).
int sq_launch_matching(int algo, const SqMatchJob *h_jobs, int nj, const SqMatchJob *jobs, const SqMatchEdge *edges,
                       size_t nedges, SqMatchEdge *dev_edges, char *d_scr, int32_t *out, int32_t *cnt,
                       const uint8_t *codes, uint32_t *job_flags, uint32_t flag_val, hipStream_t st,
                       SqMatchJob *jobs_rw, int32_t *bin_head, int inflight, const SqAlgoKnobs &kn, bool dump)
{
    int maxn = 0, maxm = 0;
    for (int q = 0; q < nj; q++) { maxn = maxn > h_jobs[q].n ? maxn : h_jobs[q].n; maxm = maxm > h_jobs[q].nedges ? maxm : h_jobs[q].nedges; }
    if (algo == 4) {                                     // SQ_ALGO_H
        const SqLsapLds P = sq_lsap_launch_lds(h_jobs, nj);
        if (P.need > 64 * 1024) sq_max_dynamic_lds((const void *)sq_lsap_kernel, (int)SQ_LSAP_LDS_CAP);
        hipLaunchKernelGGL(sq_lsap_kernel, dim3(nj), dim3(64), P.lds, st, jobs, edges, d_scr, out, (int)P.lds);
    } else if (algo == 2) {                              // SQ_ALGO_N
        const int nthr = sq_nussinov_threads(h_jobs, nj, maxn, inflight, kn);
        hipLaunchKernelGGL(sq_nussinov_kernel, dim3(nj), dim3(nthr), 0, st, jobs, edges, codes, d_scr, out, cnt, jobs_rw ? 1 : 0);
    } else {                                             // SQ_ALGO_E
        // bins: see sq_mwm_plan.  The plan writes each job's LDS slice into the job table the kernel reads.
        const SqMwmPlan P = sq_mwm_plan(h_jobs, jobs_rw, nj, bin_head, inflight, kn, dump);
        const size_t lds = P.lds;
        sq_max_dynamic_lds((const void *)sq_mwm_kernel, 156 * 1024);
        if (!P.all_in_lds && dev_edges != edges) {
            // some job keeps its adjacency in global memory and walks the edges in place: give the launch a device copy
            hipError_t e = hipMemcpyAsync(dev_edges, edges, nedges * sizeof(SqMatchEdge), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) return (int)e;
            edges = dev_edges;
        }
        if (P.waves == 1) {
            // one graph per block: blocks in table order, every block with the LDS of the launch's largest graph
            sq_max_dynamic_lds((const void *)sq_mwm_single_kernel, 156 * 1024);
            const size_t one = lds > sq_blossom_hdr() ? lds - sq_blossom_hdr() : 0;
            hipLaunchKernelGGL(sq_mwm_single_kernel, dim3(nj), dim3(64), one, st, jobs, edges, d_scr, out, (int)one, job_flags, flag_val);
        } else
            hipLaunchKernelGGL(sq_mwm_kernel, dim3(P.nbins), dim3(64 * P.waves), lds, st, jobs, bin_head, edges, d_scr, out, job_flags, flag_val);
    }
    return (int)hipGetLastError();
}
