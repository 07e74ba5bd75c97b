// sq_match.h -- job records of the on-device matching step (a-8, a-9, Nussinov); the layouts, byte counts and algorithms of the
// Hungarian and Nussinov jobs come with it (sq_lsap.h, sq_nussinov.h, included below).
#pragma once
#include <stddef.h>
#include <stdint.h>

struct SqMatchEdge {      // one cell (v, w), v < w, of a stem with its weight
    int32_t v, w;         // LSAP / Nussinov: sequence positions; blossom: vertex ids in graph order
    double weight;        // H, E: stemscore ** 1.7 (host libm);  N: stemscore
};

struct SqMatchJob {
    int32_t n;            // LSAP / Nussinov: sequence length; blossom: number of graph vertices
    int32_t nedges;
    int64_t edge_off;     // into the edge array
    int64_t scratch_off;  // bytes into the scratch arena
    int64_t out_off;      // ints into the output array (pairs: 2 ints each for Nussinov)
    int64_t pos_off;      // sequence offset into the per-position arrays (Nussinov separators)
    // blossom: the graph's slice of its block's dynamic LDS and the next graph of the same block (sq_mwm_plan)
    int32_t lds_off, lds_bytes;
    int32_t next, pad;
};

// Host+device code of the matching step (sq_blossom.h, sq_lsap.h, sq_nussinov.h also compile with a plain C++ compiler for the
// CPU tests).  SQ_HD_INLINE: the body of a kernel -- inlined before the optimiser runs, as if written into the kernel (the
// Hungarian template took one VGPR more as an ordinary inline function).
#ifdef __HIPCC__
#define SQ_HD __host__ __device__
#define SQ_HD_INLINE __host__ __device__ __forceinline__
#define SQ_UNROLL _Pragma("unroll")
#else
#define SQ_HD
#define SQ_HD_INLINE inline
#define SQ_UNROLL
#endif

// The scratch and LDS layouts of the Hungarian and Nussinov kernels are carved array by array, as sq_algo_carve (sq_algo_plan.h)
// carves the region of a chunk: the array starts at the next multiple of `align` bytes behind what `base` holds so far.
// (Offsets, not pointers, are rounded: a pointer that went through an integer has lost its address space.)
template <class T>
SQ_HD static inline void sq_take(char *base, size_t &o, T *&a, size_t count, size_t align = alignof(T))
{
    o = (o + align - 1) & ~(align - 1);
    a = reinterpret_cast<T *>(base + o);
    o += count * sizeof(T);
}

#include "sq_lsap.h"       // SqLsapLayout, sq_lsap_*_bytes, sq_lsap_form, sq_lsap_run
#include "sq_nussinov.h"   // SqNussLayout, sq_nussinov_scratch_bytes, sq_nussinov_run

// ---- records of the device-side RunAlgo (sq_algos_dev.hip) that the plan of a chunk (sq_algo_plan.h) sizes ----
struct SqAlgoSize {                // per E / H / N job after its AnnotateStems pass (pinned, read by the host)
    int32_t nedges;                // cells of its stems
    int32_t nv;                    // distinct positions on them (Edmonds: graph vertices)
    int32_t nok;                   // stems
    int32_t raw_base;              // jobs whose edge weights need the host libm: where its nok stem scores start in the raw list
                                   // (-1: weights from the paramset's table; -2: the list had no room)
};
struct SqAlgoJob {                 // per job, for the edges / finish kernels (pinned, written by the host once the sizes are known)
    int32_t job, algo;             // batch job index, SQ_ALGO_*
    SqMatchEdge *edges;            // device: the job's edge list
    int32_t *vid2pos;              // device, Edmonds: graph vertex -> sequence position
    const double *raw;             // pinned: stemscore ** 1.7 of the job's stems in survivor-list order (nullptr: the paramset's table)
};
struct SqAlgoStat {                // per launch of the finish kernel (device; sq_algo_publish_kernel copies it to the host)
    uint32_t bad;                  // 1: blossom capacity exceeded, 2: stem capacity exceeded
    uint32_t level_ovf;
    unsigned long long max_pass_job;   // (scan passes << 32) | job row: the blossom kernel's critical path
    unsigned long long passes, graphs;
    long long max_events, max_n, max_m;
};

#ifdef __HIPCC__
struct SqAlgoKnobs;                                      // sq_algo_plan.h
void sq_max_dynamic_lds(const void *fn, int bytes);      // sq_host.hip: once per (kernel, device)
int sq_launch_matching(int algo, const SqMatchJob *h_jobs, int nj, const SqMatchJob *jobs, const SqMatchEdge *edges,
                       size_t nedges, SqMatchEdge *dev_edges, char *d_scr, int32_t *out, int32_t *cnt,
                       const uint8_t *codes, uint32_t *job_flags, uint32_t flag_val, hipStream_t st,
                       SqMatchJob *jobs_rw, int32_t *bin_head, int inflight, const SqAlgoKnobs &kn, bool dump = false);
extern "C" {
__global__ void sq_lsap_kernel(const SqMatchJob *jobs, const SqMatchEdge *edges, char *scratch, int32_t *col4row_out,
                               int lds_bytes);
__global__ void sq_nussinov_kernel(const SqMatchJob *jobs, const SqMatchEdge *edges, const uint8_t *codes,
                                   char *scratch, int32_t *pairs_out, int32_t *count_out, int by_pad);
__global__ void sq_mwm_kernel(const SqMatchJob *jobs, const int32_t *bin_head, const SqMatchEdge *edges, char *scratch,
                              int32_t *mate_out, uint32_t *job_flags, uint32_t stamp);
__global__ void sq_mwm_single_kernel(const SqMatchJob *jobs, const SqMatchEdge *edges, char *scratch, int32_t *mate_out,
                                     int lds_bytes, uint32_t *job_flags, uint32_t stamp);
// one thread, launched behind a matching kernel on its stream: publishes "the results are in host memory"
__global__ void sq_flag_kernel(uint32_t *flag, uint32_t value);
}
#endif
