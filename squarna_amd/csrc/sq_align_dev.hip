// Alignment mode's consensus on the device (FoldAlignment): the two steps that used to leave it.
//
//   sq_align_pair_count   the consensus rows of a fold (pair tables of sq_result_pairs_dev) lifted through the rows' gap maps
//                         into alignment columns and counted: for every distinct column pair how many rows hold it and the
//                         first row that does -- Consensus' dict, SQRNdbnali.py:281-284, as two dense int32 tables
//                         (integer atomics: exact, any order) and a select pass
//   sq_first_fit_dev      the greedy pass over ranked candidates (MatrixToDBNs :127-192, Consensus :285-295) in rounds
//                         (sq_firstfit.h), one workgroup
//
// All buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_firstfit.h"
#include "sq_emit.h"

// ---- lift and count -----------------------------------------------------------------------------------------------------
// One thread per (row r, gap-free position i): the pair (i, j = partner) with i < j becomes the column pair (v, w).  A row
// holds a pair at most once (a partner array), so count[v, w] is the number of rows and first[v, w] the smallest row.
// A table entry outside the row or the matrix is not counted: out[1] reports it (status 2).
extern "C" __global__ __launch_bounds__(256) void sq_pair_count_kernel(const int32_t *partner, const int64_t *cell_off, const int32_t *col_off,
                                                                       const int32_t *cols, int nrec, int L, int32_t *count, int32_t *first,
                                                                       unsigned long long *out)
{
    for (int r = blockIdx.y; r < nrec; r += gridDim.y) {
        const int32_t c0 = col_off[r], n = col_off[r + 1] - c0;
        const int32_t *row = partner + cell_off[r];                       // row 0 of the record: its consensus
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
            const int32_t j = row[i];
            if (j <= i) continue;
            bool ok = j < n;
            int32_t v = 0, w = 0;
            if (ok) { v = cols[c0 + i]; w = cols[c0 + j]; ok = v >= 0 && v < w && w < L; }
            if (!ok) { out[1] = 2ull; continue; }
            const int64_t cell = (int64_t)v * L + w;
            atomicAdd(&count[cell], 1);
            atomicMin(&first[cell], r);
        }
    }
}

// The cells of the upper triangle with count >= threshold, through the block's emission stage (sq_emit.h): staged in LDS and
// written out behind one atomic per thousand.  Unordered.
extern "C" __global__ __launch_bounds__(256) void sq_pair_select_kernel(const int32_t *count, const int32_t *first, int L, int threshold,
                                                                        long long *flat_out, int32_t *count_out, int32_t *first_out,
                                                                        long long cap, unsigned long long *out)
{
    __shared__ long long s_flat[SQ_EMIT_STAGE];
    __shared__ int32_t s_cnt[SQ_EMIT_STAGE], s_first[SQ_EMIT_STAGE];
    __shared__ SqEmitStage em;
    const int tid = threadIdx.x;
    em.init();
    auto write = [&](uint32_t k, unsigned long long at) {
        if ((long long)at < cap) { flat_out[at] = s_flat[k]; count_out[at] = s_cnt[k]; first_out[at] = s_first[k]; }
    };
    for (int v = blockIdx.x; v < L; v += gridDim.x) {
        const int32_t *row = count + (int64_t)v * L;
        for (int wb = v + 1; wb < L; wb += 256) {
            const int w = wb + tid;
            const int32_t c = w < L ? row[w] : 0;
            const bool hit = c >= threshold;
            const uint32_t at = em.slot(hit);
            if (hit) { s_flat[at] = (int64_t)v * L + w; s_cnt[at] = c; s_first[at] = first[(int64_t)v * L + w]; }
            em.step(out, write);
        }
    }
    em.finish(out, write);
}

extern "C" size_t sq_align_pair_count_scratch(int32_t L)
{
    return L > 0 ? 2 * sizeof(int32_t) * (size_t)L * (size_t)L : 0;
}

extern "C" int sq_align_pair_count(const int32_t *d_partner, const int64_t *d_cell_off, const int32_t *d_col_off, const int32_t *d_cols,
                                   int32_t nrec, int32_t L, int32_t threshold, void *d_scratch, size_t scratch_bytes, int64_t *d_flat,
                                   int32_t *d_count, int32_t *d_first, int64_t cap, uint64_t *d_out, void *hip_stream)
{
    if (nrec < 0 || L <= 0 || threshold < 1 || !d_scratch || !d_out || cap < 0 || (cap && (!d_flat || !d_count || !d_first)) ||
        (nrec && (!d_partner || !d_cell_off || !d_col_off || !d_cols))) { sq_set_error("bad argument"); return -1; }
    if (scratch_bytes < sq_align_pair_count_scratch(L)) {
        sq_set_error("sq_align_pair_count: scratch of " + std::to_string(scratch_bytes) + " bytes, " +
                     std::to_string(sq_align_pair_count_scratch(L)) + " needed");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t cells = (size_t)L * L;
    int32_t *count = (int32_t *)d_scratch, *first = count + cells;
    HIPCK(hipMemsetAsync(count, 0, cells * 4, st));
    HIPCK(hipMemsetAsync(first, 0x7f, cells * 4, st));                   // (0x7f7f7f7f: above every row index)
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    if (nrec) {
        const dim3 grid((unsigned)std::min((L + 255) / 256, 64), (unsigned)std::min<int32_t>(nrec, 8192));
        hipLaunchKernelGGL(sq_pair_count_kernel, grid, dim3(256), 0, st, d_partner, d_cell_off, d_col_off, d_cols, nrec, L, count, first,
                           (unsigned long long *)d_out);
        HIPCK(hipGetLastError());
    }
    hipLaunchKernelGGL(sq_pair_select_kernel, dim3((unsigned)std::min<int32_t>(L, 2048)), dim3(256), 0, st, count, first, L, threshold,
                       (long long *)d_flat, d_count, d_first, (long long)cap, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_pair_select_kernel");
}

// ---- first fit ----------------------------------------------------------------------------------------------------------
// The device's policy of sq_firstfit.h: ONE workgroup.  The shared words (column minima, partners, the live lists and their
// lengths) live in global memory, so that L and n have no LDS bound; every access to them is a device-scope atomic or an
// agent-scope relaxed load / store, which are served by the L2 -- no copy of such a word in the CU's vector cache is ever
// read --, and the workgroup's barrier orders the phases.
struct SqFitBlock {
    __device__ int tid() const { return (int)threadIdx.x; }
    __device__ int nthreads() const { return (int)blockDim.x; }
    __device__ void barrier() const { __syncthreads(); }
    __device__ int32_t load(const int32_t *p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void store(int32_t *p, int32_t v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void min_at(int32_t *p, int32_t v) const { atomicMin(p, v); }
    __device__ int32_t add_at(int32_t *p, int32_t v) const { return atomicAdd(p, v); }
};

extern "C" __global__ __launch_bounds__(1024) void sq_first_fit_kernel(SqFirstFit f, int32_t *info)
{
    SqFitBlock x;
    f.run(x);
    if (threadIdx.x == 0) for (int q = 0; q < 4; q++) info[q] = x.load(&f.ctl[4 + q]);
}

extern "C" size_t sq_first_fit_scratch(int64_t n, int32_t L)
{
    return n >= 0 && L > 0 ? sizeof(int32_t) * SqFirstFit::scratch_ints(n, L) : 0;
}

extern "C" int sq_first_fit_dev(const int64_t *d_flat, int64_t n, int32_t L, int32_t minspan, int32_t *d_partner, void *d_scratch,
                                size_t scratch_bytes, int32_t *d_info, void *hip_stream)
{
    if (n < 0 || n >= 0x7fffffffll || L <= 0 || (n && !d_flat) || !d_partner || !d_scratch || !d_info) { sq_set_error("bad argument"); return -1; }
    if (scratch_bytes < sq_first_fit_scratch(n, L)) {
        sq_set_error("sq_first_fit_dev: scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(sq_first_fit_scratch(n, L)) +
                     " needed");
        return -1;
    }
    SqFirstFit f;
    f.flat = d_flat; f.n = n; f.L = L; f.minspan = minspan; f.partner = d_partner;
    f.bind((int32_t *)d_scratch);
    hipLaunchKernelGGL(sq_first_fit_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, f, d_info);
    return sq_check(hipGetLastError(), "sq_first_fit_kernel");
}
