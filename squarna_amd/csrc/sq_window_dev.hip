// Sliding-window folds of long sequences (FoldWindows): the pair table of all windows' consensus rows, on the device.
//
//   sq_window_pair_count   for every distinct pair of positions that the consensus row of any window holds: how many windows
//                          hold it, how many contain it and the first that holds it.  "The first holder emits"
//                          (sq_windows.h): no dense table, no scratch, no memset but the two result words.
//
// All buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_windows.h"

// One block per window at a time, one thread per position t of it: the rows of the neighbouring windows are read at
// t + const, contiguous across a wave.  The emitted records are staged in LDS and written out behind one global atomic per
// flush (sq_pair_select_kernel's form).  Whether to flush is decided from ONE read of the LDS counter between two barriers,
// so every wave of the block decides the same: no wave adds to the counter before all have read it.
#define SQ_W_STAGE 1024
extern "C" __global__ __launch_bounds__(256) void sq_window_count_kernel(SqWindows w, long long *flat_out, int32_t *count_out, int32_t *cover_out,
                                                                         int32_t *first_out, long long cap, unsigned long long *out)
{
    __shared__ long long s_flat[SQ_W_STAGE];
    __shared__ int32_t s_cnt[SQ_W_STAGE], s_cov[SQ_W_STAGE], s_first[SQ_W_STAGE];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_n = 0u;
    __syncthreads();
    auto flush = [&](uint32_t n) {                          // (block-uniform call with a block-uniform n, after a barrier)
        if (tid == 0) s_base = atomicAdd(out, (unsigned long long)n);
        __syncthreads();                                    // (every thread has read the counter by now)
        const unsigned long long base = s_base;
        if (tid == 0) s_n = 0u;
        for (uint32_t k = tid; k < n; k += 256)
            if ((long long)(base + k) < cap) {
                flat_out[base + k] = s_flat[k]; count_out[base + k] = s_cnt[k]; cover_out[base + k] = s_cov[k]; first_out[base + k] = s_first[k];
            }
        __syncthreads();                                    // (the stage is free again)
    };
    for (int k = blockIdx.x; k < w.nwin; k += gridDim.x) {
        const int32_t n = w.len[k];                         // (block-uniform: so are the loop and its barriers)
        for (int32_t tb = 0; tb < n; tb += 256) {
            const int32_t t = tb + tid;
            int64_t flat = 0;
            int32_t cnt = 0, cov = 0, first = 0;
            const int what = t < n ? w.entry(k, t, flat, cnt, cov, first) : SQ_W_NONE;
            if (what == SQ_W_INVALID) out[1] = 2ull;
            const bool hit = what == SQ_W_EMIT;
            const unsigned long long m = __ballot(hit);
            if (m != 0ull) {
                uint32_t b0 = 0u;
                if (lane == 0) b0 = atomicAdd(&s_n, (uint32_t)__popcll(m));
                b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
                if (hit) {
                    const uint32_t at = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    s_flat[at] = (long long)flat; s_cnt[at] = cnt; s_cov[at] = cov; s_first[at] = first;
                }
            }
            __syncthreads();
            const uint32_t staged = s_n;                    // (one read per thread, before anyone adds again)
            __syncthreads();
            if (staged > SQ_W_STAGE - 256u) flush(staged);  // (room for the next 256)
        }
    }
    const uint32_t staged = s_n;                            // (nothing was added since the last barrier)
    if (staged > 0u) flush(staged);
}

extern "C" int sq_window_pair_count(const int32_t *d_partner, const int64_t *d_cell_off, int32_t rec0, int32_t nwin, const int64_t *d_start,
                                    const int32_t *d_len, int64_t Ltot, int64_t *d_flat, int32_t *d_count, int32_t *d_cover,
                                    int32_t *d_first, int64_t cap, uint64_t *d_out, void *hip_stream)
{
    if (rec0 < 0 || nwin < 0 || Ltot <= 0 || Ltot > 0x7fffffffll || !d_out || cap < 0 ||
        (cap && (!d_flat || !d_count || !d_cover || !d_first)) || (nwin && (!d_partner || !d_cell_off || !d_start || !d_len))) {
        sq_set_error("sq_window_pair_count: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    if (!nwin) return 0;
    SqWindows w;
    w.partner = d_partner; w.cell_off = d_cell_off; w.start = d_start; w.len = d_len; w.rec0 = rec0; w.nwin = nwin; w.Ltot = Ltot;
    hipLaunchKernelGGL(sq_window_count_kernel, dim3((unsigned)std::min<int32_t>(nwin, 512)), dim3(256), 0, st, w, (long long *)d_flat, d_count,
                       d_cover, d_first, (long long)cap, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_window_count_kernel");
}
