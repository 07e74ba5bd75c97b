// Sliding-window folds of long sequences (FoldWindows): the pair table of all windows' consensus rows, on the device.
//
//   sq_window_pair_count   for every distinct pair of positions that the consensus row of any window holds: how many windows
//                          hold it, how many contain it and the first that holds it.  "The first holder emits"
//                          (sq_windows.h): no dense table, no scratch, no memset but the two result words.
//
// All buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_windows.h"
#include "sq_emit.h"

// One block per window at a time, one thread per position t of it: the rows of the neighbouring windows are read at
// t + const, contiguous across a wave.  The emitted records go through the block's emission stage (sq_emit.h): staged in LDS
// and written out behind one global atomic per flush.
extern "C" __global__ __launch_bounds__(256) void sq_window_count_kernel(SqWindows w, long long *flat_out, int32_t *count_out, int32_t *cover_out,
                                                                         int32_t *first_out, long long cap, unsigned long long *out)
{
    __shared__ long long s_flat[SQ_EMIT_STAGE];
    __shared__ int32_t s_cnt[SQ_EMIT_STAGE], s_cov[SQ_EMIT_STAGE], s_first[SQ_EMIT_STAGE];
    __shared__ SqEmitStage em;
    const int tid = threadIdx.x;
    em.init();
    auto write = [&](uint32_t k, unsigned long long at) {
        if ((long long)at < cap) { flat_out[at] = s_flat[k]; count_out[at] = s_cnt[k]; cover_out[at] = s_cov[k]; first_out[at] = s_first[k]; }
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
            const uint32_t at = em.slot(hit);
            if (hit) { s_flat[at] = (long long)flat; s_cnt[at] = cnt; s_cov[at] = cov; s_first[at] = first; }
            em.step(out, write);
        }
    }
    em.finish(out, write);
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
