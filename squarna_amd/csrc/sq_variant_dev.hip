// Mutational scans (FoldMutants): what every variant's consensus row changes against its wild type's, on the device.
//
//   sq_variant_diff   per variant the pairs lost, gained and kept, the positions whose partner changed with the first and the
//                     last of them; per wild-type position the variants that changed its partner.  Entry logic: sq_variants.h.
//
// All buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_variants.h"

// One wave per variant at a time, four variants per 256-thread block: the rows are short (SRtest150's mean is 60 nt -- one
// chunk of 64 positions), so a block per variant would idle three of its four waves.  The wave reads both rows once, 64
// contiguous positions per step; the four counts are popcounts of wave ballots, first / last the lowest / highest set bit of
// the first / last non-empty `changed` mask.  No LDS, no barrier: the waves of a block do not know of one another.
extern "C" __global__ __launch_bounds__(256) void sq_variant_diff_kernel(SqVariants s, int32_t *diff, int32_t *pos_changed,
                                                                         unsigned long long *out)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t m = (int64_t)blockIdx.x * 4 + wave; m < s.nvar; m += nwaves) {      // (wave-uniform: so are the loops below)
        const int32_t n = s.length((int32_t)m);
        if (n < 0) {
            out[1] = 2ull;
            continue;
        }
        const int64_t wt = s.wt_rec[m];
        const int32_t *w = s.row(wt), *v = s.row((int64_t)s.rec0 + m);
        int32_t *changed_at = pos_changed + s.pos_off[wt];
        int32_t lost = 0, kept = 0, gained = 0, changed = 0, first = -1, last = -1;
        for (int32_t tb = 0; tb < n; tb += 64) {                 // (n rounded up to 64: all 64 lanes reach the ballots)
            const int32_t t = tb + lane;
            const int f = t < n ? SqVariants::entry(w, v, n, t) : 0;
            if (f & SQ_V_INVALID) out[1] = 2ull;
            lost += __popcll(__ballot(f & SQ_V_LOST));
            kept += __popcll(__ballot(f & SQ_V_KEPT));
            gained += __popcll(__ballot(f & SQ_V_GAINED));
            const unsigned long long cm = __ballot(f & SQ_V_CHANGED);
            if (cm) {
                changed += __popcll(cm);
                if (first < 0) first = tb + __ffsll((long long)cm) - 1;
                last = tb + 63 - __clzll((long long)cm);
            }
            if (f & SQ_V_CHANGED) atomicAdd(&changed_at[t], 1);  // (contiguous int32 adds; few lanes in practice)
        }
        if (lane == 0) {
            int32_t *d = diff + m * 6;
            d[0] = lost; d[1] = gained; d[2] = kept; d[3] = changed; d[4] = first; d[5] = last;
        }
    }
}

extern "C" int sq_variant_diff(const int32_t *d_partner, const int64_t *d_cell_off, const int64_t *d_lengths, int32_t rec0, int32_t nvar,
                               const int32_t *d_wt_rec, const int64_t *d_pos_off, int64_t Ltot, int32_t *d_diff, int32_t *d_pos_changed,
                               uint64_t *d_out, void *hip_stream)
{
    if (rec0 < 0 || nvar < 0 || Ltot <= 0 || Ltot > 0x7fffffffll || !d_out || !d_pos_changed ||
        (nvar && (!d_partner || !d_cell_off || !d_lengths || !d_wt_rec || !d_pos_off || !d_diff))) {
        sq_set_error("sq_variant_diff: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    HIPCK(hipMemsetAsync(d_pos_changed, 0, (size_t)Ltot * sizeof(int32_t), st));
    if (!nvar) return 0;
    SqVariants s;
    s.partner = d_partner; s.cell_off = d_cell_off; s.lengths = d_lengths; s.wt_rec = d_wt_rec; s.pos_off = d_pos_off;
    s.rec0 = rec0; s.nvar = nvar; s.Ltot = Ltot;
    // At most SQ_VARIANT_MAX_BLOCKS = 2048 blocks, the rest by grid stride: 8 blocks of 4 waves fill the 32 wave slots of each of
    // the 256 CUs, so 2048 blocks are all the waves the chip holds at once and a larger grid would only queue behind them.
    const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)nvar + 3) / 4, SQ_VARIANT_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_variant_diff_kernel, dim3(blocks), dim3(256), 0, st, s, d_diff, d_pos_changed, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_variant_diff_kernel");
}
