// Interaction screens (FoldDuplex): what every duplex's consensus row holds between and inside its two chains, and what it
// opens of the structures the chains have alone, on the device.
//
//   sq_duplex_summary   per duplex the pairs between the chains and inside each, the pairs of each chain alone that the duplex
//                       lacks, the first and the last position of each chain that pairs across; per solo position the
//                       duplexes in which it pairs across.  Entry logic: sq_duplex.h.
//
// All buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_duplex.h"

// One wave per duplex at a time, four duplexes per 256-thread block, as sq_variant_diff_kernel: a screen's rows are short (a
// 21-nt query on a 60-nt window is two chunks of 64 positions).  The wave walks the duplex row 64 contiguous positions per step;
// a lane on the A side reads A's row at the same index, a lane behind the separator reads B's row at t - nA - 1 (contiguous,
// not chunk-aligned).  The five counts are popcounts of wave ballots, the four first / last values the lowest / highest set
// bit of the first / last non-empty inter mask of either side.  No LDS, no barrier: the waves of a block do not know of one another.
extern "C" __global__ __launch_bounds__(256) void sq_duplex_summary_kernel(SqDuplex s, int32_t *summary, int32_t *bound,
                                                                           unsigned long long *out)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t k = (int64_t)blockIdx.x * 4 + wave; k < s.ndup; k += nwaves) {      // (wave-uniform: so are the loops below)
        SqDuplexShape h;
        if (!s.shape((int32_t)k, h)) {
            out[1] = 2ull;
            continue;
        }
        const int32_t *A = s.solo_row(h.a), *B = s.solo_row(h.b), *D = s.duplex_row(k);
        int32_t *bound_a = bound + s.pos_off[h.a], *bound_b = bound + s.pos_off[h.b];
        const int32_t sep = h.nA + 1;                                // (B's position u is duplex position u + sep)
        const int64_t n = (int64_t)h.nA + 1 + h.nB;                  // (< 2^31; the chunks' start in 64 bits: tb + 64 may not be)
        int32_t inter = 0, intra_a = 0, intra_b = 0, lost_a = 0, lost_b = 0, a_first = -1, a_last = -1, b_first = -1, b_last = -1;
        for (int64_t tb = 0; tb < n; tb += 64) {                     // (n rounded up to 64: all 64 lanes reach the ballots)
            const int64_t t = tb + lane;
            const int f = t < n ? SqDuplex::entry(A, B, D, h.nA, h.nB, (int32_t)t) : 0;
            if (f & SQ_D_INVALID) out[1] = 2ull;
            intra_a += __popcll(__ballot(f & SQ_D_INTRA_A));
            intra_b += __popcll(__ballot(f & SQ_D_INTRA_B));
            lost_a += __popcll(__ballot(f & SQ_D_LOST_A));
            lost_b += __popcll(__ballot(f & SQ_D_LOST_B));
            const unsigned long long am = __ballot(f & SQ_D_INTER_A), bm = __ballot(f & SQ_D_INTER_B);
            if (am) {
                inter += __popcll(am);
                if (a_first < 0) a_first = (int32_t)tb + __ffsll((long long)am) - 1;
                a_last = (int32_t)tb + 63 - __clzll((long long)am);
            }
            if (bm) {                                                // (B's own coordinates: behind the separator)
                if (b_first < 0) b_first = (int32_t)tb + __ffsll((long long)bm) - 1 - sep;
                b_last = (int32_t)tb + 63 - __clzll((long long)bm) - sep;
            }
            if (f & SQ_D_INTER_A) atomicAdd(&bound_a[t], 1);         // (int32 adds at inter-paired positions only)
            if (f & SQ_D_INTER_B) atomicAdd(&bound_b[t - sep], 1);
        }
        if (lane == 0) {
            int32_t *d = summary + k * 9;
            d[0] = inter; d[1] = intra_a; d[2] = intra_b; d[3] = lost_a; d[4] = lost_b;
            d[5] = a_first; d[6] = a_last; d[7] = b_first; d[8] = b_last;
        }
    }
}

extern "C" int sq_duplex_summary(const int32_t *d_partner_s, const int64_t *d_cell_off_s, const int64_t *d_lengths_s, int32_t nsolo,
                                 const int32_t *d_partner_d, const int64_t *d_cell_off_d, const int64_t *d_lengths_d, int32_t ndup,
                                 const int32_t *d_a_rec, const int32_t *d_b_rec, const int64_t *d_pos_off, int64_t Ltot,
                                 int32_t *d_summary, int32_t *d_bound, uint64_t *d_out, void *hip_stream)
{
    if (nsolo < 0 || ndup < 0 || Ltot <= 0 || Ltot > 0x7fffffffll || !d_out || !d_bound ||
        (ndup && (!d_partner_s || !d_cell_off_s || !d_lengths_s || !d_partner_d || !d_cell_off_d || !d_lengths_d || !d_a_rec ||
                  !d_b_rec || !d_pos_off || !d_summary))) {
        sq_set_error("sq_duplex_summary: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    HIPCK(hipMemsetAsync(d_bound, 0, (size_t)Ltot * sizeof(int32_t), st));
    if (!ndup) return 0;
    SqDuplex s;
    s.partner_s = d_partner_s; s.cell_off_s = d_cell_off_s; s.lengths_s = d_lengths_s; s.nsolo = nsolo;
    s.partner_d = d_partner_d; s.cell_off_d = d_cell_off_d; s.lengths_d = d_lengths_d; s.ndup = ndup;
    s.a_rec = d_a_rec; s.b_rec = d_b_rec; s.pos_off = d_pos_off; s.Ltot = Ltot;
    // At most SQ_DUPLEX_MAX_BLOCKS = 2048 blocks, the rest by grid stride: 8 blocks of 4 waves fill the 32 wave slots of each of
    // the 256 CUs, so 2048 blocks are all the waves the chip holds at once and a larger grid would only queue behind them.
    const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)ndup + 3) / 4, SQ_DUPLEX_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_duplex_summary_kernel, dim3(blocks), dim3(256), 0, st, s, d_summary, d_bound, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_duplex_summary_kernel");
}
