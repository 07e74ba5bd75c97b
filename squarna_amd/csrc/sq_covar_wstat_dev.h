// Device code the translation units of the weighted covariation statistics share (sq_covar_wstat_dev.hip, and
// sq_covar_wstat_null_dev.hip for their shuffled-column null): the staged planes of a tile, and the 16 counters of a cell
// through the thread's bins in LDS, tile by tile (tile_bins) and from global memory (cell_bins).  Included by .hip files only;
// a block has 256 threads and its dynamic LDS is carved by sq_covar_wstat_lds() (sq_covar_wstat.h).
#pragma once
#include "sq_covar_wstat.h"

namespace {

constexpr int WSTAT_T = SQ_COVSTAT_TILE, WSTAT_CH = SQ_COVSTAT_WORD_CHUNK;
static_assert(WSTAT_T == 32 && 64 * WSTAT_CH == 256, "a tile is four cells per thread of a 256-thread block, a chunk one row per thread");

extern __shared__ __attribute__((aligned(16))) char s_dyn[];

struct WstatPlanesLds {
    uint64_t v[4][WSTAT_CH][WSTAT_T], w[4][WSTAT_CH][WSTAT_T];      // the planes A C G U of the tile's two column ranges
};

// The 16 bins of the thread's cell (w = w0 + tid % 32, v = v0 + vl) over all rows: bins[k * 256], cleared here.  Per CH words
// of rows the planes of both column ranges and the chunk's 256 weights are staged in LDS; words beyond W are staged as zero
// (q is zero beyond R up to the chunk), so every trip count is block-uniform.  v0 + 31, w0 + 31 < Lpad.
__device__ __forceinline__ void tile_bins(const uint64_t *plane, const uint32_t *q, int64_t W, int64_t Lpad, int64_t v0, int64_t w0,
                                          WstatPlanesLds &s, uint32_t *s_q, int vl, int64_t *bins, int64_t Q[16])
{
    constexpr int T = WSTAT_T, CH = WSTAT_CH;
    const int tid = threadIdx.x, wl = tid & 31;
    for (int k = 0; k < 16; k++) bins[k * 256] = 0;
    for (int64_t wb = 0; wb < W; wb += CH) {
        __syncthreads();                                             // (the last chunk has been read)
        for (int i = tid; i < 4 * CH * T; i += 256) {
            const int p = i / (CH * T), wd = i / T % CH, col = i % T;
            const bool have = wb + wd < W;
            s.v[p][wd][col] = have ? plane[SqCovar::at(p, wb + wd, v0 + col, W, Lpad)] : 0ull;
            s.w[p][wd][col] = have ? plane[SqCovar::at(p, wb + wd, w0 + col, W, Lpad)] : 0ull;
        }
        s_q[tid] = q[wb * 64 + tid];                                 // (wb * 64 + 255 < rpad(R))
        __syncthreads();
        for (int wd = 0; wd < CH; wd++) {
            uint64_t a[4], b[4];
            for (int p = 0; p < 4; p++) {
                a[p] = s.v[p][wd][vl];
                b[p] = s.w[p][wd][wl];
            }
            SqCovarWstat::accumulate(a, b, s_q + wd * 64, bins, 256);
        }
    }
    for (int k = 0; k < 16; k++) Q[k] = bins[k * 256];
}

// The 16 counters of one cell from global memory, through the thread's bins (the pairs lookups, and the scan's flush for the
// records it writes: between two cells of the walk the thread's bins are free).
__device__ __forceinline__ void cell_bins(const uint64_t *plane, const uint32_t *q, int64_t W, int64_t Lpad, int64_t v, int64_t w,
                                          int64_t *bins, int64_t Q[16])
{
    for (int k = 0; k < 16; k++) bins[k * 256] = 0;
    for (int64_t wd = 0; wd < W; wd++) {
        uint64_t a[4], b[4];
        for (int p = 0; p < 4; p++) {
            a[p] = plane[SqCovar::at(p, wd, v, W, Lpad)];
            b[p] = plane[SqCovar::at(p, wd, w, W, Lpad)];
        }
        SqCovarWstat::accumulate(a, b, q + wd * 64, bins, 256);      // (wd * 64 + 63 < rpad(R))
    }
    for (int k = 0; k < 16; k++) Q[k] = bins[k * 256];
}

}  // namespace
