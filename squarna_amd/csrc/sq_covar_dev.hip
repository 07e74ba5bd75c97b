// Covariation evidence for alignment columns (Covariation): how the rows of an alignment support pairs of its columns, on the
// device.  Counts, layout and predicates: sq_covar.h.
//
//   sq_covar_planes_kernel   the ASCII rows as five bit planes (A, C, G, U, gap) of 64 rows per word, the column fastest
//   sq_covar_scan_kernel     the seven counters and cov of every cell v < w with w - v >= minspan, tile by tile from LDS; the cells
//                            that pass the thresholds leave through the block's emission stage (sq_emit.h)
//   sq_covar_pairs_kernel    the same numbers for given column pairs, one lane per pair from global memory
//
// All buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_covar.h"
#include "sq_covar_planes.h"
#include "sq_emit.h"

// One block per 64 rows x 64 columns of the alignment.  The bytes are read row by row, 64 contiguous bytes per wave, and their
// classes staged in LDS (a row of rows[] starts at r * L, aligned to nothing: bytes, not words).  Then lane = row: every wave
// takes 16 of the tile's columns, and a plane's word for a column is the wave's ballot of "my row has the plane's class".
// Rows >= R and columns >= L are staged as "other", which has no plane: their bits, and the whole words of the columns
// L .. Lpad - 1, are zero.  The 5 x 64 words leave 64 consecutive columns at a time.
extern "C" __global__ __launch_bounds__(256) void sq_covar_planes_kernel(const uint8_t *rows, int32_t R, int32_t L, uint64_t *plane)
{
    __shared__ uint8_t s_cls[64][68];                            // (68: a lane's row starts one bank after its neighbour's)
    __shared__ uint64_t s_word[SQ_COV_PLANES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t word = blockIdx.x / (Lpad / 64);                // (block-uniform: one block per word of rows and 64 columns)
    const int64_t c0 = (int64_t)(blockIdx.x % (Lpad / 64)) * 64, r0 = word * 64;
    for (int k = wave; k < 64; k += 4) {
        const int64_t r = r0 + k, c = c0 + lane;
        s_cls[k][lane] = (uint8_t)(r < R && c < L ? SqCovar::cls(rows[r * L + c]) : SQ_COV_OTHER);
    }
    __syncthreads();
    for (int k = 0; k < 16; k++) {
        const int col = wave * 16 + k;
        const int mine = s_cls[lane][col];
        for (int p = 0; p < SQ_COV_PLANES; p++) {
            const unsigned long long m = __ballot(mine == p);
            if (lane == 0) s_word[p][col] = m;
        }
    }
    __syncthreads();
    for (int k = tid; k < SQ_COV_PLANES * 64; k += 256) {
        const int p = k >> 6, col = k & 63;                      // (c0 + col < Lpad and word < W: the grid has W * Lpad / 64 blocks)
        plane[SqCovar::at(p, word, c0 + col, W, Lpad)] = s_word[p][col];
    }
}

// The all-pairs scan.  A block takes the upper-triangle tiles k = blockIdx.x, + gridDim.x, ... (SqCovar::tile_of) of TILE x TILE
// cells: columns v in tile row ti, columns w in tile column tj.  Thread t has the four cells w = t % 32, v = 4 * (t / 32) .. + 3:
// the lanes of half a wave read 32 consecutive words of the w planes, and the whole half reads the same word of the v
// planes (a broadcast).  Per SQ_COV_WORD_CHUNK words of rows the planes of both column ranges are loaded into LDS, 32
// consecutive words of global memory at a time, and every thread adds 7 popcounts per cell and word to its 28 counters.
// Every trip count is block-uniform: words beyond W are staged as zero, cells outside the L columns or closer than minspan
// are computed and not emitted.  One slot() + step() per cell index of the thread (sq_emit.h's contract: at most 256 records a
// step); cov is not staged: the flush forms it again from the staged counters.
extern "C" __global__ __launch_bounds__(256) void sq_covar_scan_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t minspan,
                                                                      int32_t min_rows, long long min_cov, long long *flat_out,
                                                                      int32_t *counts_out, long long *cov_out, long long cap,
                                                                      unsigned long long *out)
{
    constexpr int T = SQ_COV_TILE, CH = SQ_COV_WORD_CHUNK;
    static_assert(T == 32 && SQ_EMIT_BLOCK == 256, "four cells per thread of a 256-thread block");
    __shared__ uint64_t s_v[SQ_COV_PLANES][CH][T], s_w[SQ_COV_PLANES][CH][T];
    __shared__ long long s_flat[SQ_EMIT_STAGE];
    __shared__ int32_t s_cnt[SQ_EMIT_STAGE * 7];
    __shared__ SqEmitStage em;
    const int tid = threadIdx.x, wl = tid & 31, vl = (tid >> 5) * 4;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t nT = ((int64_t)L + T - 1) / T, ntiles = SqCovar::tile_count(nT);
    em.init();
    auto write = [&](uint32_t k, unsigned long long at) {
        if ((long long)at < cap) {
            flat_out[at] = s_flat[k];
            for (int j = 0; j < 7; j++) counts_out[at * 7 + j] = s_cnt[k * 7 + j];
            cov_out[at] = SqCovar::finish(&s_cnt[k * 7]);
        }
    };
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ti, tj;
        SqCovar::tile_of(k, nT, ti, tj);
        const int64_t v0 = (int64_t)ti * T, w0 = (int64_t)tj * T;    // (v0 + 31, w0 + 31 < Lpad: a multiple of 64 >= L)
        int32_t cnt[4][7] = {};
        for (int64_t wb = 0; wb < W; wb += CH) {
            __syncthreads();                                         // (the last chunk has been read)
            for (int i = tid; i < SQ_COV_PLANES * CH * T; i += 256) {
                const int p = i / (CH * T), wd = i / T % CH, col = i % T;
                const bool have = wb + wd < W;
                s_v[p][wd][col] = have ? plane[SqCovar::at(p, wb + wd, v0 + col, W, Lpad)] : 0ull;
                s_w[p][wd][col] = have ? plane[SqCovar::at(p, wb + wd, w0 + col, W, Lpad)] : 0ull;
            }
            __syncthreads();
#pragma unroll 2
            for (int wd = 0; wd < CH; wd++) {
                uint64_t b[SQ_COV_PLANES];
                for (int p = 0; p < SQ_COV_PLANES; p++) b[p] = s_w[p][wd][wl];
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    uint64_t a[SQ_COV_PLANES];
                    for (int p = 0; p < SQ_COV_PLANES; p++) a[p] = s_v[p][wd][vl + c];
                    SqCovar::accumulate(a, b, cnt[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int64_t v = v0 + vl + c, w = w0 + wl;
            const bool hit = SqCovar::in_scope(v, w, L, minspan) && SqCovar::emits(cnt[c], SqCovar::finish(cnt[c]), min_rows, min_cov);
            const uint32_t at = em.slot(hit);
            if (hit) {
                s_flat[at] = (long long)(v * L + w);
                for (int j = 0; j < 7; j++) s_cnt[at * 7 + j] = cnt[c][j];
            }
            em.step(out, write);
        }
    }
    em.finish(out, write);
}

// Given pairs: one lane per pair, the planes' words read from global memory (two words of each plane per 64 rows, 8 bytes
// each, whatever the neighbouring lane reads: bound by latency, not by bandwidth; the scan is the hot path).  A pair that is
// not v < w inside the L columns gets an all-zero record and status 2.
extern "C" __global__ __launch_bounds__(256) void sq_covar_pairs_kernel(const uint64_t *plane, int32_t R, int32_t L, const int32_t *pairs,
                                                                       long long P, int32_t *counts_out, long long *cov_out,
                                                                       unsigned long long *out)
{
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < P; k += (int64_t)gridDim.x * 256) {
        const int32_t v = pairs[2 * k], w = pairs[2 * k + 1];
        int32_t cnt[7] = {};
        if (!SqCovar::valid_pair(v, w, L)) out[1] = 2ull;
        else
            for (int64_t wd = 0; wd < W; wd++) {
                uint64_t a[SQ_COV_PLANES], b[SQ_COV_PLANES];
                for (int p = 0; p < SQ_COV_PLANES; p++) {
                    a[p] = plane[SqCovar::at(p, wd, v, W, Lpad)];
                    b[p] = plane[SqCovar::at(p, wd, w, W, Lpad)];
                }
                SqCovar::accumulate(a, b, cnt);
            }
        for (int j = 0; j < 7; j++) counts_out[k * 7 + j] = cnt[j];
        cov_out[k] = SqCovar::finish(cnt);
    }
}

extern "C" size_t sq_covariation_scratch(int32_t R, int32_t L)
{
    return R < 1 || L < 1 ? 0 : (size_t)SqCovar::plane_words(R, L) * sizeof(uint64_t);
}

// The checks both entries share, and the planes of the rows in d_scratch (sq_covar_planes.h: sq_covar_stat_dev.hip calls it too).
int covar_planes(const char *who, const uint8_t *d_rows, int32_t R, int32_t L, void *d_scratch, size_t scratch_bytes,
                 uint64_t *d_out, hipStream_t st)
{
    if (!d_rows || !d_scratch || !d_out || R < 1 || L < 1) {
        sq_set_error(std::string(who) + ": bad argument");
        return -1;
    }
    const int64_t blocks = SqCovar::words(R) * (SqCovar::lpad(L) / 64);
    if (blocks > 0x7fffffffll) {
        sq_set_error(std::string(who) + ": more than 2^31 tiles of 64 rows x 64 columns");
        return -1;
    }
    if (scratch_bytes < sq_covariation_scratch(R, L)) {
        sq_set_error(std::string(who) + ": scratch too small");
        return -1;
    }
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    hipLaunchKernelGGL(sq_covar_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                       d_rows, R, L, (uint64_t *)d_scratch);
    return sq_check(hipGetLastError(), "sq_covar_planes_kernel");
}

extern "C" int sq_covariation_scan(const uint8_t *d_rows, int32_t R, int32_t L, int32_t minspan, int32_t min_rows, int64_t min_cov,
                                   void *d_scratch, size_t scratch_bytes, int64_t *d_flat, int32_t *d_counts, int64_t *d_cov, int64_t cap,
                                   uint64_t *d_out, void *hip_stream)
{
    if (minspan < 0 || min_rows < 0 || min_cov < 0 || cap < 0 || (cap && (!d_flat || !d_counts || !d_cov))) {
        sq_set_error("sq_covariation_scan: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = covar_planes("sq_covariation_scan", d_rows, R, L, d_scratch, scratch_bytes, d_out, st)) return rc;
    // At most SQ_COV_MAX_BLOCKS = 2048 blocks, the rest by grid stride: 8 blocks of 4 waves fill the 32 wave slots of each of
    // the 256 CUs, so 2048 blocks are more than the chip holds at once (the kernel's 46 KB of LDS admit three per CU) and a larger grid
    // would only queue behind them.
    const int64_t nT = ((int64_t)L + SQ_COV_TILE - 1) / SQ_COV_TILE;
    const unsigned blocks = (unsigned)std::min<int64_t>(SqCovar::tile_count(nT), SQ_COV_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_scan_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)d_scratch, R, L, minspan, min_rows,
                       (long long)min_cov, (long long *)d_flat, d_counts, (long long *)d_cov, (long long)cap, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_covar_scan_kernel");
}

extern "C" int sq_covariation_pairs(const uint8_t *d_rows, int32_t R, int32_t L, const int32_t *d_pairs, int64_t P, void *d_scratch,
                                    size_t scratch_bytes, int32_t *d_counts, int64_t *d_cov, uint64_t *d_out, void *hip_stream)
{
    if (P < 0 || (P && (!d_pairs || !d_counts || !d_cov))) {
        sq_set_error("sq_covariation_pairs: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = covar_planes("sq_covariation_pairs", d_rows, R, L, d_scratch, scratch_bytes, d_out, st)) return rc;
    if (!P) return 0;
    const unsigned blocks = (unsigned)std::min<int64_t>((P + 255) / 256, SQ_COV_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)d_scratch, R, L, d_pairs, (long long)P,
                       d_counts, (long long *)d_cov, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_covar_pairs_kernel");
}
