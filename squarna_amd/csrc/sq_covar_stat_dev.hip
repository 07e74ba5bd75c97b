// Covariation statistics of alignment columns (CovariationStatistics): MI, the G-test or chi-square of the joint table of every
// pair of columns, raw and corrected by the column means, on the device.  Definitions, layout and predicates: sq_covar_stat.h.
//
//   sq_covar_planes_kernel         (sq_covar_dev.hip) the rows as bit planes; the planes A, C, G, U are read here
//   sq_covar_stat_sums_kernel      pass 1: S of every cell v < w, tile by tile from LDS, reduced per tile along both axes into
//                                  partial column sums, one writer per (tile, column)
//   sq_covar_stat_reduce_kernel    a column's partials in ascending tile order: mean[c]
//   sq_covar_stat_total_kernel     mean_all from mean[], one block, a fixed order
//   sq_covar_stat_scan_kernel      pass 2: the counters and S again (cheaper than an L x L store), C, and the cells that pass the
//                                  thresholds through the block's emission stage (sq_emit.h)
//   sq_covar_stat_pairs_kernel     the same record for given column pairs, one lane per pair from global memory
// and for the shuffled-column null of these statistics (CovariationStatisticsSignificance; definitions: sq_covar_stat_null.h),
// on the planes that sq_covar_null_planes_kernel (sq_covar_null_dev.hip) forms for a batch of samples:
//   the three pass-1 kernels       per sample, on its planes: its column means
//   sq_covar_stat_null_scan_kernel pass 2 per sample of the batch; a cell leaves no record: its C is binned against the observed
//                                  values and folded into the sample's maximum
//   sq_covar_stat_null_pairs_kernel  one lane per (observed pair, sample): does the same cell reach the observed value?
//   sq_covar_stat_null_max_kernel  the samples' maxima from integer keys to doubles
//
// No float atomics: every sum has one fixed order, so two calls give the same bits.  All buffers are the caller's device
// memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_covar_stat.h"
#include "sq_covar_stat_null.h"
#include "sq_covar_planes.h"
#include "sq_emit.h"
#include <cmath>

namespace {

constexpr int T = SQ_COVSTAT_TILE, CH = SQ_COVSTAT_WORD_CHUNK, CELLS = SQ_COVSTAT_CELLS, PASSES = 4 / CELLS;
static_assert(T == 32 && SQ_EMIT_BLOCK == 256 && CELLS * PASSES == 4, "a tile is four cells per thread of a 256-thread block");

struct StatPlanesLds {
    uint64_t v[4][CH][T], w[4][CH][T];                              // the planes A C G U of the tile's two column ranges
};

// A tile of 32 x 32 cells is walked in PASSES = 4 / CELLS passes of 32 / PASSES rows of cells each; in a pass thread t has
// the CELLS cells w = w0 + t % 32, v = v0 + vl .. vl + CELLS - 1 with vl = pass * (32 / PASSES) + CELLS * (t / 32), and keeps
// their 16 counters each in registers (half a wave reads 32 consecutive words of the w planes, and one word of the v planes as a
// broadcast, as sq_covar_scan_kernel).  CELLS = 2 (sq_covar_stat.h says why): the tile's planes are staged twice.
// tile_counters() is one pass: per CH words of rows the planes of both column ranges are staged in LDS; words beyond W are
// staged as zero, so every trip count is block-uniform.  v0 + 31, w0 + 31 < Lpad (a multiple of 64 >= L).
__device__ __forceinline__ void tile_counters(const uint64_t *plane, int64_t W, int64_t Lpad, int64_t v0, int64_t w0, StatPlanesLds &s,
                                              int vl, int32_t cnt[CELLS][16])
{
    const int tid = threadIdx.x, wl = tid & 31;
    for (int64_t wb = 0; wb < W; wb += CH) {
        __syncthreads();                                             // (the last chunk has been read)
        for (int i = tid; i < 4 * CH * T; i += 256) {
            const int p = i / (CH * T), wd = i / T % CH, col = i % T;
            const bool have = wb + wd < W;
            s.v[p][wd][col] = have ? plane[SqCovar::at(p, wb + wd, v0 + col, W, Lpad)] : 0ull;
            s.w[p][wd][col] = have ? plane[SqCovar::at(p, wb + wd, w0 + col, W, Lpad)] : 0ull;
        }
        __syncthreads();
        for (int wd = 0; wd < CH; wd++) {
            uint64_t b[4];
            for (int p = 0; p < 4; p++) b[p] = s.w[p][wd][wl];
#pragma unroll
            for (int c = 0; c < CELLS; c++) {
                uint64_t a[4];
                for (int p = 0; p < 4; p++) a[p] = s.v[p][wd][vl + c];
                SqCovarStat::accumulate(a, b, cnt[c]);
            }
        }
    }
}

// The 16 counters of one cell from global memory (the pairs lookup, and the scan's flush for the records it writes).
__device__ __forceinline__ void cell_counters(const uint64_t *plane, int64_t W, int64_t Lpad, int64_t v, int64_t w, int32_t n[16])
{
    for (int k = 0; k < 16; k++) n[k] = 0;
    for (int64_t wd = 0; wd < W; wd++) {
        uint64_t a[4], b[4];
        for (int p = 0; p < 4; p++) {
            a[p] = plane[SqCovar::at(p, wd, v, W, Lpad)];
            b[p] = plane[SqCovar::at(p, wd, w, W, Lpad)];
        }
        SqCovarStat::accumulate(a, b, n);
    }
}

}  // namespace

// Pass 1.  A block takes the upper-triangle tiles k = blockIdx.x, + gridDim.x, ... (SqCovar::tile_of).  S of the tile's cells
// v < w < L (0.0 elsewhere) goes to LDS; then thread t < 32 adds row t of the tile over w ascending (what the tile gives to
// sum[v0 + t]) and thread 32 + t column t over v ascending (to sum[w0 + t]).  Tile (ti, tj) writes the row sums to
// partial[tj][v0 + t] and the column sums to partial[ti][w0 + t]; the diagonal tile writes row + column to partial[ti][v0 + t].
// So slot (t, c) of partial[nT][Lpad], c < nT * 32 <= Lpad, has exactly one writer, the tile that column c's range shares with
// range t, and every such slot is written: nothing is cleared beforehand.
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_sums_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t stat,
                                                                           double *partial)
{
    __shared__ StatPlanesLds s_pl;
    __shared__ double s_S[T][T + 1], s_row[T], s_col[T];
    const int tid = threadIdx.x, wl = tid & 31;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t nT = SqCovarStat::tiles(L), ntiles = SqCovar::tile_count(nT);
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ti, tj;
        SqCovar::tile_of(k, nT, ti, tj);
        const int64_t v0 = (int64_t)ti * T, w0 = (int64_t)tj * T;
        for (int pass = 0; pass < PASSES; pass++) {
            const int vl = pass * (T / PASSES) + (tid >> 5) * CELLS;
            int32_t cnt[CELLS][16] = {};
            tile_counters(plane, W, Lpad, v0, w0, s_pl, vl, cnt);
#pragma unroll
            for (int c = 0; c < CELLS; c++) {
                const int64_t v = v0 + vl + c, w = w0 + wl;
                s_S[vl + c][wl] = v < w && w < L ? SqCovarStat::raw(stat, cnt[c]) : 0.0;
            }
        }
        __syncthreads();
        if (tid < 2 * T) {
            const int t = tid & (T - 1);
            double sum = 0.0;
            if (tid < T) for (int j = 0; j < T; j++) sum += s_S[t][j];
            else for (int j = 0; j < T; j++) sum += s_S[j][t];
            (tid < T ? s_row : s_col)[t] = sum;
        }
        __syncthreads();
        if (tid < T) {
            if (ti == tj) partial[(int64_t)ti * Lpad + v0 + tid] = s_row[tid] + s_col[tid];
            else {
                partial[(int64_t)tj * Lpad + v0 + tid] = s_row[tid];
                partial[(int64_t)ti * Lpad + w0 + tid] = s_col[tid];
            }
        }
        // (the next tile's first barrier, in tile_counters, comes before anything of s_S, s_row or s_col is written again)
    }
}

// mean[c] = (the partials of column c in ascending tile order) / (L - 1), one thread per column c < L; 0 with L == 1.
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_reduce_kernel(const double *partial, int32_t L, double *mean)
{
    const int64_t Lpad = SqCovar::lpad(L), nT = SqCovarStat::tiles(L);
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= L) return;
    double sum = 0.0;
    for (int64_t t = 0; t < nT; t++) sum += partial[t * Lpad + c];
    mean[c] = L > 1 ? sum / (double)(L - 1) : 0.0;
}

// mean[L] = mean_all = (the sum of mean[c]) / L: one block; thread t adds the columns t, t + 256, ... ascending, thread 0 the
// 256 runs ascending.
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_total_kernel(int32_t L, double *mean)
{
    __shared__ double s_run[256];
    double sum = 0.0;
    for (int64_t c = threadIdx.x; c < L; c += 256) sum += mean[c];
    s_run[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double all = 0.0;
        for (int t = 0; t < 256; t++) all += s_run[t];
        mean[L] = all / (double)L;
    }
}

// Pass 2: the same tile walk and the same counters.  A cell in scope (v < w < L, w - v >= minspan) with N >= min_rows gets
// S and C; one that also has C >= min_stat is a hit.  The stage keeps a hit's flat index and S (16 bytes; with the 64 bytes
// of counters a stage of SQ_EMIT_STAGE records would be 72 KB and admit one block per CU); the flush forms the counters of the
// records it stores again from global memory (cell_counters: integers, the same numbers) and C again from S and the means (the same function
// of the same numbers: the same bits).  mean = null with corr == SQ_COVSTAT_NONE.  One slot() + step() per cell index of the
// thread (sq_emit.h's contract: at most 256 records a step).
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_scan_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t stat,
                                                                           int32_t corr, int32_t minspan, int32_t min_rows, double min_stat,
                                                                           const double *mean, long long *flat_out, int32_t *joint_out,
                                                                           double *raw_out, double *value_out, long long cap,
                                                                           unsigned long long *out)
{
    __shared__ StatPlanesLds s_pl;
    __shared__ long long s_flat[SQ_EMIT_STAGE];
    __shared__ double s_raw[SQ_EMIT_STAGE];
    __shared__ SqEmitStage em;
    const int tid = threadIdx.x, wl = tid & 31;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t nT = SqCovarStat::tiles(L), ntiles = SqCovar::tile_count(nT);
    const double mean_all = corr != SQ_COVSTAT_NONE ? mean[L] : 0.0;
    em.init();
    auto write = [&](uint32_t k, unsigned long long at) {
        if ((long long)at < cap) {
            const long long flat = s_flat[k];
            const int64_t v = flat / L, w = flat % L;                // (a staged cell: v < w < L)
            int32_t n[16];
            cell_counters(plane, W, Lpad, v, w, n);
            flat_out[at] = flat;
            for (int j = 0; j < 16; j++) joint_out[at * 16 + j] = n[j];
            raw_out[at] = s_raw[k];
            value_out[at] = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, s_raw[k], mean[v], mean[w], mean_all) : s_raw[k];
        }
    };
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ti, tj;
        SqCovar::tile_of(k, nT, ti, tj);
        const int64_t v0 = (int64_t)ti * T, w0 = (int64_t)tj * T;
        for (int pass = 0; pass < PASSES; pass++) {
            const int vl = pass * (T / PASSES) + (tid >> 5) * CELLS;
            int32_t cnt[CELLS][16] = {};
            tile_counters(plane, W, Lpad, v0, w0, s_pl, vl, cnt);
#pragma unroll
            for (int c = 0; c < CELLS; c++) {
                const int64_t v = v0 + vl + c, w = w0 + wl;
                const int64_t N = SqCovarStat::rows(cnt[c]);
                bool hit = SqCovar::in_scope(v, w, L, minspan) && N >= min_rows;     // (else no S: the logarithms are the cost)
                double S = 0.0;
                if (hit) {
                    S = SqCovarStat::raw(stat, cnt[c]);
                    const double C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mean[v], mean[w], mean_all) : S;
                    hit = SqCovarStat::emits(N, C, min_rows, min_stat);
                }
                const uint32_t at = em.slot(hit);
                if (hit) {
                    s_flat[at] = (long long)(v * L + w);
                    s_raw[at] = S;
                }
                em.step(out, write);
            }
        }
    }
    em.finish(out, write);
}

// Given pairs: one lane per pair, the planes' words read from global memory.  A pair that is not v < w inside the L columns
// gets an all-zero record and status 2.
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_pairs_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t stat,
                                                                            int32_t corr, const double *mean, const int32_t *pairs,
                                                                            long long P, int32_t *joint_out, double *raw_out,
                                                                            double *value_out, unsigned long long *out)
{
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < P; k += (int64_t)gridDim.x * 256) {
        const int32_t v = pairs[2 * k], w = pairs[2 * k + 1];
        int32_t n[16] = {};
        double S = 0.0, C = 0.0;
        if (!SqCovar::valid_pair(v, w, L)) out[1] = 2ull;
        else {
            cell_counters(plane, W, Lpad, v, w, n);
            S = SqCovarStat::raw(stat, n);
            C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mean[v], mean[w], mean[L]) : S;
        }
        for (int j = 0; j < 16; j++) joint_out[k * 16 + j] = n[j];
        raw_out[k] = S;
        value_out[k] = C;
    }
}

extern "C" size_t sq_covariation_stat_scratch(int32_t R, int32_t L)
{
    return R < 1 || L < 1 ? 0 : (size_t)SqCovarStat::scratch_words(R, L) * 8;
}

// The two reductions behind a pass 1: d_mean[0 .. L] from its partial column sums (sq_covar_planes.h: the weighted entries of
// sq_covar_wstat_dev.hip end their pass 1 with the same two kernels).
int covar_stat_means(const double *partial, int32_t L, double *d_mean, hipStream_t st)
{
    hipLaunchKernelGGL(sq_covar_stat_reduce_kernel, dim3((unsigned)(((int64_t)L + 255) / 256)), dim3(256), 0, st, partial, L, d_mean);
    if (int rc = sq_check(hipGetLastError(), "sq_covar_stat_reduce_kernel")) return rc;
    hipLaunchKernelGGL(sq_covar_stat_total_kernel, dim3(1), dim3(256), 0, st, L, d_mean);
    return sq_check(hipGetLastError(), "sq_covar_stat_total_kernel");
}

// The checks both entries share; then the planes in d_scratch and, with a correction, pass 1 and the two reductions: d_mean.
static int stat_open(const char *who, const uint8_t *d_rows, int32_t R, int32_t L, int32_t stat, int32_t corr, void *d_scratch,
                     size_t scratch_bytes, double *d_mean, uint64_t *d_out, hipStream_t st)
{
    if (stat < 0 || stat >= SQ_COVSTAT_STATS || corr < 0 || corr >= SQ_COVSTAT_CORRECTIONS || (corr != SQ_COVSTAT_NONE && !d_mean)) {
        sq_set_error(std::string(who) + ": bad argument");
        return -1;
    }
    if (R >= 1 && L >= 1 && scratch_bytes < sq_covariation_stat_scratch(R, L)) {
        sq_set_error(std::string(who) + ": scratch too small");
        return -1;
    }
    if (int rc = covar_planes(who, d_rows, R, L, d_scratch, scratch_bytes, d_out, st)) return rc;
    if (corr == SQ_COVSTAT_NONE) return 0;
    const uint64_t *plane = (const uint64_t *)d_scratch;
    double *partial = (double *)d_scratch + SqCovar::plane_words(R, L);
    const unsigned blocks = (unsigned)std::min<int64_t>(SqCovar::tile_count(SqCovarStat::tiles(L)), SQ_COVSTAT_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_stat_sums_kernel, dim3(blocks), dim3(256), 0, st, plane, R, L, stat, partial);
    if (int rc = sq_check(hipGetLastError(), "sq_covar_stat_sums_kernel")) return rc;
    return covar_stat_means(partial, L, d_mean, st);
}

extern "C" int sq_covariation_stat_scan(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction, int32_t minspan,
                                        int32_t min_rows, double min_stat, void *d_scratch, size_t scratch_bytes, double *d_mean,
                                        int64_t *d_flat, int32_t *d_joint, double *d_raw, double *d_value, int64_t cap, uint64_t *d_out,
                                        void *hip_stream)
{
    if (minspan < 0 || min_rows < 0 || std::isnan(min_stat) || cap < 0 || (cap && (!d_flat || !d_joint || !d_raw || !d_value))) {
        sq_set_error("sq_covariation_stat_scan: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = stat_open("sq_covariation_stat_scan", d_rows, R, L, statistic, correction, d_scratch, scratch_bytes, d_mean, d_out, st))
        return rc;
    // At most SQ_COVSTAT_MAX_BLOCKS blocks, the rest by grid stride, as sq_covariation_scan.
    const unsigned blocks = (unsigned)std::min<int64_t>(SqCovar::tile_count(SqCovarStat::tiles(L)), SQ_COVSTAT_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_stat_scan_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)d_scratch, R, L, statistic, correction,
                       minspan, min_rows, min_stat, (const double *)d_mean, (long long *)d_flat, d_joint, d_raw, d_value, (long long)cap,
                       (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_covar_stat_scan_kernel");
}

extern "C" int sq_covariation_stat_pairs(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction,
                                         const int32_t *d_pairs, int64_t P, void *d_scratch, size_t scratch_bytes, double *d_mean,
                                         int32_t *d_joint, double *d_raw, double *d_value, uint64_t *d_out, void *hip_stream)
{
    if (P < 0 || (P && (!d_pairs || !d_joint || !d_raw || !d_value))) {
        sq_set_error("sq_covariation_stat_pairs: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = stat_open("sq_covariation_stat_pairs", d_rows, R, L, statistic, correction, d_scratch, scratch_bytes, d_mean, d_out, st))
        return rc;
    if (!P) return 0;
    const unsigned blocks = (unsigned)std::min<int64_t>((P + 255) / 256, SQ_COVSTAT_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_stat_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)d_scratch, R, L, statistic, correction,
                       (const double *)d_mean, d_pairs, (long long)P, d_joint, d_raw, d_value, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_covar_stat_pairs_kernel");
}

// ---- the shuffled-column null of the statistics (sq_covariation_stat_null; definitions: sq_covar_stat_null.h) ----------------
//
// The all-pairs scan of the batch's samples: blockIdx.y is the sample, blockIdx.x walks the tiles as pass 2 does (the same
// passes, the same thread-to-cell map, tile_counters()).  A cell in scope leaves no record: S = raw(), C = corrected() with
// the means of its own sample (mean + sample * (L + 1); not read with corr == SQ_COVSTAT_NONE), and C goes into bin() of the
// observed values and, as its integer key, into the thread's running maximum.  The lowest SQ_COVSTATNULL_LDS_BINS thresholds
// and bins lie in LDS, the others are read from and added to global memory.  A search starts with every lane at the same
// threshold (a broadcast) and spreads from there; the lanes of a wave then hit the banks as their values fall.  With few
// observed values above nearly every null cell (a scan with min_stat) the cells share bin 0: it is counted in a register,
// and a wave whose other cells share one bin adds once (as sq_covar_null_scan_kernel).  A block adds its counters to hist and
// its maximum to null_max[sample] once, when it has walked its tiles: integer atomics only, a few per block.
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_null_scan_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t stat,
                                                                                int32_t corr, int32_t minspan, const double *mean,
                                                                                const double *thresholds, long long U,
                                                                                unsigned long long *hist, unsigned long long *null_max)
{
    constexpr int NB = SQ_COVSTATNULL_LDS_BINS;
    __shared__ StatPlanesLds s_pl;
    __shared__ double s_T[NB];
    __shared__ uint32_t s_hist[NB];
    __shared__ unsigned long long s_max;
    const int tid = threadIdx.x, lane = tid & 63, wl = tid & 31;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t nT = SqCovarStat::tiles(L), ntiles = SqCovar::tile_count(nT);
    const int lds_bins = (int)(U + 1 < NB ? U + 1 : NB), lds_thr = (int)(U < NB ? U : NB);
    plane += (int64_t)blockIdx.y * SqCovar::plane_words(R, L);
    if (corr != SQ_COVSTAT_NONE) mean += (int64_t)blockIdx.y * ((int64_t)L + 1);
    const double mean_all = corr != SQ_COVSTAT_NONE ? mean[L] : 0.0;
    for (int i = tid; i < NB; i += 256) {
        s_hist[i] = 0u;
        if (i < lds_thr) s_T[i] = thresholds[i];
    }
    if (!tid) s_max = 0ull;
    __syncthreads();
    auto thr = [&](int64_t i) -> double { return i < NB ? s_T[i] : thresholds[i]; };
    auto add = [&](int64_t b, uint32_t many) {
        if (b < NB) atomicAdd(&s_hist[b], many);
        else atomicAdd(&hist[b], (unsigned long long)many);
    };
    const double t0 = U ? thr(0) : 0.0;
    uint32_t below = 0;                                              // this thread's cells of bin 0
    unsigned long long most = 0ull;                                  // (key 0: no cell yet)
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ti, tj;
        SqCovar::tile_of(k, nT, ti, tj);
        const int64_t v0 = (int64_t)ti * T, w0 = (int64_t)tj * T;
        for (int pass = 0; pass < PASSES; pass++) {
            const int vl = pass * (T / PASSES) + (tid >> 5) * CELLS;
            int32_t cnt[CELLS][16] = {};
            tile_counters(plane, W, Lpad, v0, w0, s_pl, vl, cnt);
#pragma unroll
            for (int c = 0; c < CELLS; c++) {
                const int64_t v = v0 + vl + c, w = w0 + wl;
                const bool live = SqCovar::in_scope(v, w, L, minspan);
                int64_t b = 0;
                if (live) {
                    const double S = SqCovarStat::raw(stat, cnt[c]);
                    const double C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mean[v], mean[w], mean_all) : S;
                    const unsigned long long key = SqCovarStatNull::key(C);
                    most = key > most ? key : most;
                    if (U && C >= t0) b = SqCovarStatNull::bin_by(thr, U, C);
                    below += b == 0;
                }
                const bool rest = live && b > 0;
                const unsigned long long m = __ballot(rest);
                if (m) {                                             // (wave-uniform)
                    const int first = __ffsll((unsigned long long)m) - 1;
                    const int64_t b_first = __shfl((long long)b, first);
                    if (__ballot(rest && b == b_first) == m) {
                        if (lane == first) add(b_first, (uint32_t)__popcll(m));
                    } else if (rest)
                        add(b, 1u);
                }
            }
        }
    }
    atomicAdd(&s_hist[0], below);
    atomicMax(&s_max, most);
    __syncthreads();
    for (int i = tid; i < lds_bins; i += 256)
        if (s_hist[i]) atomicAdd(&hist[i], (unsigned long long)s_hist[i]);
    if (!tid && s_max) atomicMax(&null_max[blockIdx.y], s_max);
}

// One lane per (pair, sample of the batch), the pair running fastest: C of the sample's planes and means at the pair, formed as
// sq_covar_stat_pairs_kernel forms it, and one more for own_ge[pair] when it reaches the observed value.  A pair that is not
// v < w inside the L columns counts nothing and leaves status 2.
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_null_pairs_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t stat,
                                                                                 int32_t corr, const double *mean, const int32_t *pairs,
                                                                                 const double *value, long long P, int32_t samples,
                                                                                 int32_t *own_ge, unsigned long long *out)
{
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L), per = SqCovar::plane_words(R, L);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < P * samples; k += (int64_t)gridDim.x * 256) {
        const int64_t at = k % P, sample = k / P;
        const int32_t v = pairs[2 * at], w = pairs[2 * at + 1];
        if (!SqCovar::valid_pair(v, w, L)) {
            out[1] = 2ull;
            continue;
        }
        int32_t n[16];
        cell_counters(plane + sample * per, W, Lpad, v, w, n);
        const double S = SqCovarStat::raw(stat, n);
        const double *mine = mean + sample * ((int64_t)L + 1);       // (not read without a correction)
        const double C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mine[v], mine[w], mine[L]) : S;
        if (C >= value[at]) atomicAdd(&own_ge[at], 1);
    }
}

// null_max[k]: from the key of the sample's largest C to that double, in place (key 0, no cell in scope: -infinity).
extern "C" __global__ __launch_bounds__(256) void sq_covar_stat_null_max_kernel(unsigned long long *null_max, int32_t K)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < K) null_max[k] = SqCovarStatNull::bits(SqCovarStatNull::unkey(null_max[k]));
}

// (sq_covar_planes.h: the weighted null of sq_covar_wstat_null_dev.hip ends with the same kernel)
int covar_stat_null_max(unsigned long long *d_key, int32_t K, hipStream_t st)
{
    hipLaunchKernelGGL(sq_covar_stat_null_max_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, d_key, K);
    return sq_check(hipGetLastError(), "sq_covar_stat_null_max_kernel");
}

extern "C" size_t sq_covariation_stat_null_scratch(int32_t R, int32_t L, int32_t batch)
{
    return R < 1 || L < 1 || batch < 1 ? 0 : (size_t)SqCovarStatNull::scratch_words(R, L, batch) * 8;
}

extern "C" int sq_covariation_stat_null(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction, int32_t minspan,
                                        const int32_t *d_pairs, const double *d_value, int64_t P, const double *d_thresholds, int64_t U,
                                        int32_t K, uint64_t seed, int32_t batch, void *d_scratch, size_t scratch_bytes, int64_t *d_hist,
                                        int32_t *d_own_ge, double *d_null_max, uint64_t *d_out, void *hip_stream)
{
    const std::string who("sq_covariation_stat_null");
    if (K < 1 || minspan < 0 || P < 0 || U < 0 || !d_hist || !d_null_max || !d_out || (P && (!d_pairs || !d_value || !d_own_ge)) ||
        (U && !d_thresholds) || statistic < 0 || statistic >= SQ_COVSTAT_STATS || correction < 0 || correction >= SQ_COVSTAT_CORRECTIONS ||
        !d_rows || !d_scratch || R < 1 || L < 1 || batch < 1 || batch > 65535) {
        sq_set_error(who + ": bad argument");
        return -1;
    }
    if (R > SQ_COVNULL_MAX_ROWS) {
        sq_set_error(who + ": more than " + std::to_string(SQ_COVNULL_MAX_ROWS) + " rows (SQ_COVNULL_MAX_ROWS: a column's sort keys lie in LDS)");
        return -1;
    }
    if (L > SQ_COVNULL_MAX_COLS || (int64_t)batch * SqCovar::lpad(L) > 0x7fffffffll) {
        sq_set_error(who + ": more than 2^21 columns, or more than 2^31 columns in a batch of samples");
        return -1;
    }
    if (scratch_bytes < sq_covariation_stat_null_scratch(R, L, batch)) {
        sq_set_error(who + ": scratch too small");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t per_plane = SqCovar::plane_words(R, L), per_partial = SqCovarStat::partial_words(L), per_mean = (int64_t)L + 1;
    uint64_t *d_plane = (uint64_t *)d_scratch;
    double *d_partial = (double *)(d_plane + (int64_t)batch * per_plane), *d_mean = d_partial + (int64_t)batch * per_partial;
    uint8_t *d_cls = (uint8_t *)(d_mean + (int64_t)batch * per_mean);
    unsigned long long *d_key = (unsigned long long *)d_null_max;    // (the samples' maxima as keys until the last kernel)
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    HIPCK(hipMemsetAsync(d_hist, 0, (size_t)(U + 1) * sizeof(int64_t), st));
    HIPCK(hipMemsetAsync(d_null_max, 0, (size_t)K * sizeof(double), st));
    if (P) HIPCK(hipMemsetAsync(d_own_ge, 0, (size_t)P * sizeof(int32_t), st));
    if (int rc = null_classes(d_rows, R, L, d_cls, st)) return rc;
    const int64_t ntiles = SqCovar::tile_count(SqCovarStat::tiles(L));
    const unsigned pass1 = (unsigned)std::min<int64_t>(ntiles, SQ_COVSTAT_MAX_BLOCKS);
    for (int32_t k0 = 0; k0 < K; k0 += batch) {
        const int32_t samples = std::min(batch, K - k0);
        if (int rc = null_planes(d_cls, R, L, seed, (uint64_t)k0, samples, d_plane, st)) return rc;
        // Pass 1 of every sample with the kernels and the grid of sq_covariation_stat_scan: the means have its bits.
        for (int32_t s = 0; correction != SQ_COVSTAT_NONE && s < samples; s++) {
            const uint64_t *plane = d_plane + s * per_plane;
            double *partial = d_partial + s * per_partial, *mean = d_mean + s * per_mean;
            hipLaunchKernelGGL(sq_covar_stat_sums_kernel, dim3(pass1), dim3(256), 0, st, plane, R, L, statistic, partial);
            if (int rc = sq_check(hipGetLastError(), "sq_covar_stat_sums_kernel")) return rc;
            if (int rc = covar_stat_means(partial, L, mean, st)) return rc;
        }
        // The scan's grid: the batch's samples times as many blocks as keep the whole grid near SQ_COVSTAT_MAX_BLOCKS; a block
        // walks the rest of its sample's tiles by grid stride.
        const unsigned per = (unsigned)std::min<int64_t>(ntiles, std::max<int64_t>(SQ_COVSTAT_MAX_BLOCKS / samples, 1));
        hipLaunchKernelGGL(sq_covar_stat_null_scan_kernel, dim3(per, (unsigned)samples), dim3(256), 0, st, (const uint64_t *)d_plane, R, L,
                           statistic, correction, minspan, (const double *)d_mean, d_thresholds, (long long)U, (unsigned long long *)d_hist,
                           d_key + k0);
        if (int rc = sq_check(hipGetLastError(), "sq_covar_stat_null_scan_kernel")) return rc;
        if (!P) continue;
        const unsigned blocks = (unsigned)std::min<int64_t>((P * samples + 255) / 256, SQ_COVSTAT_MAX_BLOCKS);
        hipLaunchKernelGGL(sq_covar_stat_null_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)d_plane, R, L, statistic,
                           correction, (const double *)d_mean, d_pairs, d_value, (long long)P, samples, d_own_ge,
                           (unsigned long long *)d_out);
        if (int rc = sq_check(hipGetLastError(), "sq_covar_stat_null_pairs_kernel")) return rc;
    }
    return covar_stat_null_max(d_key, K, st);
}
