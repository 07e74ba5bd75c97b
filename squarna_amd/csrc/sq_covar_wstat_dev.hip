// Covariation statistics of alignment columns with a weight per row (CovariationStatistics(weights=)): the joint table of two
// columns as sums of fixed-point row weights, MI, the G-test or chi-square of it, raw and corrected by the column means, on the
// device.  Definitions, the LDS layout and the predicates: sq_covar_wstat.h.
//
//   sq_covar_planes_kernel           (sq_covar_dev.hip) the rows as bit planes; the planes A, C, G, U are read here
//   sq_covar_wstat_quantise_kernel   the weights as uint32 q, zero beyond R up to a chunk of rows; status 3 on a bad weight
//   sq_covar_wstat_sums_kernel       pass 1: S of every cell v < w, tile by tile, reduced per tile into partial column sums as
//                                    sq_covar_stat_sums_kernel reduces them
//   sq_covar_stat_reduce_kernel, sq_covar_stat_total_kernel   (sq_covar_stat_dev.hip) the means, as they are
//   sq_covar_wstat_scan_kernel       pass 2: the counters and S again, C, and the cells that pass the thresholds through the
//                                    block's emission stage (sq_emit.h)
//   sq_covar_wstat_pairs_kernel      the same record for given column pairs, one lane per pair from global memory
//
// A popcount cannot weigh a row, so a thread walks the rows of its cell: the 16 int64 counters of the cell lie in LDS as
// bins[k][tid] (SqCovarWstat::accumulate), a thread has one cell at a time and a tile takes four passes.  The sums are integer:
// no float atomics, and the float sums have the fixed order of sq_covar_stat_dev.hip, so two calls give the same bits.  All
// buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_covar_wstat_dev.h"
#include "sq_covar_planes.h"
#include "sq_emit.h"
#include <cmath>

namespace {

constexpr int T = SQ_COVSTAT_TILE, CH = SQ_COVSTAT_WORD_CHUNK, PASSES = 4;
static_assert(T == 32 && SQ_EMIT_BLOCK == 256 && 64 * CH == 256, "a tile is four cells per thread of a 256-thread block, a chunk one row per thread");
static_assert(SQ_EMIT_STAGE == SQ_COVWSTAT_STAGE && sizeof(SqEmitStage) <= SQ_COVWSTAT_EMIT_BYTES, "sq_covar_wstat_lds() places sq_emit.h's stage");
static_assert(sizeof(long long) == sizeof(int64_t), "the stage's flat indices");
// (the staged planes of a tile, tile_bins() and cell_bins(): sq_covar_wstat_dev.h)

}  // namespace

// q[r] of w[r] for r < R, 0 for R <= r < Rpad; out[1] = 3 when a weight is not a finite number in 0 .. 2048 (its q is 0).
extern "C" __global__ __launch_bounds__(256) void sq_covar_wstat_quantise_kernel(const double *w, int32_t R, int64_t Rpad, uint32_t *q,
                                                                                unsigned long long *out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= Rpad) return;
    uint32_t mine = 0u;
    if (r < R && !SqCovarWstat::quantise(w[r], mine)) atomicMax(&out[1], 3ull);
    q[r] = mine;
}

// Pass 1: the tile walk, the thread-to-cell map of a pass (one cell: v = v0 + pass * 8 + tid / 32, w = w0 + tid % 32), the
// reduction of the tile's S along both axes and the one writer per slot of partial[] are those of sq_covar_stat_sums_kernel.
extern "C" __global__ __launch_bounds__(256) void sq_covar_wstat_sums_kernel(const uint64_t *plane, const uint32_t *q, int32_t R, int32_t L,
                                                                            int32_t stat, double *partial)
{
    const SqCovarWstatLds lds = sq_covar_wstat_lds(SQ_COVWSTAT_LDS_SUMS);
    WstatPlanesLds &s_pl = *reinterpret_cast<WstatPlanesLds *>(s_dyn + lds.planes);
    uint32_t *s_q = reinterpret_cast<uint32_t *>(s_dyn + lds.q);
    int64_t *bins = reinterpret_cast<int64_t *>(s_dyn + lds.bins) + threadIdx.x;
    double (*s_S)[T + 1] = reinterpret_cast<double (*)[T + 1]>(s_dyn + lds.S);
    double *s_row = reinterpret_cast<double *>(s_dyn + lds.row), *s_col = reinterpret_cast<double *>(s_dyn + lds.col);
    const int tid = threadIdx.x, wl = tid & 31;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t nT = SqCovarStat::tiles(L), ntiles = SqCovar::tile_count(nT);
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ti, tj;
        SqCovar::tile_of(k, nT, ti, tj);
        const int64_t v0 = (int64_t)ti * T, w0 = (int64_t)tj * T;
        for (int pass = 0; pass < PASSES; pass++) {
            const int vl = pass * (T / PASSES) + (tid >> 5);
            int64_t Q[16];
            tile_bins(plane, q, W, Lpad, v0, w0, s_pl, s_q, vl, bins, Q);
            const int64_t v = v0 + vl, w = w0 + wl;
            s_S[vl][wl] = v < w && w < L ? SqCovarWstat::raw_w(stat, Q) : 0.0;
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
        // (the next tile's first barrier, in tile_bins, comes before anything of s_S, s_row or s_col is written again)
    }
}

// Pass 2: the same walk and the same counters.  A cell in scope with X_N >= min_rows gets S and C; one that also has
// C >= min_stat is a hit.  The stage keeps a hit's flat index and S; the flush forms the counters of the records it stores
// again from global memory (cell_bins: integers, the same numbers) and C again from S and the means (the same function of the
// same numbers: the same bits), as sq_covar_stat_scan_kernel.  mean = null with corr == SQ_COVSTAT_NONE.  One slot() +
// step() per cell of the thread.
extern "C" __global__ __launch_bounds__(256) void sq_covar_wstat_scan_kernel(const uint64_t *plane, const uint32_t *q, int32_t R, int32_t L,
                                                                            int32_t stat, int32_t corr, int32_t minspan, double min_rows,
                                                                            double min_stat, const double *mean, long long *flat_out,
                                                                            long long *joint_out, double *raw_out, double *value_out,
                                                                            long long cap, unsigned long long *out)
{
    const SqCovarWstatLds lds = sq_covar_wstat_lds(SQ_COVWSTAT_LDS_SCAN);
    WstatPlanesLds &s_pl = *reinterpret_cast<WstatPlanesLds *>(s_dyn + lds.planes);
    uint32_t *s_q = reinterpret_cast<uint32_t *>(s_dyn + lds.q);
    int64_t *bins = reinterpret_cast<int64_t *>(s_dyn + lds.bins) + threadIdx.x;
    long long *s_flat = reinterpret_cast<long long *>(s_dyn + lds.flat);
    double *s_raw = reinterpret_cast<double *>(s_dyn + lds.raw);
    SqEmitStage &em = *reinterpret_cast<SqEmitStage *>(s_dyn + lds.em);
    const int tid = threadIdx.x, wl = tid & 31;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t nT = SqCovarStat::tiles(L), ntiles = SqCovar::tile_count(nT);
    const double mean_all = corr != SQ_COVSTAT_NONE ? mean[L] : 0.0;
    em.init();
    auto write = [&](uint32_t k, unsigned long long at) {
        if ((long long)at < cap) {
            const long long flat = s_flat[k];
            const int64_t v = flat / L, w = flat % L;                // (a staged cell: v < w < L)
            int64_t Q[16];
            cell_bins(plane, q, W, Lpad, v, w, bins, Q);
            flat_out[at] = flat;
            for (int j = 0; j < 16; j++) joint_out[at * 16 + j] = Q[j];
            raw_out[at] = s_raw[k];
            value_out[at] = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, s_raw[k], mean[v], mean[w], mean_all) : s_raw[k];
        }
    };
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ti, tj;
        SqCovar::tile_of(k, nT, ti, tj);
        const int64_t v0 = (int64_t)ti * T, w0 = (int64_t)tj * T;
        for (int pass = 0; pass < PASSES; pass++) {
            const int vl = pass * (T / PASSES) + (tid >> 5);
            int64_t Q[16];
            tile_bins(plane, q, W, Lpad, v0, w0, s_pl, s_q, vl, bins, Q);
            const int64_t v = v0 + vl, w = w0 + wl;
            const double XN = SqCovarWstat::rows(SqCovarWstat::total(Q));
            bool hit = SqCovar::in_scope(v, w, L, minspan) && XN >= min_rows;        // (else no S: the logarithms are the cost)
            double S = 0.0;
            if (hit) {
                S = SqCovarWstat::raw_w(stat, Q);
                const double C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mean[v], mean[w], mean_all) : S;
                hit = SqCovarWstat::emits_w(XN, C, min_rows, min_stat);
            }
            const uint32_t at = em.slot(hit);
            if (hit) {
                s_flat[at] = (long long)(v * L + w);
                s_raw[at] = S;
            }
            em.step(out, write);
        }
    }
    em.finish(out, write);
}

// Given pairs: one lane per pair, the planes' words and the weights read from global memory, the bins in LDS.  A pair that is
// not v < w inside the L columns gets an all-zero record and status 2 (a status 3 of the weights stays).
extern "C" __global__ __launch_bounds__(256) void sq_covar_wstat_pairs_kernel(const uint64_t *plane, const uint32_t *q, int32_t R, int32_t L,
                                                                             int32_t stat, int32_t corr, const double *mean,
                                                                             const int32_t *pairs, long long P, long long *joint_out,
                                                                             double *raw_out, double *value_out, unsigned long long *out)
{
    const SqCovarWstatLds lds = sq_covar_wstat_lds(SQ_COVWSTAT_LDS_PAIRS);
    int64_t *bins = reinterpret_cast<int64_t *>(s_dyn + lds.bins) + threadIdx.x;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < P; k += (int64_t)gridDim.x * 256) {
        const int32_t v = pairs[2 * k], w = pairs[2 * k + 1];
        int64_t Q[16] = {};
        double S = 0.0, C = 0.0;
        if (!SqCovar::valid_pair(v, w, L)) atomicMax(&out[1], 2ull);
        else {
            cell_bins(plane, q, W, Lpad, v, w, bins, Q);
            S = SqCovarWstat::raw_w(stat, Q);
            C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mean[v], mean[w], mean[L]) : S;
        }
        for (int j = 0; j < 16; j++) joint_out[k * 16 + j] = Q[j];
        raw_out[k] = S;
        value_out[k] = C;
    }
}

extern "C" size_t sq_covariation_wstat_scratch(int32_t R, int32_t L)
{
    return R < 1 || L < 1 ? 0 : (size_t)SqCovarWstat::scratch_words(R, L) * 8;
}

// The two launches the weighted null shares with the entries here (sq_covar_planes.h): q[rpad(R)] of the weights, and pass 1
// of one alignment's planes.
int covar_wstat_quantise(const double *d_weights, int32_t R, uint32_t *d_q, uint64_t *d_out, hipStream_t st)
{
    const int64_t Rpad = SqCovarWstat::rpad(R);
    hipLaunchKernelGGL(sq_covar_wstat_quantise_kernel, dim3((unsigned)(Rpad / 256)), dim3(256), 0, st, d_weights, R, Rpad, d_q,
                       (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_covar_wstat_quantise_kernel");
}

int covar_wstat_sums(const uint64_t *d_plane, const uint32_t *d_q, int32_t R, int32_t L, int32_t stat, double *d_partial, hipStream_t st)
{
    const unsigned blocks = (unsigned)std::min<int64_t>(SqCovar::tile_count(SqCovarStat::tiles(L)), SQ_COVSTAT_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_wstat_sums_kernel, dim3(blocks), dim3(256), sq_covar_wstat_lds(SQ_COVWSTAT_LDS_SUMS).total, st, d_plane, d_q, R,
                       L, stat, d_partial);
    return sq_check(hipGetLastError(), "sq_covar_wstat_sums_kernel");
}

// The checks both entries share; then the planes and q in d_scratch and, with a correction, pass 1 and the two reductions:
// d_mean.
static int wstat_open(const char *who, const uint8_t *d_rows, int32_t R, int32_t L, const double *d_weights, int32_t stat, int32_t corr,
                      void *d_scratch, size_t scratch_bytes, double *d_mean, uint64_t *d_out, hipStream_t st)
{
    if (!d_weights || stat < 0 || stat >= SQ_COVSTAT_STATS || corr < 0 || corr >= SQ_COVSTAT_CORRECTIONS ||
        (corr != SQ_COVSTAT_NONE && !d_mean)) {
        sq_set_error(std::string(who) + ": bad argument");
        return -1;
    }
    if (R > SQ_COVWSTAT_MAX_ROWS) {
        sq_set_error(std::string(who) + ": more than 2^22 rows (SQ_COVWSTAT_MAX_ROWS: the weighted sums stay exact doubles)");
        return -1;
    }
    if (R >= 1 && L >= 1 && scratch_bytes < sq_covariation_wstat_scratch(R, L)) {
        sq_set_error(std::string(who) + ": scratch too small");
        return -1;
    }
    if (int rc = covar_planes(who, d_rows, R, L, d_scratch, scratch_bytes, d_out, st)) return rc;
    const uint64_t *plane = (const uint64_t *)d_scratch;
    uint32_t *q = (uint32_t *)((uint64_t *)d_scratch + SqCovarWstat::q_at(R, L));
    if (int rc = covar_wstat_quantise(d_weights, R, q, d_out, st)) return rc;
    if (corr == SQ_COVSTAT_NONE) return 0;
    double *partial = (double *)d_scratch + SqCovar::plane_words(R, L);
    if (int rc = covar_wstat_sums(plane, q, R, L, stat, partial, st)) return rc;
    return covar_stat_means(partial, L, d_mean, st);
}

extern "C" int sq_covariation_wstat_scan(const uint8_t *d_rows, int32_t R, int32_t L, const double *d_weights, int32_t statistic,
                                         int32_t correction, int32_t minspan, double min_rows, double min_stat, void *d_scratch,
                                         size_t scratch_bytes, double *d_mean, int64_t *d_flat, int64_t *d_joint, double *d_raw, double *d_value,
                                         int64_t cap, uint64_t *d_out, void *hip_stream)
{
    if (minspan < 0 || !(min_rows >= 0.0) || std::isnan(min_stat) || cap < 0 || (cap && (!d_flat || !d_joint || !d_raw || !d_value))) {
        sq_set_error("sq_covariation_wstat_scan: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = wstat_open("sq_covariation_wstat_scan", d_rows, R, L, d_weights, statistic, correction, d_scratch, scratch_bytes, d_mean, d_out,
                            st))
        return rc;
    const uint32_t *q = (const uint32_t *)((uint64_t *)d_scratch + SqCovarWstat::q_at(R, L));
    const unsigned blocks = (unsigned)std::min<int64_t>(SqCovar::tile_count(SqCovarStat::tiles(L)), SQ_COVSTAT_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_wstat_scan_kernel, dim3(blocks), dim3(256), sq_covar_wstat_lds(SQ_COVWSTAT_LDS_SCAN).total, st,
                       (const uint64_t *)d_scratch, q, R, L, statistic, correction, minspan, min_rows, min_stat, (const double *)d_mean,
                       (long long *)d_flat, (long long *)d_joint, d_raw, d_value, (long long)cap, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_covar_wstat_scan_kernel");
}

extern "C" int sq_covariation_wstat_pairs(const uint8_t *d_rows, int32_t R, int32_t L, const double *d_weights, int32_t statistic,
                                          int32_t correction, const int32_t *d_pairs, int64_t P, void *d_scratch, size_t scratch_bytes,
                                          double *d_mean, int64_t *d_joint, double *d_raw, double *d_value, uint64_t *d_out, void *hip_stream)
{
    if (P < 0 || (P && (!d_pairs || !d_joint || !d_raw || !d_value))) {
        sq_set_error("sq_covariation_wstat_pairs: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = wstat_open("sq_covariation_wstat_pairs", d_rows, R, L, d_weights, statistic, correction, d_scratch, scratch_bytes, d_mean,
                            d_out, st))
        return rc;
    if (!P) return 0;
    const uint32_t *q = (const uint32_t *)((uint64_t *)d_scratch + SqCovarWstat::q_at(R, L));
    const unsigned blocks = (unsigned)std::min<int64_t>((P + 255) / 256, SQ_COVSTAT_MAX_BLOCKS);
    hipLaunchKernelGGL(sq_covar_wstat_pairs_kernel, dim3(blocks), dim3(256), sq_covar_wstat_lds(SQ_COVWSTAT_LDS_PAIRS).total, st,
                       (const uint64_t *)d_scratch, q, R, L, statistic, correction, (const double *)d_mean, d_pairs, (long long)P,
                       (long long *)d_joint, d_raw, d_value, (unsigned long long *)d_out);
    return sq_check(hipGetLastError(), "sq_covar_wstat_pairs_kernel");
}
