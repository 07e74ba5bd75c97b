// The shuffled-column null of the weighted covariation statistics (CovariationStatisticsSignificance(weights=); definitions:
// sq_covar_wstat_null.h), on the planes that sq_covar_null_planes_kernel (sq_covar_null_dev.hip) forms for a batch of samples
// and the weights quantised once -- row r of every sample keeps q[r]:
//   sq_covar_wstat_quantise_kernel   (sq_covar_wstat_dev.hip) q of the weights; status 3 on a bad weight
//   sq_covar_wstat_sums_kernel and the two reductions of sq_covar_stat_dev.hip   per sample, on its planes: its column means,
//                                    with the bits sq_covariation_wstat_scan gives them
//   sq_covar_wstat_null_scan_kernel  pass 2 per sample of the batch; a cell leaves no record: its C is binned against the
//                                    observed values and folded into the sample's maximum
//   sq_covar_wstat_null_pairs_kernel one lane per (observed pair, sample): does the same cell reach the observed value?
//   sq_covar_stat_null_max_kernel    (sq_covar_stat_dev.hip) the samples' maxima from integer keys to doubles
//
// Integer atomics only, no float atomics, no record, no L x L matrix: two calls give the same bits, whatever the batch.  All
// buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_covar_wstat_null.h"
#include "sq_covar_wstat_dev.h"
#include "sq_covar_planes.h"
#include <cmath>

namespace {

constexpr int T = SQ_COVSTAT_TILE, PASSES = 4, NB = SQ_COVWSTATNULL_LDS_BINS;
static_assert(NB >= 2 && NB % 4 == 0, "the thresholds end on 16 bytes");

}  // namespace

// The all-pairs scan of the batch's samples: blockIdx.y is the sample, blockIdx.x walks the tiles as sq_covar_wstat_scan_kernel
// does (the same four passes, one cell per thread, tile_bins() for its 16 counters).  A cell in scope gets S = raw_w() and C =
// corrected() with the means of its own sample (mean + sample * (L + 1); not read with corr == SQ_COVSTAT_NONE); C goes into
// bin() of the observed values and, as its integer key, into the thread's running maximum.  The bin is added as
// sq_covar_stat_null_scan_kernel adds it: bin 0 in a register, a wave whose other cells share one bin adds once, the lowest
// SQ_COVWSTATNULL_LDS_BINS thresholds and bins in LDS (a search starts with every lane at the same threshold, a broadcast), the
// others in global memory.  A block adds its counters to hist and its maximum to null_max[sample] once, when it has walked its
// tiles: integer atomics only, a few per block.
extern "C" __global__ __launch_bounds__(256) void sq_covar_wstat_null_scan_kernel(const uint64_t *plane, const uint32_t *q, int32_t R,
                                                                                 int32_t L, int32_t stat, int32_t corr, int32_t minspan,
                                                                                 const double *mean, const double *thresholds, long long U,
                                                                                 unsigned long long *hist, unsigned long long *null_max)
{
    const SqCovarWstatLds lds = sq_covar_wstat_lds(SQ_COVWSTAT_LDS_NULL);
    WstatPlanesLds &s_pl = *reinterpret_cast<WstatPlanesLds *>(s_dyn + lds.planes);
    uint32_t *s_q = reinterpret_cast<uint32_t *>(s_dyn + lds.q);
    int64_t *bins = reinterpret_cast<int64_t *>(s_dyn + lds.bins) + threadIdx.x;
    double *s_T = reinterpret_cast<double *>(s_dyn + lds.thresholds);
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_dyn + lds.hist);
    unsigned long long &s_max = *reinterpret_cast<unsigned long long *>(s_dyn + lds.top);
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
            const int vl = pass * (T / PASSES) + (tid >> 5);
            int64_t Q[16];
            tile_bins(plane, q, W, Lpad, v0, w0, s_pl, s_q, vl, bins, Q);
            const int64_t v = v0 + vl, w = w0 + wl;
            const bool live = SqCovar::in_scope(v, w, L, minspan);
            int64_t b = 0;
            if (live) {
                const double S = SqCovarWstat::raw_w(stat, Q);
                const double C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mean[v], mean[w], mean_all) : S;
                const unsigned long long key = SqCovarStatNull::key(C);
                most = key > most ? key : most;
                if (U && C >= t0) b = SqCovarStatNull::bin_by(thr, U, C);
                below += b == 0;
            }
            const bool rest = live && b > 0;
            const unsigned long long m = __ballot(rest);
            if (m) {                                                 // (wave-uniform)
                const int first = __ffsll((unsigned long long)m) - 1;
                const int64_t b_first = __shfl((long long)b, first);
                if (__ballot(rest && b == b_first) == m) {
                    if (lane == first) add(b_first, (uint32_t)__popcll(m));
                } else if (rest)
                    add(b, 1u);
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
// sq_covar_wstat_pairs_kernel forms it (cell_bins() through the thread's bins in LDS), and one more for own_ge[pair] when it
// reaches the observed value.  A pair that is not v < w inside the L columns counts nothing and leaves status 2 (a status 3 of
// the weights stays).
extern "C" __global__ __launch_bounds__(256) void sq_covar_wstat_null_pairs_kernel(const uint64_t *plane, const uint32_t *q, int32_t R,
                                                                                  int32_t L, int32_t stat, int32_t corr, const double *mean,
                                                                                  const int32_t *pairs, const double *value, long long P,
                                                                                  int32_t samples, int32_t *own_ge, unsigned long long *out)
{
    const SqCovarWstatLds lds = sq_covar_wstat_lds(SQ_COVWSTAT_LDS_PAIRS);
    int64_t *bins = reinterpret_cast<int64_t *>(s_dyn + lds.bins) + threadIdx.x;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L), per = SqCovar::plane_words(R, L);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < P * samples; k += (int64_t)gridDim.x * 256) {
        const int64_t at = k % P, sample = k / P;
        const int32_t v = pairs[2 * at], w = pairs[2 * at + 1];
        if (!SqCovar::valid_pair(v, w, L)) {
            atomicMax(&out[1], 2ull);
            continue;
        }
        int64_t Q[16];
        cell_bins(plane + sample * per, q, W, Lpad, v, w, bins, Q);
        const double S = SqCovarWstat::raw_w(stat, Q);
        const double *mine = mean + sample * ((int64_t)L + 1);       // (not read without a correction)
        const double C = corr != SQ_COVSTAT_NONE ? SqCovarStat::corrected(corr, S, mine[v], mine[w], mine[L]) : S;
        if (C >= value[at]) atomicAdd(&own_ge[at], 1);
    }
}

extern "C" size_t sq_covariation_wstat_null_scratch(int32_t R, int32_t L, int32_t batch)
{
    return R < 1 || L < 1 || batch < 1 ? 0 : (size_t)SqCovarWstatNull::scratch(R, L, batch).words * 8;
}

extern "C" int sq_covariation_wstat_null(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction, int32_t minspan,
                                         const int32_t *d_pairs, const double *d_value, int64_t P, const double *d_thresholds, int64_t U,
                                         int32_t K, uint64_t seed, int32_t batch, void *d_scratch, size_t scratch_bytes, int64_t *d_hist,
                                         int32_t *d_own_ge, double *d_null_max, uint64_t *d_out, void *hip_stream, const double *d_weights)
{
    const std::string who("sq_covariation_wstat_null");
    if (K < 1 || minspan < 0 || P < 0 || U < 0 || !d_hist || !d_null_max || !d_out || (P && (!d_pairs || !d_value || !d_own_ge)) ||
        (U && !d_thresholds) || statistic < 0 || statistic >= SQ_COVSTAT_STATS || correction < 0 || correction >= SQ_COVSTAT_CORRECTIONS ||
        !d_rows || !d_weights || !d_scratch || R < 1 || L < 1 || batch < 1 || batch > 65535) {
        sq_set_error(who + ": bad argument");
        return -1;
    }
    static_assert(SQ_COVNULL_MAX_ROWS <= SQ_COVWSTAT_MAX_ROWS, "the shuffle's cap is the one that binds");
    if (R > SQ_COVNULL_MAX_ROWS) {
        sq_set_error(who + ": more than " + std::to_string(SQ_COVNULL_MAX_ROWS) + " rows (SQ_COVNULL_MAX_ROWS: a column's sort keys lie in LDS)");
        return -1;
    }
    if (L > SQ_COVNULL_MAX_COLS || (int64_t)batch * SqCovar::lpad(L) > 0x7fffffffll) {
        sq_set_error(who + ": more than 2^21 columns, or more than 2^31 columns in a batch of samples");
        return -1;
    }
    if (scratch_bytes < sq_covariation_wstat_null_scratch(R, L, batch)) {
        sq_set_error(who + ": scratch too small");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const SqCovarWstatNullScratch at = SqCovarWstatNull::scratch(R, L, batch);
    const int64_t per_plane = SqCovar::plane_words(R, L), per_partial = SqCovarStat::partial_words(L), per_mean = (int64_t)L + 1;
    uint64_t *d_plane = (uint64_t *)d_scratch + at.planes;
    double *d_partial = (double *)d_scratch + at.partial, *d_mean = (double *)d_scratch + at.mean;
    uint8_t *d_cls = (uint8_t *)((uint64_t *)d_scratch + at.cls);
    uint32_t *d_q = (uint32_t *)((uint64_t *)d_scratch + at.q);
    unsigned long long *d_key = (unsigned long long *)d_null_max;    // (the samples' maxima as keys until the last kernel)
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    HIPCK(hipMemsetAsync(d_hist, 0, (size_t)(U + 1) * sizeof(int64_t), st));
    HIPCK(hipMemsetAsync(d_null_max, 0, (size_t)K * sizeof(double), st));
    if (P) HIPCK(hipMemsetAsync(d_own_ge, 0, (size_t)P * sizeof(int32_t), st));
    if (int rc = null_classes(d_rows, R, L, d_cls, st)) return rc;
    if (int rc = covar_wstat_quantise(d_weights, R, d_q, d_out, st)) return rc;      // (once: q is the same for every sample)
    const int64_t ntiles = SqCovar::tile_count(SqCovarStat::tiles(L));
    for (int32_t k0 = 0; k0 < K; k0 += batch) {
        const int32_t samples = std::min(batch, K - k0);
        if (int rc = null_planes(d_cls, R, L, seed, (uint64_t)k0, samples, d_plane, st)) return rc;
        // Pass 1 of every sample with the kernels and the grid of sq_covariation_wstat_scan: the means have its bits.
        for (int32_t s = 0; correction != SQ_COVSTAT_NONE && s < samples; s++) {
            double *partial = d_partial + s * per_partial;
            if (int rc = covar_wstat_sums(d_plane + s * per_plane, d_q, R, L, statistic, partial, st)) return rc;
            if (int rc = covar_stat_means(partial, L, d_mean + s * per_mean, st)) return rc;
        }
        // The scan's grid: the batch's samples times as many blocks as keep the whole grid near SQ_COVSTAT_MAX_BLOCKS; a block
        // walks the rest of its sample's tiles by grid stride.
        const unsigned per = (unsigned)std::min<int64_t>(ntiles, std::max<int64_t>(SQ_COVSTAT_MAX_BLOCKS / samples, 1));
        hipLaunchKernelGGL(sq_covar_wstat_null_scan_kernel, dim3(per, (unsigned)samples), dim3(256),
                           sq_covar_wstat_lds(SQ_COVWSTAT_LDS_NULL).total, st, (const uint64_t *)d_plane, (const uint32_t *)d_q, R, L, statistic,
                           correction, minspan, (const double *)d_mean, d_thresholds, (long long)U, (unsigned long long *)d_hist, d_key + k0);
        if (int rc = sq_check(hipGetLastError(), "sq_covar_wstat_null_scan_kernel")) return rc;
        if (!P) continue;
        const unsigned blocks = (unsigned)std::min<int64_t>((P * samples + 255) / 256, SQ_COVSTAT_MAX_BLOCKS);
        hipLaunchKernelGGL(sq_covar_wstat_null_pairs_kernel, dim3(blocks), dim3(256), sq_covar_wstat_lds(SQ_COVWSTAT_LDS_PAIRS).total, st,
                           (const uint64_t *)d_plane, (const uint32_t *)d_q, R, L, statistic, correction, (const double *)d_mean, d_pairs,
                           d_value, (long long)P, samples, d_own_ge, (unsigned long long *)d_out);
        if (int rc = sq_check(hipGetLastError(), "sq_covar_wstat_null_pairs_kernel")) return rc;
    }
    return covar_stat_null_max(d_key, K, st);
}
