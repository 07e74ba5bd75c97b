// The shuffled-column null of the covariation statistic (CovariationSignificance) on the device.  Definition: sq_covar_null.h;
// planes, counts and predicates: sq_covar.h.
//
//   sq_covar_null_classes_kernel  the class bytes of the observed rows, column after column (once per call)
//   sq_covar_null_planes_kernel   the bit planes of the shuffled alignments of a batch of samples, one block per (sample, column):
//                                 sort keys in LDS, a bitonic sort, the planes' words from wave ballots; no shuffled alignment
//                                 is ever written as bytes
//   sq_covar_null_scan_kernel     sq_covar_scan_kernel's tile loop per sample of the batch; a cell leaves no record: its cov is
//                                 binned against the observed values and folded into the sample's maximum
//   sq_covar_null_pairs_kernel    one lane per (observed pair, sample): does the same cell reach the observed cov?
//
// All buffers are the caller's device memory, everything is enqueued on the caller's stream, nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_covar_null.h"

// cls_t[c * R + r] = the class of row r at column c: 64 x 64 bytes through LDS, read along the rows and written along the
// columns, so that a block of the planes kernel reads its column as R consecutive bytes.
extern "C" __global__ __launch_bounds__(256) void sq_covar_null_classes_kernel(const uint8_t *rows, int32_t R, int32_t L, uint8_t *cls_t)
{
    __shared__ uint8_t s_cls[64][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ctiles = ((int64_t)L + 63) / 64;
    const int64_t c0 = (int64_t)(blockIdx.x % ctiles) * 64, r0 = (int64_t)(blockIdx.x / ctiles) * 64;
    for (int k = wave; k < 64; k += 4) {
        const int64_t r = r0 + k, c = c0 + lane;
        s_cls[k][lane] = (uint8_t)(r < R && c < L ? SqCovar::cls(rows[r * L + c]) : SQ_COV_OTHER);
    }
    __syncthreads();
    for (int k = wave; k < 64; k += 4) {
        const int64_t c = c0 + k, r = r0 + lane;
        if (c < L && r < R) cls_t[c * R + r] = s_cls[lane][k];
    }
}

// Block b: column b % Lpad of sample k0 + b / Lpad of the batch, whose planes start at plane + (b / Lpad) * plane_words.  The
// padded(R) keys and the R class bytes of the column lie in dynamic LDS.  After the sort lane = row of the shuffled column:
// wave w takes the words w, w + 4, ..., and a plane's word is the wave's ballot of "my row has the plane's class" (rows >= R
// count as "other", which has no plane).  A column L .. Lpad - 1 is written as zeros.  Every trip count is block-uniform.
extern "C" __global__ __launch_bounds__(256) void sq_covar_null_planes_kernel(const uint8_t *cls_t, int32_t R, int32_t L, unsigned long long seed,
                                                                             unsigned long long k0, uint64_t *plane)
{
    extern __shared__ uint64_t s_key[];
    const uint32_t n = SqCovarNull::padded(R), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint8_t *s_cls = (uint8_t *)(s_key + n);
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t c = blockIdx.x % Lpad, s = blockIdx.x / Lpad;
    uint64_t *out = plane + s * SqCovar::plane_words(R, L);
    if (c >= L) {
        for (int64_t i = tid; i < SQ_COV_PLANES * W; i += 256) out[SqCovar::at((int)(i / W), i % W, c, W, Lpad)] = 0ull;
        return;
    }
    for (uint32_t r = tid; r < n; r += 256) {
        const bool real = r < (uint32_t)R;
        s_key[r] = real ? SqCovarNull::sortkey(seed, k0 + (uint64_t)s, (uint64_t)c, r, (uint64_t)R, (uint64_t)L) : SqCovarNull::sentinel();
        if (real) s_cls[r] = cls_t[c * R + r];
    }
    __syncthreads();
    for (uint32_t k = 2; k <= n; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t t = tid; t < n / 2; t += 256) SqCovarNull::bitonic_pair(s_key, t, k, j);
            __syncthreads();
        }
    for (int64_t wd = wave; wd < W; wd += 4) {
        const int64_t row = wd * 64 + lane;                          // (the first R keys are the real ones: their rows are < R)
        const int mine = row < R ? s_cls[SqCovarNull::source_row(s_key[row])] : SQ_COV_OTHER;
        for (int p = 0; p < SQ_COV_PLANES; p++) {
            const unsigned long long m = __ballot(mine == p);
            if ((int)lane == p) out[SqCovar::at(p, wd, c, W, Lpad)] = m;
        }
    }
}

// The all-pairs scan of the batch's samples: blockIdx.y is the sample, blockIdx.x walks the tiles as sq_covar_scan_kernel does
// (same thread-to-cell map, same LDS chunks).  What differs is the end of a tile.  An in-scope cell's cov goes into bin() of the
// observed values and into the thread's running maximum.  Nearly every null cell lies below the smallest observed value:
// bin 0 is counted in a register.  The other bins of a wave's 64 cells go to the block's LDS counters (the lowest
// SQ_COVNULL_LDS_BINS bins, whose thresholds are in LDS too, 4 bytes each: cov < R^2 <= 2^24 here, so a larger threshold is
// kept as 2^32 - 1) -- as one add when they are one bin, else lane by lane -- and beyond those bins to global memory.  A
// block adds its counters to hist and its maximum to null_max[sample] once, when it has walked its tiles: integer atomics
// only, a few per block.
extern "C" __global__ __launch_bounds__(256) void sq_covar_null_scan_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t minspan,
                                                                           const long long *T, long long U, unsigned long long *hist,
                                                                           unsigned long long *null_max)
{
    constexpr int TL = SQ_COV_TILE, CH = SQ_COV_WORD_CHUNK, NB = SQ_COVNULL_LDS_BINS;
    static_assert(TL == 32, "four cells per thread of a 256-thread block");
    __shared__ uint64_t s_v[SQ_COV_PLANES][CH][TL], s_w[SQ_COV_PLANES][CH][TL];
    __shared__ uint32_t s_T[NB], s_hist[NB];
    __shared__ unsigned long long s_max;
    const int tid = threadIdx.x, lane = tid & 63, wl = tid & 31, vl = (tid >> 5) * 4;
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
    const int64_t nT = ((int64_t)L + TL - 1) / TL, ntiles = SqCovar::tile_count(nT);
    const int lds_bins = (int)(U + 1 < NB ? U + 1 : NB), lds_thr = (int)(U < NB ? U : NB);
    plane += (int64_t)blockIdx.y * SqCovar::plane_words(R, L);
    for (int i = tid; i < NB; i += 256) {
        s_hist[i] = 0u;
        if (i < lds_thr) s_T[i] = (uint32_t)(T[i] < 0xFFFFFFFFll ? T[i] : 0xFFFFFFFFll);
    }
    if (!tid) s_max = 0ull;
    __syncthreads();
    auto thr = [&](int64_t i) -> int64_t { return i < NB ? (int64_t)s_T[i] : (int64_t)T[i]; };
    auto add = [&](int64_t b, uint32_t many) {
        if (b < NB) atomicAdd(&s_hist[b], many);
        else atomicAdd(&hist[b], (unsigned long long)many);
    };
    const int64_t t0 = U ? thr(0) : 0;
    uint32_t below = 0;                                              // this thread's cells of bin 0
    int64_t most = 0;
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ti, tj;
        SqCovar::tile_of(k, nT, ti, tj);
        const int64_t v0 = (int64_t)ti * TL, w0 = (int64_t)tj * TL;  // (v0 + 31, w0 + 31 < Lpad: a multiple of 64 >= L)
        int32_t cnt[4][7] = {};
        for (int64_t wb = 0; wb < W; wb += CH) {
            __syncthreads();                                         // (the last chunk has been read)
            for (int i = tid; i < SQ_COV_PLANES * CH * TL; i += 256) {
                const int p = i / (CH * TL), wd = i / TL % CH, col = i % TL;
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
            const bool live = SqCovar::in_scope(v0 + vl + c, w0 + wl, L, minspan);
            int64_t b = 0;
            if (live) {
                const int64_t cov = SqCovar::finish(cnt[c]);
                most = cov > most ? cov : most;
                if (U && cov >= t0) b = SqCovarNull::bin_by(thr, U, cov);
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
    atomicMax(&s_max, (unsigned long long)most);
    __syncthreads();
    for (int i = tid; i < lds_bins; i += 256)
        if (s_hist[i]) atomicAdd(&hist[i], (unsigned long long)s_hist[i]);
    if (!tid && s_max) atomicMax(&null_max[blockIdx.y], s_max);
}

// One lane per (pair, sample of the batch), the pair running fastest: cov of the sample's planes at the pair, formed as
// sq_covar_pairs_kernel forms it, and one more for own_ge[pair] when it reaches the observed value.  A pair that is not
// v < w inside the L columns counts nothing and leaves status 2.
extern "C" __global__ __launch_bounds__(256) void sq_covar_null_pairs_kernel(const uint64_t *plane, int32_t R, int32_t L, const int32_t *pairs,
                                                                            const long long *cov, long long P, int32_t samples,
                                                                            int32_t *own_ge, unsigned long long *out)
{
    const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L), per = SqCovar::plane_words(R, L);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < P * samples; k += (int64_t)gridDim.x * 256) {
        const int64_t at = k % P;
        const uint64_t *mine = plane + (k / P) * per;
        const int32_t v = pairs[2 * at], w = pairs[2 * at + 1];
        if (!SqCovar::valid_pair(v, w, L)) {
            out[1] = 2ull;
            continue;
        }
        int32_t cnt[7] = {};
        for (int64_t wd = 0; wd < W; wd++) {
            uint64_t a[SQ_COV_PLANES], b[SQ_COV_PLANES];
            for (int p = 0; p < SQ_COV_PLANES; p++) {
                a[p] = mine[SqCovar::at(p, wd, v, W, Lpad)];
                b[p] = mine[SqCovar::at(p, wd, w, W, Lpad)];
            }
            SqCovar::accumulate(a, b, cnt);
        }
        if (SqCovar::finish(cnt) >= cov[at]) atomicAdd(&own_ge[at], 1);
    }
}

// d_scratch: the planes of `batch` samples, then the class bytes (R * L, rounded up to 8)
static size_t null_class_bytes(int32_t R, int32_t L) { return ((size_t)R * (size_t)L + 7) & ~(size_t)7; }

extern "C" size_t sq_covariation_null_scratch(int32_t R, int32_t L, int32_t batch)
{
    if (R < 1 || L < 1 || batch < 1) return 0;
    return (size_t)batch * (size_t)SqCovar::plane_words(R, L) * sizeof(uint64_t) + null_class_bytes(R, L);
}

// The checks both entries share.
static int null_check(const char *who, const void *d_rows, int32_t R, int32_t L, int32_t batch, const void *d_scratch, size_t scratch_bytes)
{
    const std::string name(who);
    if (!d_rows || !d_scratch || R < 1 || L < 1 || batch < 1 || batch > 65535) {
        sq_set_error(name + ": bad argument");
        return -1;
    }
    if (R > SQ_COVNULL_MAX_ROWS) {
        sq_set_error(name + ": more than " + std::to_string(SQ_COVNULL_MAX_ROWS) + " rows (SQ_COVNULL_MAX_ROWS: a column's sort keys lie in LDS)");
        return -1;
    }
    if (L > SQ_COVNULL_MAX_COLS || (int64_t)batch * SqCovar::lpad(L) > 0x7fffffffll) {
        sq_set_error(name + ": more than 2^21 columns, or more than 2^31 columns in a batch of samples");
        return -1;
    }
    if (scratch_bytes < sq_covariation_null_scratch(R, L, batch)) {
        sq_set_error(name + ": scratch too small");
        return -1;
    }
    return 0;
}

// (sq_internal.h declares null_classes and null_planes: sq_covar_stat_dev.hip shuffles with them too)
int null_classes(const uint8_t *d_rows, int32_t R, int32_t L, uint8_t *d_cls, hipStream_t st)
{
    const int64_t blocks = (((int64_t)L + 63) / 64) * (((int64_t)R + 63) / 64);      // (<= 2^15 * 2^6)
    hipLaunchKernelGGL(sq_covar_null_classes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_rows, R, L, d_cls);
    return sq_check(hipGetLastError(), "sq_covar_null_classes_kernel");
}

int null_planes(const uint8_t *d_cls, int32_t R, int32_t L, uint64_t seed, uint64_t k0, int32_t samples, uint64_t *d_plane, hipStream_t st)
{
    const size_t lds = (size_t)SqCovarNull::padded(R) * sizeof(uint64_t) + (((size_t)R + 7) & ~(size_t)7);
    hipLaunchKernelGGL(sq_covar_null_planes_kernel, dim3((unsigned)(samples * SqCovar::lpad(L))), dim3(256), lds, st, d_cls, R, L,
                       (unsigned long long)seed, (unsigned long long)k0, d_plane);
    return sq_check(hipGetLastError(), "sq_covar_null_planes_kernel");
}

extern "C" int sq_covariation_null_planes(const uint8_t *d_rows, int32_t R, int32_t L, int64_t k, int32_t count, uint64_t seed,
                                          void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    if (int rc = null_check("sq_covariation_null_planes", d_rows, R, L, count, d_scratch, scratch_bytes)) return rc;
    if (k < 0) {
        sq_set_error("sq_covariation_null_planes: bad argument");
        return -1;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    uint64_t *d_plane = (uint64_t *)d_scratch;
    uint8_t *d_cls = (uint8_t *)(d_plane + (int64_t)count * SqCovar::plane_words(R, L));
    if (int rc = null_classes(d_rows, R, L, d_cls, st)) return rc;
    return null_planes(d_cls, R, L, seed, (uint64_t)k, count, d_plane, st);
}

extern "C" int sq_covariation_null(const uint8_t *d_rows, int32_t R, int32_t L, int32_t minspan, const int32_t *d_pairs, const int64_t *d_cov,
                                   int64_t P, const int64_t *d_thresholds, int64_t U, int32_t K, uint64_t seed, int32_t batch, void *d_scratch,
                                   size_t scratch_bytes, int64_t *d_hist, int32_t *d_own_ge, int64_t *d_null_max, uint64_t *d_out,
                                   void *hip_stream)
{
    if (K < 1 || minspan < 0 || P < 0 || U < 0 || !d_hist || !d_null_max || !d_out || (P && (!d_pairs || !d_cov || !d_own_ge)) ||
        (U && !d_thresholds)) {
        sq_set_error("sq_covariation_null: bad argument");
        return -1;
    }
    if (int rc = null_check("sq_covariation_null", d_rows, R, L, batch, d_scratch, scratch_bytes)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    uint64_t *d_plane = (uint64_t *)d_scratch;
    uint8_t *d_cls = (uint8_t *)(d_plane + (int64_t)batch * SqCovar::plane_words(R, L));
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    HIPCK(hipMemsetAsync(d_hist, 0, (size_t)(U + 1) * sizeof(int64_t), st));
    HIPCK(hipMemsetAsync(d_null_max, 0, (size_t)K * sizeof(int64_t), st));
    if (P) HIPCK(hipMemsetAsync(d_own_ge, 0, (size_t)P * sizeof(int32_t), st));
    if (int rc = null_classes(d_rows, R, L, d_cls, st)) return rc;
    // The scan's grid: the batch's samples times as many blocks as keep the whole grid near SQ_COV_MAX_BLOCKS (sq_covar_dev.hip
    // says why that many); a block walks the rest of its sample's tiles by grid stride.
    const int64_t nT = ((int64_t)L + SQ_COV_TILE - 1) / SQ_COV_TILE, ntiles = SqCovar::tile_count(nT);
    for (int32_t k0 = 0; k0 < K; k0 += batch) {
        const int32_t samples = std::min(batch, K - k0);
        if (int rc = null_planes(d_cls, R, L, seed, (uint64_t)k0, samples, d_plane, st)) return rc;
        const unsigned per = (unsigned)std::min<int64_t>(ntiles, std::max<int64_t>(SQ_COV_MAX_BLOCKS / samples, 1));
        hipLaunchKernelGGL(sq_covar_null_scan_kernel, dim3(per, (unsigned)samples), dim3(256), 0, st, (const uint64_t *)d_plane, R, L, minspan,
                           (const long long *)d_thresholds, (long long)U, (unsigned long long *)d_hist, (unsigned long long *)d_null_max + k0);
        if (int rc = sq_check(hipGetLastError(), "sq_covar_null_scan_kernel")) return rc;
        if (!P) continue;
        const unsigned blocks = (unsigned)std::min<int64_t>((P * samples + 255) / 256, SQ_COV_MAX_BLOCKS);
        hipLaunchKernelGGL(sq_covar_null_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)d_plane, R, L, d_pairs,
                           (const long long *)d_cov, (long long)P, samples, d_own_ge, (unsigned long long *)d_out);
        if (int rc = sq_check(hipGetLastError(), "sq_covar_null_pairs_kernel")) return rc;
    }
    return 0;
}
