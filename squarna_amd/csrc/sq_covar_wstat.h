// Covariation statistics of two alignment columns with a weight per row (sq_covariation_wstat_scan / sq_covariation_wstat_pairs,
// CovariationStatistics(weights=)): the statistics of sq_covar_stat.h on a joint table whose cells are sums of row weights
// instead of row counts.
//
// Fixed-point weights.  A weight w[r] is a finite double, 0 <= w <= SQ_COVWSTAT_MAX_WEIGHT = 2048.  It is quantised once,
// q[r] = rint(w[r] * 2^20) (quantise(): the product is exact in fp64, the rounding ties-to-even), q <= 2^31 fits a uint32, and
// everything after is integer: the sums are exact, free of the order of the rows and the same in two calls.  A row of weight
// 0 takes part in nothing.  R <= SQ_COVWSTAT_MAX_ROWS = 2^22: every counter, margin and total is an int64 <= 2^53 and
// converts to a double exactly.
//
// Joint table.  Q[a * 4 + b], a and b in A C G U, = the sum of q[r] over the rows with residue a at v and residue b at w (the
// classes and planes of sq_covar.h; a row with a gap or "other" at either column adds nothing).  accumulate() is the one place
// a word of 64 rows is added: from the planes lo = C | U, hi = G | U (the two bits of the class) and valid = A | C | G | U of
// both columns, and per row the 4-bit cell index hi_v lo_v hi_w lo_w and q[r] under valid_v & valid_w.  The public joint table
// is Q / 2^20 as a double, which is exact.
//
// Raw statistic (raw_w()).  x = (double)Q / 2^20 for the 16 cells, the margins and N, the margins and N summed as int64
// first; then the formulas and the term order of SqCovarStat::raw() in doubles: log(the quotient (x_k * X_N) / (x_a * x_b)), and
// e = (x_a * x_b) / X_N for chi; FP contraction off, as there; 0 when N is 0.  When every weight is an integer and N * N < 2^53
// (n * N and na * nb are then exact doubles) this gives the bits of raw() on the integer counts: every x is the count, the
// products are the products raw() forms as int64 and converts, and each operation after that is the same one.
//
// The quotient under the logarithm (ratio()).  raw() divides two exact integers: its quotient is rounded once.  Two rounded
// products in front of the division would put the quotient off by up to two ulp, and where it is near 1 -- a row of weight 2048
// among rows of weight 2^-20 makes such tables -- its logarithm is small and takes that error whole: the terms of MI and the
// G-test cancel to second order there, and S would be off by 10^-12 of itself.  So the two products are kept exact as a double
// and its fma residual each (the 2^20 cancel: the quotient is Q_k Q_N / (Q_a Q_b)), and the quotient of the leading parts is
// corrected once by the division's own residual: rounded once, for all but quotients within 2^-100 of a tie.  Where both
// products are exact doubles no correction is made: the quotient is raw()'s, bit for bit.
//
// Thresholds, means, correction.  A cell emits when X_N >= min_rows and C >= min_stat, both compared as doubles (emits_w()).
// The column means, mean_all, SqCovarStat::corrected(), SqCovar::in_scope(), the tile walk and the order of every float sum
// are those of sq_covar_stat.h / sq_covar_stat_dev.hip.
//
// LDS.  sq_covar_wstat_lds() places the regions of a block of each of the three kernels, and of the scan kernel of the
// weighted null (sq_covar_wstat_null_dev.hip); the launch site takes `total` from it and the kernel carves with it (as
// sq_launch_lds.h does for the launched kernels).  Every offset is a multiple of 16 and the total stays below 64 KB: no limit
// is raised.  tests/native/covar_wstat_host.cpp checks the layout and runs the header as one thread
// (tests/native/covar_wstat_null_host.cpp: the null's kind).
#pragma once
#include <stddef.h>
#include "sq_covar_stat.h"

#define SQ_COVWSTAT_ONE (1 << 20)
#define SQ_COVWSTAT_MAX_WEIGHT 2048.0
#define SQ_COVWSTAT_MAX_ROWS (1 << 22)
// the records of the scan's emission stage (SQ_EMIT_STAGE) and the bytes of its bookkeeping (SqEmitStage); sq_covar_wstat_dev.hip
// asserts both against sq_emit.h, which is HIP and not included here
#define SQ_COVWSTAT_STAGE 1024
#define SQ_COVWSTAT_EMIT_BYTES 16

// The thresholds (8 bytes each) and bins (4 bytes each) that the scan of the weighted null (sq_covar_wstat_null.h) keeps in LDS
// beside the planes, q and the 32 KB of counters; thresholds and bins beyond them are global memory.  The 2048 of the
// unweighted null (24 KB) would not fit below 64 KB here.  Measured on an MI355X (512 x 5,000, 100 samples, 433 thresholds, the
// entry alone): 512, 768 and 896 bins 546 - 547 ms, 1024 and 1536 bins 568 - 569 ms.  With 896 a block has 52,752 bytes and a CU
// of 160 KB holds three, the blocks the kernel's 132 registers admit; with 1024 (54,288 bytes, three of which are still below
// 160 KB) the time is that of 1536, where two fit: presumably the LDS is handed out in units that keep the third block out
// (supposed from these times, not read anywhere).  So 896, the most that was as fast as fewer.  (A build may set another multiple of 4 to measure it:
// tools/covariation_wstat_null_probe.py, DESIGN.md.)
#ifndef SQ_COVWSTATNULL_LDS_BINS
#define SQ_COVWSTATNULL_LDS_BINS 896
#endif

enum { SQ_COVWSTAT_LDS_SUMS = 0, SQ_COVWSTAT_LDS_SCAN = 1, SQ_COVWSTAT_LDS_PAIRS = 2, SQ_COVWSTAT_LDS_NULL = 3 };

// The LDS of a 256-thread block, in bytes from the start of its dynamic region.  planes: uint64 [2][4][WORD_CHUNK][TILE], the
// planes A C G U of the tile's two column ranges; q: uint32 [64 * WORD_CHUNK], the weights of the chunk's rows; bins: int64
// [16][256], bins[k][tid] = cell k of the table of the thread's cell (a wave's lanes hit consecutive addresses and a bin has
// one writer).  Pass 1 then has S: double [TILE][TILE + 1] and row, col: double [TILE]; pass 2 the stage's flat: int64
// [STAGE], raw: double [STAGE] and em (SqEmitStage).  The pairs kernel has the bins alone.  The null's scan has, after the
// bins, thresholds: double [SQ_COVWSTATNULL_LDS_BINS], hist: uint32 [SQ_COVWSTATNULL_LDS_BINS] and top: one uint64 (the
// block's largest key) in 16 bytes.  A region a kernel does not have is empty, at the offset of the one after it.
struct SqCovarWstatLds { uint32_t planes, q, bins, S, row, col, flat, raw, em, thresholds, hist, top; size_t total; };
SQ_COV_HD inline SqCovarWstatLds sq_covar_wstat_lds(int kernel)
{
    SqCovarWstatLds L;
    const bool tiles = kernel != SQ_COVWSTAT_LDS_PAIRS;
    uint32_t o = 0;
    L.planes = o; o += tiles ? 2u * 4u * SQ_COVSTAT_WORD_CHUNK * SQ_COVSTAT_TILE * 8u : 0u;
    L.q = o;      o += tiles ? 64u * SQ_COVSTAT_WORD_CHUNK * 4u : 0u;
    L.bins = o;   o += 16u * 256u * 8u;
    L.S = o;      o += kernel == SQ_COVWSTAT_LDS_SUMS ? SQ_COVSTAT_TILE * (SQ_COVSTAT_TILE + 1u) * 8u : 0u;
    L.row = o;    o += kernel == SQ_COVWSTAT_LDS_SUMS ? SQ_COVSTAT_TILE * 8u : 0u;
    L.col = o;    o += kernel == SQ_COVWSTAT_LDS_SUMS ? SQ_COVSTAT_TILE * 8u : 0u;
    L.flat = o;   o += kernel == SQ_COVWSTAT_LDS_SCAN ? SQ_COVWSTAT_STAGE * 8u : 0u;
    L.raw = o;    o += kernel == SQ_COVWSTAT_LDS_SCAN ? SQ_COVWSTAT_STAGE * 8u : 0u;
    L.em = o;     o += kernel == SQ_COVWSTAT_LDS_SCAN ? (uint32_t)SQ_COVWSTAT_EMIT_BYTES : 0u;
    L.thresholds = o; o += kernel == SQ_COVWSTAT_LDS_NULL ? SQ_COVWSTATNULL_LDS_BINS * 8u : 0u;
    L.hist = o;   o += kernel == SQ_COVWSTAT_LDS_NULL ? SQ_COVWSTATNULL_LDS_BINS * 4u : 0u;
    L.top = o;    o += kernel == SQ_COVWSTAT_LDS_NULL ? 16u : 0u;
    L.total = o;
    return L;
}

// One more for a bin.  On the device the bins lie in LDS and the add is the LDS's own (no value comes back, so the next row
// does not wait for this one); a bin has one writer either way.
#if defined(__HIP_DEVICE_COMPILE__)
#define SQ_COVWSTAT_ADD(p, x) atomicAdd((unsigned long long *)(p), (unsigned long long)(x))
#else
#define SQ_COVWSTAT_ADD(p, x) (*(p) += (int64_t)(x))
#endif

struct SqCovarWstat {
    // ---- the scratch of the two entries: the planes and the partial column sums of sq_covar_stat.h, then q[rpad(R)]
    // (rpad: R up to a chunk of 64 * SQ_COVSTAT_WORD_CHUNK rows, q zero beyond R: a block stages a whole chunk of q)
    SQ_COV_HD static int64_t rpad(int32_t R) { return ((int64_t)R + 64 * SQ_COVSTAT_WORD_CHUNK - 1) / (64 * SQ_COVSTAT_WORD_CHUNK) * (64 * SQ_COVSTAT_WORD_CHUNK); }
    SQ_COV_HD static int64_t q_at(int32_t R, int32_t L) { return SqCovarStat::scratch_words(R, L); }     // in 8-byte words
    SQ_COV_HD static int64_t scratch_words(int32_t R, int32_t L) { return q_at(R, L) + rpad(R) / 2; }

    // ---- q of a weight; false (and q = 0) when the weight is not a finite number in 0 .. SQ_COVWSTAT_MAX_WEIGHT
    SQ_COV_HD static bool quantise(double w, uint32_t &q)
    {
        const bool good = w >= 0.0 && w <= SQ_COVWSTAT_MAX_WEIGHT;  // (false for a NaN)
        q = good ? (uint32_t)rint(w * (double)SQ_COVWSTAT_ONE) : 0u;
        return good;
    }

    // ---- one 64-row word of two columns (a, b: the planes A C G U of v and of w; q: the weights of the word's 64 rows):
    // bins[k * stride] += q[r] for the rows r of cell k
    SQ_COV_HD static void accumulate(const uint64_t a[4], const uint64_t b[4], const uint32_t *q, int64_t *bins, int stride)
    {
        const uint64_t lo_v = a[SQ_COV_C] | a[SQ_COV_U], hi_v = a[SQ_COV_G] | a[SQ_COV_U];
        const uint64_t lo_w = b[SQ_COV_C] | b[SQ_COV_U], hi_w = b[SQ_COV_G] | b[SQ_COV_U];
        const uint64_t valid = (a[0] | a[1] | a[2] | a[3]) & (b[0] | b[1] | b[2] | b[3]);
        // Eight rows at a time: their weights are read first, whatever the rows hold (the reads go out together and none waits
        // behind an add), then each row adds its weight, or 0 when it does not count.
        SQ_COVSTAT_UNROLL
        for (int r0 = 0; r0 < 64; r0 += 8) {
            uint32_t x[8];
            SQ_COVSTAT_UNROLL
            for (int j = 0; j < 8; j++) x[j] = q[r0 + j];
            const uint32_t lv = (uint32_t)(lo_v >> r0), hv = (uint32_t)(hi_v >> r0), lw = (uint32_t)(lo_w >> r0);
            const uint32_t hw = (uint32_t)(hi_w >> r0), ok = (uint32_t)(valid >> r0);
            SQ_COVSTAT_UNROLL
            for (int j = 0; j < 8; j++) {
                const uint32_t k = (hv >> j & 1u) << 3 | (lv >> j & 1u) << 2 | (hw >> j & 1u) << 1 | (lw >> j & 1u);
                SQ_COVWSTAT_ADD(&bins[(int)k * stride], x[j] & (0u - (ok >> j & 1u)));
            }
        }
    }

    SQ_COV_HD static int64_t total(const int64_t Q[16])
    {
        int64_t N = 0;
        SQ_COVSTAT_UNROLL
        for (int k = 0; k < 16; k++) N += Q[k];
        return N;
    }
    // X_N, the weighted rows of a table, from total()
    SQ_COV_HD static double rows(int64_t N) { return (double)N / (double)SQ_COVWSTAT_ONE; }

    // ---- a * b / (c * d) of integers below 2^53 held as doubles, rounded once (the header's text says how nearly)
    SQ_COVSTAT_NO_CONTRACT SQ_COV_HD static double ratio(double a, double b, double c, double d)
    {
        SQ_COVSTAT_NO_CONTRACT_BODY
        const double num = a * b, num_lo = fma(a, b, -num), den = c * d, den_lo = fma(c, d, -den);
        const double q = num / den;
        if (num_lo == 0.0 && den_lo == 0.0) return q;
        const double rest = fma(-q, den, num) + (num_lo - q * den_lo);   // num + num_lo - q * (den + den_lo)
        return q + rest / den;
    }

    // ---- S of a cell's weighted counters
    SQ_COVSTAT_NO_CONTRACT SQ_COV_HD static double raw_w(int stat, const int64_t Q[16])
    {
        SQ_COVSTAT_NO_CONTRACT_BODY
        int64_t qa[4] = {0, 0, 0, 0}, qb[4] = {0, 0, 0, 0}, QN = 0;
        SQ_COVSTAT_UNROLL
        for (int k = 0; k < 16; k++) {
            qa[k >> 2] += Q[k];
            qb[k & 3] += Q[k];
            QN += Q[k];
        }
        if (QN == 0) return 0.0;
        const double one = (double)SQ_COVWSTAT_ONE, XN = (double)QN / one;
        double xa[4], xb[4];
        SQ_COVSTAT_UNROLL
        for (int k = 0; k < 4; k++) {
            xa[k] = (double)qa[k] / one;
            xb[k] = (double)qb[k] / one;
        }
        double s = 0.0;
        SQ_COVSTAT_UNROLL
        for (int k = 0; k < 16; k++) {
            const double x = (double)Q[k] / one, margins = xa[k >> 2] * xb[k & 3];
            if (stat == SQ_COVSTAT_CHI) {
                if (margins > 0.0) {
                    const double e = margins / XN, d = x - e;
                    s += d * d / e;
                }
            } else if (Q[k] > 0) {
                const double l = log(ratio((double)Q[k], (double)QN, (double)qa[k >> 2], (double)qb[k & 3]));
                s += (stat == SQ_COVSTAT_MI ? x / XN : x) * l;
            }
        }
        return stat == SQ_COVSTAT_GT ? 2.0 * s : s;
    }

    // ---- which cells the scan emits (in scope: SqCovar::in_scope)
    SQ_COV_HD static bool emits_w(double XN, double C, double min_rows, double min_stat) { return XN >= min_rows && C >= min_stat; }
};
