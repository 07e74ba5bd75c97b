// The shuffled-column null of the covariation statistics (sq_covariation_stat_null, CovariationStatisticsSignificance): is
// the MI, G-test or chi-square value of a pair of columns remarkable?  The shuffle is that of sq_covar_null.h: sample k of K
// permutes the rows of every column on its own by the sort keys of (seed, k, column, row).  The statistic is that of
// sq_covar_stat.h: a null cell's value is C = corrected(raw(the cell's joint table)) with the column means of that shuffled
// sample over every pair of its distinct columns -- what sq_covariation_stat_scan returns for the shuffled alignment, bit for
// bit (the same counters, the same functions, the same order of every sum).
//
// Statistics.  For the observed values value[p] with sorted distinct values T[0..U-1] (IEEE order: -0.0 and 0.0 are one
// value, no NaN -- corrected() returns S when mean_all == 0), a null cell falls into bin() = the number of T <= its C, 0..U;
// the pooled count null_ge[p] is the sum of the bins from 1 + (index of value[p] in T) on.  own_ge[p] counts the samples in
// which the same cell has C >= value[p].  null_max[k] is the largest C of sample k's in-scope cells, -infinity without one: it
// is folded as the integer key() of the double, which has the doubles' order, so that an integer atomic maximum finds it
// (no float atomics: two calls give the same bits); key 0 is below every number's key and stands for "no cell".
//
// This header compiles for the device and for the host (tests/native/covar_stat_null_host.cpp runs it as one thread).
#pragma once
#include <string.h>
#include "sq_covar_null.h"
#include "sq_covar_stat.h"

// The scan keeps the lowest SQ_COVSTATNULL_LDS_BINS thresholds (8 bytes each) and bins (4 bytes each: a block counts fewer than
// 2^32 cells for L <= SQ_COVNULL_MAX_COLS columns) of a block in LDS: 24 KB beside the 8 KB of staged planes, so that LDS admits
// as many blocks per CU as the registers do (sq_covar_stat_dev.hip has the figures).  Thresholds and bins beyond them are
// global memory.
#define SQ_COVSTATNULL_LDS_BINS 2048

struct SqCovarStatNull {
    SQ_COV_HD static uint64_t bits(double x)
    {
        uint64_t u;
        memcpy(&u, &x, sizeof u);
        return u;
    }
    // An unsigned key with the order of the doubles: negative numbers have all bits flipped, the others the sign bit set.
    // -inf < .. < -0.0 < +0.0 < .. < +inf; every key of a number (NaN aside) is above 0.
    SQ_COV_HD static uint64_t key(double x)
    {
        const uint64_t u = bits(x);
        return (u >> 63) ? ~u : u | 0x8000000000000000ull;
    }
    // the double of a key; key 0 ("no cell") gives -infinity
    SQ_COV_HD static double unkey(uint64_t k)
    {
        const uint64_t u = k == 0 ? 0xFFF0000000000000ull : (k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k;
        double x;
        memcpy(&x, &u, sizeof x);
        return x;
    }

    // The number of thresholds <= C among thr(0) < thr(1) < .. < thr(U - 1), compared as doubles: a binary search.
    template <class F> SQ_COV_HD static int64_t bin_by(F thr, int64_t U, double C)
    {
        int64_t lo = 0, hi = U;                                      // (thr(i) <= C for i < lo, thr(i) > C for i >= hi)
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (thr(mid) <= C) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
    SQ_COV_HD static int64_t bin(const double *T, int64_t U, double C)
    {
        return bin_by([T](int64_t i) { return T[i]; }, U, C);
    }

    // ---- the scratch of sq_covariation_stat_null: the planes of `batch` samples, then per sample the partial column sums of
    // pass 1, then per sample L + 1 means, then the class bytes of the rows (R * L, rounded up to 8)
    SQ_COV_HD static int64_t sample_words(int32_t R, int32_t L) { return SqCovarStat::scratch_words(R, L) + (int64_t)L + 1; }
    SQ_COV_HD static int64_t class_words(int32_t R, int32_t L) { return ((int64_t)R * L + 7) / 8; }
    SQ_COV_HD static int64_t scratch_words(int32_t R, int32_t L, int32_t batch) { return batch * sample_words(R, L) + class_words(R, L); }
};
