// The shuffled-column null of the covariation statistic (sq_covariation_null, CovariationSignificance): is the cov of a pair
// of columns remarkable?  Sample k of K permutes the rows of every column of the alignment on its own -- the columns keep
// their composition and lose their association -- and the covs of the shuffled alignment's cells are the null.  Byte classes,
// the plane layout, accumulate, finish and in_scope: sq_covar.h.  All integers: every implementation agrees bit for bit.
//
// Shuffle.  Row r of column c of sample k has the sort key
//   z = seed + 0x9E3779B97F4A7C15 * (1 + ((k * L + c) * R + r))   (mod 2^64), then the splitmix64 finaliser,
//   key = (z & ~0xFFFF) | r,
// distinct by construction for R <= 65,535 (SQ_COVNULL_KEY_ROWS); 2^64 - 1 is above every key (its low 16 bits are no row)
// and pads a column to a power of two.  Row j of the shuffled column holds the class of the row whose key is the j-th
// smallest.  Gaps and "other" bytes move like letters.
//
// Statistics.  For the observed values cov[p] with sorted distinct values T[0..U-1], a null cell falls into bin() = the
// number of T <= its cov, 0..U; the pooled count null_ge[p] is the sum of the bins from 1 + (index of cov[p] in T) on.
// own_ge[p] counts the samples in which the same cell reaches cov[p], null_max[k] is the largest null cov of sample k.
//
// This header compiles for the device and for the host (tests/native/covar_null_host.cpp runs it as one thread).
#pragma once
#include "sq_covar.h"

// The most rows the device sorts: the padded keys of a column lie in LDS, 8 bytes each (32 KB), beside its class bytes.
// The sort-key form itself holds up to SQ_COVNULL_KEY_ROWS rows.
#define SQ_COVNULL_MAX_ROWS 4096
#define SQ_COVNULL_KEY_ROWS 65535
// The scan keeps the lowest SQ_COVNULL_LDS_BINS bins and thresholds of a block in LDS (4 bytes each: a null cov is below
// R^2 <= 2^24 on the device, and a block counts fewer than 2^32 cells for L <= SQ_COVNULL_MAX_COLS columns).
#define SQ_COVNULL_LDS_BINS 4096
#define SQ_COVNULL_MAX_COLS (1 << 21)

struct SqCovarNull {
    SQ_COV_HD static uint64_t mix(uint64_t z)
    {
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
        z ^= z >> 27; z *= 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    // the sort key of row r of column c of sample k (every product mod 2^64)
    SQ_COV_HD static uint64_t sortkey(uint64_t seed, uint64_t k, uint64_t c, uint64_t r, uint64_t R, uint64_t L)
    {
        const uint64_t z = seed + 0x9E3779B97F4A7C15ull * (1ull + ((k * L + c) * R + r));
        return (mix(z) & ~0xFFFFull) | r;
    }
    SQ_COV_HD static uint64_t sentinel() { return ~0ull; }
    SQ_COV_HD static int32_t source_row(uint64_t key) { return (int32_t)(key & 0xFFFFull); }
    // the keys of a column are sorted as padded(R) of them: a power of two, at least 2
    SQ_COV_HD static uint32_t padded(int32_t R)
    {
        uint32_t n = 2;
        while (n < (uint32_t)R) n <<= 1;
        return n;
    }
    // Pair t < n / 2 of the bitonic network's stage (k, j): k = 2, 4, .. n the length of the sorted runs being formed,
    // j = k / 2, .. 1 the distance of the two keys.  All pairs of a stage are independent; the stages follow one another.
    SQ_COV_HD static void bitonic_pair(uint64_t *key, uint32_t t, uint32_t k, uint32_t j)
    {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const bool up = !(i & k);
        const uint64_t a = key[i], b = key[p];
        if ((a > b) == up) { key[i] = b; key[p] = a; }
    }
    // The whole sort as one thread: key[0 .. padded(R) - 1], the first R sorted afterwards (the host's form of the kernel's loop).
    SQ_COV_HD static void sort_keys(uint64_t *key, uint64_t seed, uint64_t k, uint64_t c, int32_t R, int32_t L)
    {
        const uint32_t n = padded(R);
        for (uint32_t r = 0; r < n; r++) key[r] = r < (uint32_t)R ? sortkey(seed, k, c, r, (uint64_t)R, (uint64_t)L) : sentinel();
        for (uint32_t kk = 2; kk <= n; kk <<= 1)
            for (uint32_t j = kk >> 1; j; j >>= 1)
                for (uint32_t t = 0; t < n / 2; t++) bitonic_pair(key, t, kk, j);
    }

    // The number of thresholds <= cov among thr(0) < thr(1) < .. < thr(U - 1): a binary search.
    template <class F> SQ_COV_HD static int64_t bin_by(F thr, int64_t U, int64_t cov)
    {
        int64_t lo = 0, hi = U;                                      // (thr(i) <= cov for i < lo, thr(i) > cov for i >= hi)
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (thr(mid) <= cov) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
    SQ_COV_HD static int64_t bin(const int64_t *T, int64_t U, int64_t cov)
    {
        return bin_by([T](int64_t i) { return T[i]; }, U, cov);
    }

    // the in-scope cells of one sample: the (v, w) with v < w < L and w - v >= minspan
    SQ_COV_HD static int64_t scope_cells(int32_t L, int32_t minspan)
    {
        const int64_t m = minspan < 1 ? 1 : minspan;
        return m >= L ? 0 : ((int64_t)L - m) * ((int64_t)L - m + 1) / 2;
    }
};
