// The shuffled-column null of the weighted covariation statistics (sq_covariation_wstat_null,
// CovariationStatisticsSignificance(weights=)): sq_covar_stat_null.h with the joint tables of sq_covar_wstat.h.
//
// The weights belong to the row slots, not to the letters.  Sample k permutes the rows of every column on its own, as
// sq_covar_null.h states it (the same function of seed, k, column and row), and row r of the shuffled alignment keeps q[r]: a
// null cell's value is the C that sq_covariation_wstat_scan returns for the shuffled rows and the same weights, bit for bit --
// raw_w() of the weighted table, the column means of that sample's own weighted S over every pair of distinct columns,
// SqCovarStat::corrected().  A row of weight 0 takes part in the shuffle (its letters move) and counts nothing.  The shuffle
// keeps each column's letter counts; it does not keep each column's weighted composition.
//
// The bins, own_ge, the key of the maximum and their meanings are those of sq_covar_stat_null.h (SqCovarStatNull::bin_by, key,
// unkey); the scan keeps SQ_COVWSTATNULL_LDS_BINS thresholds and bins in LDS (sq_covar_wstat.h: sq_covar_wstat_lds()).
//
// This header compiles for the device and for the host (tests/native/covar_wstat_null_host.cpp runs it as one thread).
#pragma once
#include "sq_covar_stat_null.h"
#include "sq_covar_wstat.h"

// Where the regions of sq_covariation_wstat_null's scratch begin, in 8-byte words: the planes of `batch` samples, then per
// sample the partial column sums of pass 1, then per sample L + 1 means, then the class bytes of the rows (R * L, rounded up to
// 8: SqCovarStatNull's layout so far), then q[rpad(R)] (uint32, zero beyond R; rpad is a multiple of 256).
struct SqCovarWstatNullScratch { int64_t planes, partial, mean, cls, q, words; };

struct SqCovarWstatNull {
    SQ_COV_HD static SqCovarWstatNullScratch scratch(int32_t R, int32_t L, int32_t batch)
    {
        SqCovarWstatNullScratch s;
        s.planes = 0;
        s.partial = s.planes + (int64_t)batch * SqCovar::plane_words(R, L);
        s.mean = s.partial + (int64_t)batch * SqCovarStat::partial_words(L);
        s.cls = s.mean + (int64_t)batch * ((int64_t)L + 1);
        s.q = s.cls + SqCovarStatNull::class_words(R, L);                // = SqCovarStatNull::scratch_words(R, L, batch)
        s.words = s.q + SqCovarWstat::rpad(R) / 2;
        return s;
    }
};
