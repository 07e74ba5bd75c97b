// Covariation statistics of two alignment columns (sq_covariation_stat_scan / sq_covariation_stat_pairs,
// CovariationStatistics): mutual information, the G-test and chi-square of the 4 x 4 joint table of residues at two columns
// v < w, raw and with a background correction from the column means (APC, ASC).
//
// Joint table.  n[a * 4 + b], a and b in A C G U, = the rows with residue a at v and residue b at w, from the bit planes A, C,
// G, U of sq_covar.h (the classes of SqCovar::cls): 16 AND + popcounts per 64-row word.  A row with a gap or "other" at either
// column takes part in nothing; the gap plane is not read.  N = the sum of n, na[a] = the sum over b, nb[b] = the sum over a.
//
// Raw statistic S (raw()).  A double from the 16 counters, the terms added in the order ab = 0 .. 15, 0 when N == 0:
//   mi   the sum over n > 0 of (n / N) * ln(n * N / (na * nb))                 (nats)
//   gt   2 * the sum over n > 0 of n * ln(n * N / (na * nb))
//   chi  the sum over na * nb > 0 of (n - e)^2 / e, e = na * nb / N            (cells with n == 0 included)
// The ratio form: one log of one quotient per term (the entropy form cancels).  A fully conserved pair of columns has
// n = N = na = nb in its one cell: the quotient is 1, ln 1 == 0 and S == 0.0 exactly.  n * N and na * nb are formed as int64
// (the counters are below 2^31) and divided as doubles.  The function is the only place S is formed, with FP contraction off
// inside it whatever the build's flags: pass 1, pass 2, the pairs lookup and the host give the same bits for the same counters.
//
// Column means.  sum[c] = the sum over c' != c of S(c, c'), mean[c] = sum[c] / (L - 1), over every pair of distinct columns
// (no minspan, no threshold).  mean_all = the mean of S over v < w = the sum of mean[c] over c, divided by L (each S is in two
// column sums; the same number as the sum of S over v < w divided by L (L - 1) / 2 but for the last bits).  The device forms
// them in a fixed order (sq_covar_stat_dev.hip): per tile the cells of a column ascending, per column its tiles ascending,
// the columns ascending in 256 strided runs and the runs ascending.  The array mean[] has L + 1
// doubles: mean[L] = mean_all.  With L == 1 all of it is 0.
//
// Corrected statistic C (corrected()).  apc: S - mean[v] * mean[w] / mean_all, or S when mean_all == 0; asc:
// S - (mean[v] + mean[w] - mean_all); none: S.
//
// This header compiles for the device and for the host (tests/native/covar_stat_host.cpp runs it as one thread).
#pragma once
#include <stdint.h>
#include <math.h>
#include "sq_covar.h"

// The scans' tile of columns, the 64-row words of the four planes they keep in LDS at a time and the most blocks they launch
// (the rest by grid stride).  squarna_amd/device_calls.py holds the same three numbers for the tests.
// SQ_COVSTAT_CELLS: the cells whose 16 counters a thread keeps at a time, 1, 2 or 4 (a tile is 4 cells per thread, walked in
// 4 / CELLS passes that each stage the planes again).  The compiler's figures for gfx950, pass 1 / pass 2: with 4 cells 204 /
// 204 VGPRs, two waves per SIMD; with 2 cells 142 / 152 VGPRs, three waves per SIMD.  S of one cell alone (16 unrolled
// logarithms on 16 counters) takes 90 VGPRs in the pairs kernel, so a third cell's 16 counters would already cost the third
// wave.  LDS does not bind: 17 KB (pass 1) and 24 KB (pass 2) a block.  The null's scan (sq_covar_stat_null_scan_kernel,
// sq_covar_stat_null.h) keeps the shape: with 2 cells 160 VGPRs, three waves per SIMD, and 32 KB of LDS a block (the planes,
// 2048 thresholds and 2048 bins), three blocks in a CU's 160 KB; its pairs kernel takes 94 VGPRs.
#define SQ_COVSTAT_TILE 32
#define SQ_COVSTAT_WORD_CHUNK 4
#define SQ_COVSTAT_MAX_BLOCKS 2048
#define SQ_COVSTAT_CELLS 2

enum { SQ_COVSTAT_MI = 0, SQ_COVSTAT_GT = 1, SQ_COVSTAT_CHI = 2, SQ_COVSTAT_STATS = 3 };
enum { SQ_COVSTAT_NONE = 0, SQ_COVSTAT_APC = 1, SQ_COVSTAT_ASC = 2, SQ_COVSTAT_CORRECTIONS = 3 };

// SQ_COVSTAT_UNROLL: the loops over the 16 cells are unrolled for the device, so that the counters stay in registers.
#if defined(__clang__)
#define SQ_COVSTAT_UNROLL _Pragma("unroll")
#define SQ_COVSTAT_NO_CONTRACT
#define SQ_COVSTAT_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define SQ_COVSTAT_UNROLL
#define SQ_COVSTAT_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#define SQ_COVSTAT_NO_CONTRACT_BODY
#else
#define SQ_COVSTAT_UNROLL
#define SQ_COVSTAT_NO_CONTRACT
#define SQ_COVSTAT_NO_CONTRACT_BODY
#endif

struct SqCovarStat {
    // ---- the scratch of the two entries: the planes of sq_covar.h, then the partial column sums of pass 1,
    // partial[t * Lpad + c] = what the tile that column c shares with tile index t adds to sum[c] (sq_covar_stat_dev.hip)
    SQ_COV_HD static int64_t tiles(int32_t L) { return ((int64_t)L + SQ_COVSTAT_TILE - 1) / SQ_COVSTAT_TILE; }
    SQ_COV_HD static int64_t partial_words(int32_t L) { return tiles(L) * SqCovar::lpad(L); }
    SQ_COV_HD static int64_t scratch_words(int32_t R, int32_t L) { return SqCovar::plane_words(R, L) + partial_words(L); }

    // ---- one 64-row word of two columns: the 16 cells of the joint table (a, b: the planes A C G U of v and of w)
    SQ_COV_HD static void accumulate(const uint64_t a[4], const uint64_t b[4], int32_t n[16])
    {
        SQ_COVSTAT_UNROLL
        for (int x = 0; x < 4; x++)
        SQ_COVSTAT_UNROLL
            for (int y = 0; y < 4; y++) n[x * 4 + y] += __builtin_popcountll(a[x] & b[y]);
    }

    SQ_COV_HD static int64_t rows(const int32_t n[16])
    {
        int64_t N = 0;
        SQ_COVSTAT_UNROLL
        for (int k = 0; k < 16; k++) N += n[k];
        return N;
    }

    // ---- S of a cell's counters
    SQ_COVSTAT_NO_CONTRACT SQ_COV_HD static double raw(int stat, const int32_t n[16])
    {
        SQ_COVSTAT_NO_CONTRACT_BODY
        int64_t na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0}, N = 0;
        SQ_COVSTAT_UNROLL
        for (int k = 0; k < 16; k++) {
            na[k >> 2] += n[k];
            nb[k & 3] += n[k];
            N += n[k];
        }
        if (N == 0) return 0.0;
        double s = 0.0;
        SQ_COVSTAT_UNROLL
        for (int k = 0; k < 16; k++) {
            const int64_t margins = na[k >> 2] * nb[k & 3];           // (< 2^62)
            if (stat == SQ_COVSTAT_CHI) {
                if (margins > 0) {
                    const double e = (double)margins / (double)N, d = (double)n[k] - e;
                    s += d * d / e;
                }
            } else if (n[k] > 0) {
                const double l = log((double)((int64_t)n[k] * N) / (double)margins);
                s += (stat == SQ_COVSTAT_MI ? (double)n[k] / (double)N : (double)n[k]) * l;
            }
        }
        return stat == SQ_COVSTAT_GT ? 2.0 * s : s;
    }

    // ---- C from S and the means of the two columns
    SQ_COVSTAT_NO_CONTRACT SQ_COV_HD static double corrected(int corr, double S, double mean_v, double mean_w, double mean_all)
    {
        SQ_COVSTAT_NO_CONTRACT_BODY
        if (corr == SQ_COVSTAT_APC) return mean_all == 0.0 ? S : S - mean_v * mean_w / mean_all;
        if (corr == SQ_COVSTAT_ASC) return S - (mean_v + mean_w - mean_all);
        return S;
    }

    // ---- which cells the scan emits (in scope: SqCovar::in_scope)
    SQ_COV_HD static bool emits(int64_t N, double C, int32_t min_rows, double min_stat) { return N >= min_rows && C >= min_stat; }
};
