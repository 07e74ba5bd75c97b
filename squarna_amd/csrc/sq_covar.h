// Covariation evidence for two alignment columns (sq_covariation_scan / sq_covariation_pairs, Covariation): how the rows of
// an alignment support a pair of columns v < w, in integers.
//
// Bytes.  A row byte is upper-cased and T reads as U; it is then one of A, C, G, U, a gap ('-', '.', '~') or "other"
// (everything else, separators included).  cls() gives the class: 0..3 = A C G U, 4 = gap, 5 = other.
//
// Planes.  The alignment of R rows and L columns is kept bit-sliced: five planes (A, C, G, U, gap) of W = ceil(R / 64) words of
// 64 rows per column, bit r % 64 of word r / 64 set when row r's byte at the column has the plane's class.  Bits of rows >= R
// are zero and "other" has no plane: it takes part in nothing but `incompatible`.  Word w of plane p of column c is
// plane[(p * W + w) * Lpad + c], Lpad = L rounded up to 64 with the columns >= L all zero: the column runs fastest, so a tile of
// consecutive columns is one contiguous load per plane and word, and consecutive lanes read consecutive 8-byte words of LDS.
//
// Counts.  The six canonical pair types are AU UA GC CG GU UG, in this order.  For one word of two columns accumulate() adds
// the rows of every type (popcounts of the AND of two planes) and the rows with a gap in both columns: seven counters,
// cnt[0..5] = c[t], cnt[6] = both_gap.  From them bp_rows = the sum of c, incompatible = R - bp_rows - both_gap, and
//   cov = the sum over t < t' of c[t] * c[t'] * d(t, t'),   d = the Hamming distance of the two two-letter strings,
// which is the sum, over the unordered pairs of rows that both hold a canonical pair, of the distance of the two pairs.
//
// This header compiles for the device and for the host (tests/native/covar_host.cpp runs it as one thread).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SQ_COV_HD __host__ __device__
#else
#define SQ_COV_HD
#endif

// The scan's tile: SQ_COV_TILE x SQ_COV_TILE cells of columns, the planes of both column ranges in LDS SQ_COV_WORD_CHUNK words
// (64 rows each) at a time (4, not 8: 121 VGPRs and 46 KB of LDS instead of 176 and 56 KB, three blocks per CU instead of two, and
// the scan of 512 x 5000 took 10 % less time).  At most SQ_COV_MAX_BLOCKS blocks, the rest by grid stride (sq_covar_dev.hip says
// why 2048).
// squarna_amd/device_calls.py holds the same three numbers for the tests.
#define SQ_COV_TILE 32
#define SQ_COV_WORD_CHUNK 4
#define SQ_COV_MAX_BLOCKS 2048

enum { SQ_COV_A = 0, SQ_COV_C = 1, SQ_COV_G = 2, SQ_COV_U = 3, SQ_COV_GAP = 4, SQ_COV_OTHER = 5, SQ_COV_PLANES = 5 };

struct SqCovar {
    // the class of a row byte
    SQ_COV_HD static int cls(uint8_t b)
    {
        if (b >= 'a' && b <= 'z') b = (uint8_t)(b - 'a' + 'A');
        switch (b) {
        case 'A': return SQ_COV_A;
        case 'C': return SQ_COV_C;
        case 'G': return SQ_COV_G;
        case 'U': case 'T': return SQ_COV_U;
        case '-': case '.': case '~': return SQ_COV_GAP;
        default: return SQ_COV_OTHER;
        }
    }

    // ---- the plane layout
    SQ_COV_HD static int64_t words(int32_t R) { return ((int64_t)R + 63) / 64; }
    SQ_COV_HD static int64_t lpad(int32_t L) { return ((int64_t)L + 63) / 64 * 64; }
    SQ_COV_HD static int64_t plane_words(int32_t R, int32_t L) { return (int64_t)SQ_COV_PLANES * words(R) * lpad(L); }
    SQ_COV_HD static int64_t at(int p, int64_t w, int64_t col, int64_t W, int64_t Lpad) { return ((int64_t)p * W + w) * Lpad + col; }

    // ---- the scan's tiles: the upper triangle (ti <= tj) of nT x nT tiles, row after row; tile_count(nT) of them
    SQ_COV_HD static int64_t tile_count(int64_t nT) { return nT * (nT + 1) / 2; }
    SQ_COV_HD static int64_t tile_row_start(int64_t ti, int64_t nT) { return ti * nT - ti * (ti - 1) / 2; }
    // Tile k < tile_count(nT): its row ti and column tj.  The estimate of ti comes from the root of the tiles that lie behind
    // k; the two loops mend what the root's rounding leaves (nT < 2^26, so the numbers are exact in a double up to that).
    SQ_COV_HD static void tile_of(int64_t k, int64_t nT, int32_t &ti, int32_t &tj)
    {
        const int64_t behind = tile_count(nT) - 1 - k;                // tiles behind k: row ti has nT - ti
        int64_t m = (int64_t)((__builtin_sqrt(8.0 * (double)behind + 1.0) - 1.0) * 0.5);   // rows that lie wholly behind k
        while (m > 0 && tile_count(m) > behind) m--;
        while (tile_count(m + 1) <= behind) m++;
        const int64_t row = nT - 1 - m;
        ti = (int32_t)row;
        tj = (int32_t)(row + (k - tile_row_start(row, nT)));
    }

    // ---- one 64-row word of two columns: the six types and both_gap
    SQ_COV_HD static void accumulate(const uint64_t a[5], const uint64_t b[5], int32_t cnt[7])
    {
        cnt[0] += __builtin_popcountll(a[SQ_COV_A] & b[SQ_COV_U]);
        cnt[1] += __builtin_popcountll(a[SQ_COV_U] & b[SQ_COV_A]);
        cnt[2] += __builtin_popcountll(a[SQ_COV_G] & b[SQ_COV_C]);
        cnt[3] += __builtin_popcountll(a[SQ_COV_C] & b[SQ_COV_G]);
        cnt[4] += __builtin_popcountll(a[SQ_COV_G] & b[SQ_COV_U]);
        cnt[5] += __builtin_popcountll(a[SQ_COV_U] & b[SQ_COV_G]);
        cnt[6] += __builtin_popcountll(a[SQ_COV_GAP] & b[SQ_COV_GAP]);
    }

    SQ_COV_HD static int32_t bp_rows(const int32_t cnt[7]) { return cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + cnt[5]; }

    // cov of a cell's counters.  d is 2 but for AU-GU, UA-UG, GC-GU and CG-UG, which differ in one letter.  The six counters sum
    // to at most the alignment's rows, R < 2^31: every number formed here is below R^2 < 2^62.
    SQ_COV_HD static int64_t finish(const int32_t cnt[7])
    {
        const int64_t n = bp_rows(cnt);
        int64_t squares = 0;
        for (int t = 0; t < 6; t++) squares += (int64_t)cnt[t] * cnt[t];
        const int64_t ones = (int64_t)cnt[4] * ((int64_t)cnt[0] + cnt[2]) + (int64_t)cnt[5] * ((int64_t)cnt[1] + cnt[3]);
        return n * n - squares - ones;                               // (n^2 - squares = 2 * the sum over t < t' of c[t] c[t'])
    }

    // ---- which cells the scan covers and which of them it emits
    SQ_COV_HD static bool in_scope(int64_t v, int64_t w, int32_t L, int32_t minspan) { return v < w && w < L && w - v >= minspan; }
    SQ_COV_HD static bool emits(const int32_t cnt[7], int64_t cov, int32_t min_rows, int64_t min_cov)
    {
        return bp_rows(cnt) >= min_rows && cov >= min_cov;
    }
    // a pair of sq_covariation_pairs that has a record
    SQ_COV_HD static bool valid_pair(int32_t v, int32_t w, int32_t L) { return v >= 0 && v < w && w < L; }
};
