// Row identities of an alignment (sq_row_identity, RowIdentity): how alike two rows are, how many rows lie within a threshold
// of a row, and which rows a greedy redundancy filter keeps, in integers.
//
// Bytes.  A row byte has the class SqCovar::cls() gives it (sq_covar.h): 0..3 = A C G U, 4 = a gap, 5 = "other".  A residue is
// any non-gap, "other" included; a base is A, C, G or U.  "Other" matches nothing, not even itself.
//
// Planes.  The alignment of R rows and L columns is kept bit-sliced along the rows: four planes (the two bits of the base's
// class, `base`, `residue`) of Wc = ceil(L / 64) words of 64 columns per row, bit c % 64 of word c / 64 set when the row's byte
// at column c has the plane's property.  Bits of columns >= L are zero, and so are the words of the rows R .. Rpad - 1, Rpad = R
// rounded up to 64.  Word w of plane p of row r is plane[(p * Wc + w) * Rpad + r]: the row runs fastest, so one word of 64
// consecutive rows is one contiguous load per plane, and consecutive lanes read consecutive 8-byte words of LDS.
//
// Counts.  For one word of two rows accumulate() adds the columns where both hold the same base (`same`) and the columns
// where both hold a residue (`both`).  len[a] = both[a, a], bases[a] = same[a, a].  The denominator of a pair is
// min(len[a], len[b]) ("shorter": Easel's pairwise identity), both[a, b] ("aligned") or L ("columns"); rows a != b are
// neighbours at T basis points iff den > 0 and same * 10000 >= T * den, in int64.
//
// Tiles.  Rows are compared in tiles of SQ_ID_TILE x SQ_ID_TILE cells, the upper triangle (ta <= tb) of nT x nT tiles in the
// order of SqCovar::tile_of(); a tile off the diagonal also stands for its mirror image.  The neighbours of row a among the 64
// rows of tile t are bit b % 64 of nbr[a * Wr + t], Wr = ceil(R / 64): a bit matrix uint64[R x Wr].
//
// Filter.  keep[a], greedy in row order: row a is kept iff no kept row b < a is its neighbour.  The kept rows are a bit array
// of Wr words; row a tests kept & nbr[a] over the words_below(a) words that hold the rows below it (the bits of the rows >= a
// are still zero there, and a row is not its own neighbour).
//
// This header compiles for the device and for the host (tests/native/identity_host.cpp runs it as one thread).
#pragma once
#include <stdint.h>
#include "sq_covar.h"

#ifdef __HIPCC__
#define SQ_ID_HD __host__ __device__
#else
#define SQ_ID_HD
#endif

// The pairs kernel's tile: SQ_ID_TILE x SQ_ID_TILE cells of rows (64: a neighbour word is one wave ballot), the planes of both
// row ranges in LDS SQ_ID_WORD_CHUNK words (64 columns each) at a time.  At most SQ_ID_MAX_BLOCKS blocks, the rest by grid
// stride.  At most SQ_ID_MAX_ROWS rows (the bit matrix is then 512 MB) of at most SQ_ID_MAX_COLS columns; a lane of the filter kernel
// holds SQ_ID_FILTER_WORDS words of neighbour bits of the rows ahead, loaded or on their way.
// squarna_amd/device_calls.py holds the same numbers for the tests.
#define SQ_ID_MAX_BLOCKS 2048
#define SQ_ID_TILE 64
#define SQ_ID_WORD_CHUNK 4
#define SQ_ID_MAX_ROWS 65535
#define SQ_ID_MAX_COLS (1 << 21)
#define SQ_ID_FILTER_WORDS 64

enum { SQ_ID_CODE0 = 0, SQ_ID_CODE1 = 1, SQ_ID_BASE = 2, SQ_ID_RES = 3, SQ_ID_PLANES = 4 };
enum { SQ_ID_DEN_SHORTER = 0, SQ_ID_DEN_ALIGNED = 1, SQ_ID_DEN_COLUMNS = 2, SQ_ID_DENS = 3 };

struct SqIdentity {
    // the planes a byte of class cls (SqCovar::cls) sets, bit p for plane p
    SQ_ID_HD static uint32_t plane_bits(int cls)
    {
        if (cls < SQ_COV_GAP) return (uint32_t)cls | 1u << SQ_ID_BASE | 1u << SQ_ID_RES;
        return cls == SQ_COV_GAP ? 0u : 1u << SQ_ID_RES;
    }

    // ---- the plane layout and the bit matrix
    SQ_ID_HD static int64_t col_words(int32_t L) { return ((int64_t)L + 63) / 64; }
    SQ_ID_HD static int64_t row_words(int32_t R) { return ((int64_t)R + 63) / 64; }
    SQ_ID_HD static int64_t rpad(int32_t R) { return row_words(R) * 64; }
    SQ_ID_HD static int64_t plane_words(int32_t R, int32_t L) { return (int64_t)SQ_ID_PLANES * col_words(L) * rpad(R); }
    SQ_ID_HD static int64_t nbr_words(int32_t R) { return (int64_t)R * row_words(R); }
    SQ_ID_HD static int64_t at(int p, int64_t w, int64_t row, int64_t Wc, int64_t Rpad) { return ((int64_t)p * Wc + w) * Rpad + row; }

    // ---- the tile walk: the upper triangle of nT x nT tiles of rows, row after row (SqCovar's)
    SQ_ID_HD static int64_t tiles(int32_t R) { return (rpad(R) + SQ_ID_TILE - 1) / SQ_ID_TILE; }
    SQ_ID_HD static int64_t tile_count(int64_t nT) { return SqCovar::tile_count(nT); }
    SQ_ID_HD static void tile_of(int64_t k, int64_t nT, int32_t &ta, int32_t &tb) { SqCovar::tile_of(k, nT, ta, tb); }

    // ---- one 64-column word of two rows
    SQ_ID_HD static void accumulate(const uint64_t a[SQ_ID_PLANES], const uint64_t b[SQ_ID_PLANES], int32_t &same, int32_t &both)
    {
        same += __builtin_popcountll(~(a[SQ_ID_CODE0] ^ b[SQ_ID_CODE0]) & ~(a[SQ_ID_CODE1] ^ b[SQ_ID_CODE1]) & a[SQ_ID_BASE] & b[SQ_ID_BASE]);
        both += __builtin_popcountll(a[SQ_ID_RES] & b[SQ_ID_RES]);
    }

    // ---- the three denominators and the neighbour test
    SQ_ID_HD static int64_t den(int32_t kind, int32_t len_a, int32_t len_b, int32_t both, int32_t L)
    {
        return kind == SQ_ID_DEN_SHORTER ? (len_a < len_b ? len_a : len_b) : kind == SQ_ID_DEN_ALIGNED ? both : L;
    }
    // (same <= den <= 2^21 and T <= 10000: every product is below 2^35)
    SQ_ID_HD static bool within(int64_t same, int64_t den, int32_t T) { return den > 0 && same * 10000 >= (int64_t)T * den; }
    // rows a and b of the R rows are neighbours: two different rows of the alignment within the threshold
    SQ_ID_HD static bool neighbours(int64_t a, int64_t b, int32_t R, int32_t same, int32_t both, int32_t len_a, int32_t len_b, int32_t L,
                                    int32_t kind, int32_t T)
    {
        return a != b && a < R && b < R && within(same, den(kind, len_a, len_b, both, L), T);
    }

    // ---- the greedy filter over the neighbour bit words
    SQ_ID_HD static int64_t words_below(int64_t a) { return a / 64 + 1; }
    SQ_ID_HD static bool word_hits(uint64_t kept, uint64_t nbr) { return (kept & nbr) != 0; }
    SQ_ID_HD static uint64_t row_bit(int64_t a) { return 1ull << (a % 64); }
    // the filter as one thread: kept = Wr words, all zero before; returns the number of kept rows
    SQ_ID_HD static int32_t greedy(const uint64_t *nbr, int32_t R, uint64_t *kept)
    {
        const int64_t Wr = row_words(R);
        int32_t n = 0;
        for (int64_t a = 0; a < R; a++) {
            bool hit = false;
            for (int64_t w = 0; w < words_below(a) && !hit; w++) hit = word_hits(kept[w], nbr[a * Wr + w]);
            if (!hit) {
                kept[a / 64] |= row_bit(a);
                n++;
            }
        }
        return n;
    }
};
