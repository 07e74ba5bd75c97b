// Base-pair distances of structures (sq_structure_distances, Distances): how many pairs two structures share, which structures
// lie within a radius of a structure, and which structures a greedy filter in row order keeps, in integers.
//
// Rows.  A structure is a partner row p of `width` columns, p[i] = the partner of column i or -1.  Its pairs are
// {(i, p[i]) : p[i] > i}; npairs[a] = their number, common[a, b] = the pairs two rows share, and the base-pair distance is
// d(a, b) = npairs[a] + npairs[b] - 2 common[a, b].  A row is invalid when a partner lies outside [-1, width), p[p[i]] != i or
// p[i] == i: it has no pair, shares none and is nobody's neighbour.
//
// Planes.  The S rows are kept bit-sliced along the rows, in the layout of sq_identity.h: plane SQ_DIST_OPEN has the bit of
// column i set when i opens a pair, and the B = span_bits(Wmax) planes after it hold the bits of the span p[i] - i of the
// opening columns (1 <= span <= Wmax - 1, Wmax = the widest row; at most 15 bits, 16 planes in all).  Two rows share the pair
// that column i opens iff both open one there and every span bit agrees.  Word w (64 columns) of plane p of row r is
// plane[SqIdentity::at(p, w, r, Wc, Spad)], Wc = ceil(Wmax / 64), Spad = S rounded up to 64; the bits of the columns beyond a
// row's width, the planes of an invalid row and the words of the rows S .. Spad - 1 are zero.
//
// Groups.  Rows are compared within a group only; the rows of a group are consecutive: group g has the rows group_off[g] ..
// group_off[g + 1] - 1, row_group[r] = the group of row r.  common[] is block-diagonal: the cell (a, b) of group g, of n_g rows
// from row `first` on, sits at mat_off[g] + (a - first) * n_g + (b - first).
//
// Tiles.  Rows are compared in tiles of SQ_DIST_TILE x SQ_DIST_TILE cells over the GLOBAL row index; only the upper-triangle
// tiles (ta <= tb) that hold a cell of one group are planned (plan_tiles): ta == tb, or the last row of tile ta and the first
// row of tile tb lie in one group.  A tile off the diagonal also stands for its mirror image.  The neighbours of row a among
// the 64 rows of tile t are bit b % 64 of nbr[a * Wr + t], Wr = ceil(S / 64); the filter reads the words first / 64 .. a / 64
// of a row a of a group that starts at `first`, and each of them belongs to exactly one planned tile.
//
// Filter.  keep[a], greedy in row order within the group: row a is kept iff no kept row below it in its group is its
// neighbour; leader[a] = a when kept, else the lowest kept neighbour below it.
//
// This header compiles for the device and for the host (tests/native/distances_host.cpp runs it as one thread).
#pragma once
#include <stdint.h>
#include "sq_identity.h"

// The pairs kernel's tile and the 64-column words of both row ranges it keeps in LDS at a time (2 x 16 planes x 2 words x 64
// rows x 8 bytes = 32 KB); the most blocks it and the filter kernel launch; the most rows, columns and planes; the words of
// neighbour bits a lane of the filter kernel holds ahead.  squarna_amd/device_calls.py holds the same numbers for the tests.
#define SQ_DIST_TILE 64
#define SQ_DIST_WORD_CHUNK 2
#define SQ_DIST_MAX_BLOCKS 2048
#define SQ_DIST_MAX_ROWS 65535
#define SQ_DIST_MAX_COLS 32768
#define SQ_DIST_MAX_PLANES 16
#define SQ_DIST_FILTER_WORDS 64

enum { SQ_DIST_OPEN = 0, SQ_DIST_SPAN0 = 1 };
enum { SQ_DIST_RADIUS = 0, SQ_DIST_RELATIVE = 1, SQ_DIST_MODES = 2 };
// the bits of the status word (d_out[1]): a tile entry outside the tile range; a group the filter cannot take
enum { SQ_DIST_BAD_TILE = 1, SQ_DIST_BAD_GROUP = 2 };

struct SqDistances {
    // ---- the planes: `open` and the bits of the largest span Wmax - 1
    SQ_ID_HD static int32_t span_bits(int32_t Wmax)
    {
        int32_t bits = 0;
        for (int64_t v = (int64_t)Wmax - 1; v > 0; v >>= 1) bits++;
        return bits;
    }
    SQ_ID_HD static int32_t planes(int32_t Wmax) { return 1 + span_bits(Wmax); }
    SQ_ID_HD static int64_t col_words(int32_t Wmax) { return SqIdentity::col_words(Wmax); }
    SQ_ID_HD static int64_t row_words(int32_t S) { return SqIdentity::row_words(S); }
    SQ_ID_HD static int64_t spad(int32_t S) { return SqIdentity::rpad(S); }
    SQ_ID_HD static int64_t plane_words(int32_t S, int32_t Wmax) { return (int64_t)planes(Wmax) * col_words(Wmax) * spad(S); }
    SQ_ID_HD static int64_t nbr_words(int32_t S) { return SqIdentity::nbr_words(S); }
    SQ_ID_HD static int64_t scratch_words(int32_t S, int32_t Wmax) { return plane_words(S, Wmax) + nbr_words(S); }

    // ---- one column of a row: is the partner p of column c of a row of `width` columns (whose partner's partner is `back`,
    // read only when 0 <= p < width) a fault of the row?
    SQ_ID_HD static bool partner_in_range(int32_t p, int32_t width) { return p >= -1 && p < width; }
    SQ_ID_HD static bool column_bad(int32_t c, int32_t p, int32_t back, int32_t width)
    {
        return !partner_in_range(p, width) || p == c || (p >= 0 && back != c);
    }
    // the planes column c with partner p sets, bit k for plane k (a valid row: p > c means 1 <= p - c <= width - 1)
    SQ_ID_HD static uint32_t plane_bits(int32_t c, int32_t p) { return p > c ? 1u | (uint32_t)(p - c) << SQ_DIST_SPAN0 : 0u; }

    // ---- one 64-column word of two rows, of np planes each
    SQ_ID_HD static int32_t common_word(const uint64_t *a, const uint64_t *b, int32_t np)
    {
        uint64_t m = a[SQ_DIST_OPEN] & b[SQ_DIST_OPEN];
        for (int32_t p = SQ_DIST_SPAN0; p < np; p++) m &= ~(a[p] ^ b[p]);
        return __builtin_popcountll(m);
    }

    // ---- the distance and the two neighbour tests (npairs <= 16384, T <= 10000: every product is below 2^29)
    SQ_ID_HD static int64_t distance(int32_t na, int32_t nb, int32_t common) { return (int64_t)na + nb - 2 * (int64_t)common; }
    SQ_ID_HD static bool within_radius(int32_t na, int32_t nb, int32_t common, int32_t k) { return distance(na, nb, common) <= k; }
    SQ_ID_HD static bool within_relative(int32_t na, int32_t nb, int32_t common, int32_t T)
    {
        return distance(na, nb, common) * 10000 <= (int64_t)T * ((int64_t)na + nb);
    }
    SQ_ID_HD static bool within(int32_t mode, int32_t threshold, int32_t na, int32_t nb, int32_t common)
    {
        return mode == SQ_DIST_RADIUS ? within_radius(na, nb, common, threshold) : within_relative(na, nb, common, threshold);
    }
    // rows a and b are neighbours: two different valid rows of one group within the threshold (ga, gb: their groups, -1 for a
    // row that has none, such as a row >= S)
    SQ_ID_HD static bool neighbours(int64_t a, int64_t b, int32_t ga, int32_t gb, bool valid_a, bool valid_b, int32_t mode, int32_t threshold,
                                    int32_t na, int32_t nb, int32_t common)
    {
        return a != b && ga >= 0 && ga == gb && valid_a && valid_b && within(mode, threshold, na, nb, common);
    }

    // ---- the block-diagonal matrix
    SQ_ID_HD static int64_t cell(int64_t mat_off_g, int64_t first, int64_t n_g, int64_t a, int64_t b)
    {
        return mat_off_g + (a - first) * n_g + (b - first);
    }
    // mat_off[G + 1] of the groups group_off[G + 1]; returns the cells of all groups
    static int64_t matrix_offsets(const int32_t *group_off, int32_t G, int64_t *mat_off)
    {
        mat_off[0] = 0;
        for (int32_t g = 0; g < G; g++) {
            const int64_t n = (int64_t)group_off[g + 1] - group_off[g];
            mat_off[g + 1] = mat_off[g] + n * n;
        }
        return mat_off[G];
    }

    // ---- the tile plan: the upper-triangle tiles that hold a cell of one group, row after row.  row_group[S] ascends.
    SQ_ID_HD static int64_t tiles(int32_t S) { return SqIdentity::tiles(S); }
    SQ_ID_HD static bool tile_planned(const int32_t *row_group, int32_t S, int64_t ta, int64_t tb)
    {
        if (ta == tb) return true;
        const int64_t last = ta * SQ_DIST_TILE + SQ_DIST_TILE - 1, first = tb * SQ_DIST_TILE;
        return last < S && first < S && row_group[last] == row_group[first];
    }
    // tiles[2 k], tiles[2 k + 1] = (ta, tb) of the k-th planned tile, when tiles is given; returns their number
    static int64_t plan_tiles(const int32_t *row_group, int32_t S, int32_t *tiles_out)
    {
        const int64_t nT = tiles(S);
        int64_t n = 0;
        for (int64_t ta = 0; ta < nT; ta++)
            for (int64_t tb = ta; tb < nT && tile_planned(row_group, S, ta, tb); tb++) {   // (a group's rows are consecutive)
                if (tiles_out) {
                    tiles_out[2 * n] = (int32_t)ta;
                    tiles_out[2 * n + 1] = (int32_t)tb;
                }
                n++;
            }
        return n;
    }
    SQ_ID_HD static bool tile_in_range(int32_t ta, int32_t tb, int64_t nT) { return ta >= 0 && ta <= tb && tb < nT; }

    // ---- the greedy filter over the neighbour bit words of the rows first .. last - 1 of one group
    SQ_ID_HD static int64_t first_word(int64_t first) { return first / 64; }
    // the words a group spans: those the rows first .. last - 1 lie in (0 for an empty group)
    SQ_ID_HD static int64_t group_words(int64_t first, int64_t last) { return last > first ? (last - 1) / 64 - first / 64 + 1 : 0; }
    // the lowest kept neighbour in word w of a row, given the word of the kept mask and of the row: its global row index
    SQ_ID_HD static int64_t lowest_hit(int64_t w, uint64_t kept, uint64_t nbr) { return w * 64 + __builtin_ctzll(kept & nbr); }
    // The filter of one group as one thread: kept = at least group_words(first, last) words, all zero before (word 0 stands
    // for word first_word(first) of the rows); valid[a] != 0 for a row that takes part.  keep[] and leader[] of the group's
    // rows are written.  Returns the number of kept rows.
    static int32_t greedy(const uint64_t *nbr, int64_t Wr, int64_t first, int64_t last, const uint8_t *valid, uint64_t *kept, uint8_t *keep,
                          int32_t *leader)
    {
        const int64_t w0 = first_word(first);
        int32_t n = 0;
        for (int64_t a = first; a < last; a++) {
            keep[a] = 0;
            leader[a] = -1;
            if (!valid[a]) continue;
            for (int64_t w = w0; w < SqIdentity::words_below(a) && leader[a] < 0; w++)
                if (SqIdentity::word_hits(kept[w - w0], nbr[a * Wr + w])) leader[a] = (int32_t)lowest_hit(w, kept[w - w0], nbr[a * Wr + w]);
            if (leader[a] < 0) {
                kept[a / 64 - w0] |= SqIdentity::row_bit(a);
                keep[a] = 1;
                leader[a] = (int32_t)a;
                n++;
            }
        }
        return n;
    }
};
