// Structures between the columns of an alignment and the residues of its rows (sq_project_rows, sq_lift_rows; Project, Lift):
// the gap map of a row, a structure over the columns projected onto the row's residues with the class of every pair in that
// row, and a structure over a row's residues lifted onto the columns.  All numbers are integers.
//
// Bytes.  A row byte has the class SqCovar::cls() gives it (sq_covar.h): 0..3 = A C G U, 4 = a gap, 5 = "other"; the kernels
// read it from a 256-entry table (fill_table).  A residue is any non-gap, "other" included.
//
// Gap map.  The L columns of a row are walked in chunks of 64: word[j] has bit c % 64 set when column c = 64 j + c % 64 holds
// a residue (bits of columns >= L are zero), base[j] = the residues of the chunks before j, base[nW] = the row's length,
// nW = ceil(L / 64).  The residue index of a residue column c is pos(c) = base[c >> 6] + popcount(word[c >> 6] & below(c & 63));
// for any column, rank(c) is the same sum: the residues left of c.  The column of residue i is col(i): the last chunk j with
// base[j] <= i (an upper bound over the bases: an empty chunk has its successor's base and is passed over), then the
// (i - base[j])-th set bit of word[j] (select64).  No table of L entries is kept.
//
// Structures.  A structure is a row of partners, p[i] = the partner of i or -1.  A row is invalid when a partner lies outside
// [-1, width), p[p[i]] != i or p[i] == i (column_bad: Distances' rule).
//
// Pair classes.  The class of a pair (v, w), v < w, in a row is read from the two class bytes in that order: 1..6 = AU UA GC CG
// GU UG, 7 = two residues that are no canonical pair, 8 = a gap in exactly one column, 9 = a gap in both.  A pair is kept in
// the projected row iff its class is 1..6, or 7 unless canonical_only, and the residues strictly between its ends number at
// least min_loop.  counts[12] of a line: [0] its pairs, [1..9] the pairs per class, [10] the pairs of class 1..7 that min_loop
// alone drops, [11] the pairs kept.
//
// This header compiles for the device and for the host (tests/native/project_host.cpp runs it as one thread).
#pragma once
#include <stdint.h>
#include "sq_covar.h"

#ifdef __HIPCC__
#define SQ_PROJ_HD __host__ __device__
#else
#define SQ_PROJ_HD
#endif

// The threads of a block (one block per alignment row at a time), the most blocks launched (the rest by grid stride), the
// most columns and rows, the chunk words of the longest row and the counters of a line.  squarna_amd/device_calls.py holds
// the same numbers for the tests.
#define SQ_PROJ_THREADS 256
#define SQ_PROJ_MAX_BLOCKS 2048
#define SQ_PROJ_MAX_COLS 32768
#define SQ_PROJ_MAX_ROWS (1 << 20)
#define SQ_PROJ_MAX_WORDS (SQ_PROJ_MAX_COLS / 64)
#define SQ_PROJ_COUNTS 12

enum { SQ_PROJ_NONE = 0, SQ_PROJ_AU = 1, SQ_PROJ_UA = 2, SQ_PROJ_GC = 3, SQ_PROJ_CG = 4, SQ_PROJ_GU = 5, SQ_PROJ_UG = 6,
       SQ_PROJ_NONCANONICAL = 7, SQ_PROJ_ONE_GAP = 8, SQ_PROJ_BOTH_GAP = 9 };
enum { SQ_PROJ_CNT_PAIRS = 0, SQ_PROJ_CNT_DROPPED = 10, SQ_PROJ_CNT_KEPT = 11 };
// status of a line: 1 = an invalid structure row; 2 = the row does not fit the caller's buffers (more residues than Lmax,
// or, lifting, its short rows do not lie inside the short buffer or are narrower than the row's residues)
enum { SQ_PROJ_OK = 0, SQ_PROJ_INVALID = 1, SQ_PROJ_NO_ROOM = 2 };

struct SqProject {
    // ---- bytes
    SQ_PROJ_HD static uint8_t table_entry(int b) { return (uint8_t)SqCovar::cls((uint8_t)b); }
    static void fill_table(uint8_t tab[256])
    {
        for (int b = 0; b < 256; b++) tab[b] = table_entry(b);
    }
    SQ_PROJ_HD static bool is_residue(uint8_t cls) { return cls != SQ_COV_GAP; }

    // ---- the gap map
    SQ_PROJ_HD static int32_t words(int32_t L) { return (int32_t)(((int64_t)L + 63) / 64); }
    SQ_PROJ_HD static uint64_t below(int bit) { return ((uint64_t)1 << bit) - 1; }              // bit in 0..63
    SQ_PROJ_HD static bool residue_at(const uint64_t *word, int32_t c) { return word[c >> 6] >> (c & 63) & 1; }
    SQ_PROJ_HD static int32_t rank(const uint64_t *word, const int32_t *base, int32_t c)
    {
        return base[c >> 6] + __builtin_popcountll(word[c >> 6] & below(c & 63));
    }
    SQ_PROJ_HD static int32_t pos(const uint64_t *word, const int32_t *base, int32_t c) { return rank(word, base, c); }
    // the bit index of the k-th set bit of w (k from 0, k < popcount(w)): halving by popcounts
    SQ_PROJ_HD static int select64(uint64_t w, int k)
    {
        int at = 0;
        for (int s = 32; s; s >>= 1) {
            const int n = __builtin_popcountll(w & below(s));
            if (k >= n) {
                k -= n;
                w >>= s;
                at += s;
            }
        }
        return at;
    }
    // the chunk of residue i (0 <= i < base[nW]): the last j with base[j] <= i
    SQ_PROJ_HD static int32_t chunk_of(const int32_t *base, int32_t nW, int32_t i)
    {
        int32_t lo = 0, hi = nW;                                     // base[lo] <= i < base[hi]
        while (hi - lo > 1) {
            const int32_t mid = (lo + hi) >> 1;
            if (base[mid] <= i) lo = mid; else hi = mid;
        }
        return lo;
    }
    SQ_PROJ_HD static int32_t col(const uint64_t *word, const int32_t *base, int32_t nW, int32_t i)
    {
        const int32_t j = chunk_of(base, nW, i);
        return j * 64 + select64(word[j], i - base[j]);
    }
    // popcounts of the chunks (in base[0 .. nW - 1]) -> exclusive bases, base[nW] = the length; returns it
    static int32_t exclusive_bases(int32_t *base, int32_t nW)
    {
        int32_t run = 0;
        for (int32_t j = 0; j < nW; j++) {
            const int32_t n = base[j];
            base[j] = run;
            run += n;
        }
        base[nW] = run;
        return run;
    }

    // ---- one column of a structure row (Distances' rule): is the partner p of column c of a row of `width` columns (whose
    // partner's partner is `back`, read only when 0 <= p < width) a fault of the row?
    SQ_PROJ_HD static bool partner_in_range(int32_t p, int32_t width) { return p >= -1 && p < width; }
    SQ_PROJ_HD static bool column_bad(int32_t c, int32_t p, int32_t back, int32_t width)
    {
        return !partner_in_range(p, width) || p == c || (p >= 0 && back != c);
    }

    // ---- the class of the pair (v, w), v < w, from the class bytes at v and at w
    SQ_PROJ_HD static int pair_class(uint8_t a, uint8_t b)
    {
        const bool ga = !is_residue(a), gb = !is_residue(b);
        if (ga || gb) return ga && gb ? SQ_PROJ_BOTH_GAP : SQ_PROJ_ONE_GAP;
        if (a == SQ_COV_A && b == SQ_COV_U) return SQ_PROJ_AU;
        if (a == SQ_COV_U && b == SQ_COV_A) return SQ_PROJ_UA;
        if (a == SQ_COV_G && b == SQ_COV_C) return SQ_PROJ_GC;
        if (a == SQ_COV_C && b == SQ_COV_G) return SQ_PROJ_CG;
        if (a == SQ_COV_G && b == SQ_COV_U) return SQ_PROJ_GU;
        if (a == SQ_COV_U && b == SQ_COV_G) return SQ_PROJ_UG;
        return SQ_PROJ_NONCANONICAL;
    }
    // two residues, of a class the call admits
    SQ_PROJ_HD static bool admitted(int cls, bool canonical_only)
    {
        return cls >= SQ_PROJ_AU && (cls <= SQ_PROJ_UG || (cls == SQ_PROJ_NONCANONICAL && !canonical_only));
    }
    // `inner` = the residues strictly between the ends (read only for an admitted class: both ends are residues there)
    SQ_PROJ_HD static bool kept(int cls, bool canonical_only, int32_t min_loop, int32_t inner)
    {
        return admitted(cls, canonical_only) && inner >= min_loop;
    }
    SQ_PROJ_HD static bool dropped_by_loop(int cls, bool canonical_only, int32_t min_loop, int32_t inner)
    {
        return admitted(cls, canonical_only) && inner < min_loop;
    }
    // What column c with partner p >= 0 of a valid line gives in a row: the class of its pair, whether the pair is kept, and
    // the residues between its ends.  Both ends of a pair call this with the same ordered pair and decide alike.
    SQ_PROJ_HD static int judge(const uint8_t *cls, const uint64_t *word, const int32_t *base, int32_t c, int32_t p, bool canonical_only,
                                int32_t min_loop, bool &keep, bool &loop_drop)
    {
        const int32_t v = c < p ? c : p, w = c < p ? p : c;
        const int pc = pair_class(cls[v], cls[w]);
        const int32_t inner = admitted(pc, canonical_only) ? pos(word, base, w) - pos(word, base, v) - 1 : 0;
        keep = kept(pc, canonical_only, min_loop, inner);
        loop_drop = dropped_by_loop(pc, canonical_only, min_loop, inner);
        return pc;
    }
};
