// What a substitution does to a structure (sq_variant_diff, FoldMutants): one entry of a variant's row against its wild type's.
//
// Variant m is record rec0 + m of the pair tables, its wild type is record wt_rec[m]; both are read at row 0, the consensus
// row, and both have the same length n: a substitution changes no column.  Position t has the wild-type partner p = w[t] and
// the variant's partner q = v[t] (-1: unpaired).  The pairs are counted at their 5' ends:
//   lost     p > t and q != p      a wild-type pair the variant lacks
//   kept     p > t and q == p      a pair of both
//   gained   q > t and q != p      a variant's pair the wild type lacks
//   changed  p != q                the position's partner differs
// so lost / gained / kept are the sizes of the set differences and of the intersection of the two rows' sets of pairs -- as
// long as both rows are symmetric, which valid_entry() checks for every entry that is read.
//
// This header compiles for the device and for the host (tests/native/variants_host.cpp runs it as one thread).  Every read
// is bounded by the records' common length and that by both tables (length()), whatever the caller's arrays hold.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SQ_V_HD __host__ __device__
#else
#define SQ_V_HD
#endif

enum { SQ_V_LOST = 1, SQ_V_KEPT = 2, SQ_V_GAINED = 4, SQ_V_CHANGED = 8, SQ_V_INVALID = 16 };   // the flags of an entry

// Most blocks of a launch (4 variants each at a time): squarna_amd/device_calls.py holds the same number for the tests.
#define SQ_VARIANT_MAX_BLOCKS 2048

struct SqVariants {
    const int32_t *partner;               // pair tables in sq_result_pairs_dev's layout
    const int64_t *cell_off;              // [rec0 + nvar + 1]
    const int64_t *lengths;               // [rec0 + nvar]
    const int32_t *wt_rec;                // [nvar]: the wild type's record, in [0, rec0)
    const int64_t *pos_off;               // [rec0 at least]: where a wild type's positions start on the axis of Ltot positions
    int32_t rec0, nvar;
    int64_t Ltot;

    SQ_V_HD const int32_t *row(int64_t r) const { return partner + cell_off[r]; }

    // The common length of variant m and its wild type, or -1: the wild type is no record before rec0, the lengths differ, a
    // row is longer than its table, or the wild type's positions do not lie inside the axis.  (n <= Ltot < 2^31 then.)
    SQ_V_HD int32_t length(int32_t m) const
    {
        const int64_t r = (int64_t)rec0 + m, wt = wt_rec[m];
        if (wt < 0 || wt >= rec0) return -1;
        const int64_t n = lengths[r];
        if (n < 0 || lengths[wt] != n || n > cell_off[r + 1] - cell_off[r] || n > cell_off[wt + 1] - cell_off[wt]) return -1;
        if (pos_off[wt] < 0 || pos_off[wt] + n > Ltot) return -1;
        return (int32_t)n;
    }

    // an entry inside [-1, n) that is not the position itself and points back
    SQ_V_HD static bool valid_entry(const int32_t *r, int32_t n, int32_t t)
    {
        const int32_t p = r[t];
        return p == -1 || (p >= 0 && p < n && p != t && r[p] == t);
    }

    // The flags of position t < n of the rows w (wild type) and v (variant) of n entries each.
    SQ_V_HD static int entry(const int32_t *w, const int32_t *v, int32_t n, int32_t t)
    {
        if (!valid_entry(w, n, t) || !valid_entry(v, n, t)) return SQ_V_INVALID;
        const int32_t p = w[t], q = v[t];
        return (p > t && q != p ? SQ_V_LOST : 0) | (p > t && q == p ? SQ_V_KEPT : 0) | (q > t && q != p ? SQ_V_GAINED : 0) |
               (p != q ? SQ_V_CHANGED : 0);
    }
};
