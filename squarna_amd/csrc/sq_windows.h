// Pair counts over the overlapping windows of long sequences (sq_window_pair_count, FoldWindows): "the first holder emits".
//
// Window k covers the positions [start[k], start[k] + len[k]) of one axis on which all records lie behind one another; its
// structure is a partner row in the window's own coordinates.  For every distinct pair (gi, gj), gi < gj, of the axis:
// count = the windows whose row pairs gi and gj, cover = the windows that contain both positions, first = the smallest
// index of a window that holds the pair.
//
// Starts and ends of the windows are both non-decreasing in k, and a window of another record never contains a pair, so the
// windows that contain (gi, gj) are one contiguous run of k.  The entry (k, t) with partner p > t looks at that run only:
//   down   from k - 1 while the window still ends behind gj: if one of them holds the same pair, this entry is not the first
//          holder and gives nothing;
//   up     from k + 1 while the window starts at or before gi: holders are counted.
// The first holder then knows count, first = k and cover = the run's length, and every distinct pair is given exactly once:
// no table of positions, no atomics on data, a result that does not depend on the order of the work.
//
// This header compiles for the device and for the host (tests/native/windows_host.cpp runs it as one thread).  Every read
// is bounded by the window's own length and that by its table (valid()), whatever the caller's arrays hold.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SQ_W_HD __host__ __device__
#else
#define SQ_W_HD
#endif

enum { SQ_W_NONE = 0, SQ_W_EMIT = 1, SQ_W_INVALID = 2 };   // what an entry gives

struct SqWindows {
    const int32_t *partner;               // pair tables in sq_result_pairs_dev's layout
    const int64_t *cell_off;              // [rec0 + nwin + 1]: window k is record rec0 + k, row 0 of it is read
    const int64_t *start;                 // [nwin] on the concatenated axis, non-decreasing
    const int32_t *len;                   // [nwin]
    int32_t rec0, nwin;
    int64_t Ltot;

    SQ_W_HD const int32_t *row(int32_t k) const { return partner + cell_off[rec0 + k]; }

    // a window inside the axis and inside its table
    SQ_W_HD bool valid(int32_t k) const
    {
        const int64_t s = start[k], n = len[k];
        return s >= 0 && n >= 0 && s + n <= Ltot && n <= cell_off[rec0 + k + 1] - cell_off[rec0 + k];
    }

    // whether window q pairs the axis positions gi < gj, both inside it (a valid entry of a valid window: row[a] = b, row[b] = a)
    SQ_W_HD bool holds(int32_t q, int64_t gi, int64_t gj) const
    {
        if (!valid(q)) return false;
        const int32_t *r = row(q);
        const int64_t a = gi - start[q], b = gj - start[q];
        return r[a] == b && r[b] == a;
    }

    // whether window q contains both positions
    SQ_W_HD bool contains(int32_t q, int64_t gi, int64_t gj) const { return start[q] <= gi && gj < start[q] + len[q]; }

    // Entry t < len[k] of window k.  SQ_W_EMIT: this entry is the pair's first holder, flat = gi * Ltot + gj.
    // SQ_W_INVALID: the window reaches outside the axis or its table, the partner lies outside [-1, len), is the position
    // itself or does not point back; such an entry is not counted, here or as another window's holder.
    SQ_W_HD int entry(int32_t k, int32_t t, int64_t &flat, int32_t &count, int32_t &cover, int32_t &first) const
    {
        if (!valid(k)) return SQ_W_INVALID;
        const int32_t *r = row(k);
        const int32_t p = r[t], n = len[k];
        if (p == -1) return SQ_W_NONE;
        if (p < -1 || p >= n || p == t || r[p] != t) return SQ_W_INVALID;
        if (p < t) return SQ_W_NONE;
        const int64_t gi = start[k] + t, gj = start[k] + p;
        int32_t lo = k, hi = k, c = 1;
        for (int32_t q = k - 1; q >= 0 && contains(q, gi, gj); q--) {
            if (holds(q, gi, gj)) return SQ_W_NONE;
            lo = q;
        }
        for (int32_t q = k + 1; q < nwin && contains(q, gi, gj); q++) {
            c += holds(q, gi, gj) ? 1 : 0;
            hi = q;
        }
        flat = gi * Ltot + gj; count = c; cover = hi - lo + 1; first = k;
        return SQ_W_EMIT;
    }
};
