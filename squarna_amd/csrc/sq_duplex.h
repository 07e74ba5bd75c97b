// What two chains do to one another when they fold together (sq_duplex_summary, FoldDuplex): one entry of a duplex's row
// against the rows of its two chains folded alone.
//
// Two sets of pair tables in sq_result_pairs_dev's layout, which may be one allocation: the solo records (partner_s /
// cell_off_s / lengths_s, nsolo of them) and the duplex records (partner_d / cell_off_d / lengths_d, ndup of them).  Duplex k
// is the chain of solo record a_rec[k] (nA positions), a separator column and the chain of solo record b_rec[k] (nB
// positions): n = nA + 1 + nB entries, entry nA the separator; a_rec[k] == b_rec[k] is a homodimer.  All three rows are read
// at row 0, the consensus row: A = the row of solo a, B = the row of solo b, D = the duplex's.  Duplex position t < nA is A's
// position t, t > nA is B's position u = t - nA - 1, and a partner p of B's row corresponds to p + nA + 1 in the duplex.
// With q = D[t] the flags of a position are, pairs counted at their 5' ends:
//   inter_a   t < nA and q > nA              A's position pairs across the separator (one flag per inter-chain pair)
//   inter_b   t > nA and 0 <= q < nA         B's position pairs across the separator
//   intra_a   t < nA and t < q < nA          a duplex pair inside chain A
//   intra_b   t > nA and q > t               a duplex pair inside chain B
//   lost_a    t < nA, A[t] > t, q != A[t]                a pair of A alone whose 5' end has another partner, or none
//   lost_b    t > nA, B[u] > u, q != B[u] + nA + 1       the same for B
// which are set sizes as long as all three rows are symmetric: SqVariants::valid_entry() checks every entry that is read.
//
// This header compiles for the device and for the host (tests/native/duplex_host.cpp runs it as one thread).  Every read is
// bounded by the three rows' lengths and those by their tables (shape()), whatever the caller's arrays hold.
#pragma once
#include <stdint.h>
#include "sq_variants.h"

enum { SQ_D_INTER_A = 1, SQ_D_INTER_B = 2, SQ_D_INTRA_A = 4, SQ_D_INTRA_B = 8, SQ_D_LOST_A = 16, SQ_D_LOST_B = 32,
       SQ_D_INVALID = 64 };                                                                      // the flags of an entry

// Most blocks of a launch (4 duplexes each at a time): squarna_amd/device_calls.py holds the same number for the tests.
#define SQ_DUPLEX_MAX_BLOCKS 2048

struct SqDuplexShape {
    int64_t a, b;                         // the solo records of the two chains
    int32_t nA, nB;                       // their lengths: the duplex row has nA + 1 + nB entries
};

struct SqDuplex {
    const int32_t *partner_s;             // the solo records' pair tables
    const int64_t *cell_off_s;            // [nsolo + 1]
    const int64_t *lengths_s;             // [nsolo]
    const int32_t *partner_d;             // the duplex records' pair tables
    const int64_t *cell_off_d;            // [ndup + 1]
    const int64_t *lengths_d;             // [ndup]
    const int32_t *a_rec, *b_rec;         // [ndup]: the chains' solo records, in [0, nsolo)
    const int64_t *pos_off;               // [nsolo + 1]: where a solo record's positions start on the axis of Ltot positions
    int32_t nsolo, ndup;
    int64_t Ltot;

    SQ_V_HD const int32_t *solo_row(int64_t r) const { return partner_s + cell_off_s[r]; }
    SQ_V_HD const int32_t *duplex_row(int64_t k) const { return partner_d + cell_off_d[k]; }

    // A solo record's length, or -1: the row is longer than its table or its positions do not lie inside the axis.
    SQ_V_HD int64_t solo_length(int64_t r) const
    {
        const int64_t n = lengths_s[r];
        if (n < 0 || n > cell_off_s[r + 1] - cell_off_s[r] || pos_off[r] < 0 || pos_off[r] + n > Ltot) return -1;
        return n;
    }

    // The chains of duplex k and their lengths; false: a chain is no solo record, the duplex row is not nA + 1 + nB entries
    // long or longer than its table, a solo row is longer than its table or outside the axis, or the separator column is
    // paired.  (nA, nB <= Ltot < 2^31 then, and a duplex row of 2^31 entries or more is refused: its partners are int32.)
    SQ_V_HD bool shape(int32_t k, SqDuplexShape &h) const
    {
        h.a = a_rec[k]; h.b = b_rec[k];
        if (h.a < 0 || h.a >= nsolo || h.b < 0 || h.b >= nsolo) return false;
        const int64_t nA = solo_length(h.a), nB = solo_length(h.b), n = nA + 1 + nB;
        if (nA < 0 || nB < 0 || lengths_d[k] != n || n > 0x7fffffffll || n > cell_off_d[k + 1] - cell_off_d[k]) return false;
        h.nA = (int32_t)nA; h.nB = (int32_t)nB;
        return duplex_row(k)[nA] == -1;
    }

    // The flags of position t < nA + 1 + nB of the duplex row D over the solo rows A (nA entries) and B (nB entries).
    SQ_V_HD static int entry(const int32_t *A, const int32_t *B, const int32_t *D, int32_t nA, int32_t nB, int32_t t)
    {
        if (!SqVariants::valid_entry(D, nA + 1 + nB, t)) return SQ_D_INVALID;
        const int32_t q = D[t];
        if (t < nA) {
            if (!SqVariants::valid_entry(A, nA, t)) return SQ_D_INVALID;
            const int32_t p = A[t];
            return (q > nA ? SQ_D_INTER_A : 0) | (q > t && q < nA ? SQ_D_INTRA_A : 0) | (p > t && q != p ? SQ_D_LOST_A : 0);
        }
        if (t == nA) return 0;                                   // (the separator: shape() has seen that it is unpaired)
        const int32_t u = t - nA - 1;
        if (!SqVariants::valid_entry(B, nB, u)) return SQ_D_INVALID;
        const int32_t p = B[u];
        return (q >= 0 && q < nA ? SQ_D_INTER_B : 0) | (q > t ? SQ_D_INTRA_B : 0) | (p > u && q != p + nA + 1 ? SQ_D_LOST_B : 0);
    }
};
