// sq_choose.h -- ChooseStems for a-5 (SQRNdbnseq.py:754-789), the one statement of it in the product.
//
// The reference sorts a structure's scored stems by finalscore, descending and stable -- so among equals the order they
// were emitted in, which is the order of their keys ((i + j) << 16 | i) --, takes the first, and then every stem whose
// finalscore is not below subopt x the best one and that shares a base with EVERY stem taken so far (:779-789).  A pool
// that is full only uses the first element (:1147, the stopper).
//
//   sq_shares_base     :783-786 on two stems (i, j, len): one of the four pairs of strands overlaps
//   sq_choose_before   the order: finalscore descending, emission key ascending
//   sq_choose_first    the stopper's pick: among the survivors at the best finalscore the one with the smallest key
//   sq_choose_stems    the full choice: survivors within range into the caller's arrays, their ranks by counting, the
//                      conflict filter in rank order; every stem taken is handed to the caller
//
// Host+device inline code, as sq_lsap.h: the kernels run it with one wave (nl = 64, SqCoopWave, the block's barrier) on
// their own LDS arrays -- sq_pool_choose_kernel over a structure's SqOk records, sq_pool_round_body over its survivors in
// LDS (its stopper's pick is sq_choose_first's loop written out: sq_pool_round.hip says why) --; tests/native/choose_host.cpp
// runs it on one lane (nl = 1, SqCoopSingle, no barrier) against the oracle's _choose_stems.  The host loop
// (sq_round_host.hip) keeps std::sort, by sq_choose_before, and filters with sq_shares_base; sq_chain_kernel takes the pick,
// sq_rounds_kernel the order and the base-sharing test.
//
// A survivor source has  uint32_t size(),  double fin(q),  uint32_t key(q)  and  void get(q, key, len, bps).
#pragma once
#include <stdint.h>
#include "sq_blossom.h"            // SQ_HD, SQ_HD_INLINE, SqCoopSingle / SqCoopWave

#define SQ_POOL_CMAX 64            // stems ChooseStems may return for one structure (the result arrays ri / rj / rl hold as many)

#define SQ_CHOOSE_NONE 0xFFFFFFFFu // sq_choose_first: no survivor has the best finalscore
enum {
    SQ_CHOOSE_OVF_RANGE = -1,      // more survivors within range than the caller's arrays hold
    SQ_CHOOSE_OVF_PICKS = -2       // a stem would join a result that already holds min(SQ_POOL_CMAX, cmax) stems
};
struct SqChoice {
    int taken;                     // stems taken, or SQ_CHOOSE_OVF_*
    int in_range;                  // survivors within range
};

SQ_HD_INLINE bool sq_shares_base(int ai, int aj, int al, int bi, int bj, int bl)   // :783-786
{
    const int as0 = ai, as1 = ai + al - 1, at0 = aj - al + 1, at1 = aj;
    const int bs0 = bi, bs1 = bi + bl - 1, bt0 = bj - bl + 1, bt1 = bj;
    return (as0 <= bs1 && bs0 <= as1) || (as0 <= bt1 && bt0 <= as1) || (at0 <= bs1 && bs0 <= at1) || (at0 <= bt1 && bt0 <= at1);
}

// does (fy, ky) rank before (fx, kx)?  The reference's stable descending sort (:758) on stems emitted in key order
SQ_HD_INLINE bool sq_choose_before(double fx, uint32_t kx, double fy, uint32_t ky)
{
    return fy > fx || (fy == fx && ky < kx);
}

// the survivor source over an array of records with members key, len, bps, fin (SqOk: the launched kernels' survivors)
template <class Rec>
struct SqChooseRecs {
    const Rec *recs; uint32_t n;
    SQ_HD uint32_t size() const { return n; }
    SQ_HD double fin(uint32_t q) const { return recs[q].fin; }
    SQ_HD uint32_t key(uint32_t q) const { return recs[q].key; }
    SQ_HD void get(uint32_t q, uint32_t &k, int &len, double &bps) const { const Rec r = recs[q]; k = r.key; len = (int)r.len; bps = r.bps; }
};

// ChooseStems' first element, all a full pool uses (:1147): the survivor's index, or SQ_CHOOSE_NONE
template <class Src, class Coop>
SQ_HD_INLINE uint32_t sq_choose_first(const Src &src, double best, int lane, int nl, Coop coop)
{
    const uint32_t ns = src.size();
    unsigned long long pick = ~0ull;
    for (uint32_t q = (uint32_t)lane; q < ns; q += (uint32_t)nl)
        if (src.fin(q) == best) { const unsigned long long v = ((unsigned long long)src.key(q) << 32) | q; pick = v < pick ? v : pick; }
    return (uint32_t)coop.min_u64(pick);                   // (none: the lower half of ~0 is SQ_CHOOSE_NONE)
}

// The full choice.  fin / key / idx / ord: `cap` entries each, ri / rj / rl: SQ_POOL_CMAX, all the caller's (LDS in the
// kernels); Idx is the caller's index type, wide enough for src.size().  take(k, key, len, bps, fin) is called by lane 0 for
// the k-th stem taken, in ChooseStems' order.  (-inf finalscores -- rejected or pruned stems -- never pass the range.  The
// first in rank order always joins: a non-empty range gives a non-empty result.)
template <class Idx, class Src, class Sync, class Coop, class Take>
SQ_HD_INLINE SqChoice sq_choose_stems(const Src &src, double range, int cap, int cmax, double *fin, uint32_t *key, Idx *idx, uint16_t *ord,
                                      int *ri, int *rj, int *rl, int lane, int nl, Sync sync, Coop coop, Take take)
{
    // ---- the survivors within range (:769-778) ----
    const uint32_t ns = src.size();
    int n = 0;
    for (uint32_t q0 = 0; q0 < ns; q0 += (uint32_t)nl) {
        const uint32_t q = q0 + (uint32_t)lane;
        double f = 0.0;
        bool keep = false;
        if (q < ns) { f = src.fin(q); keep = !(f < range); }
        int total;
        const int pos = n + coop.rank_true(keep, lane, total);
        if (keep && pos < cap) { idx[pos] = (Idx)q; fin[pos] = f; key[pos] = src.key(q); }
        n += total;
    }
    if (n > cap) return SqChoice{SQ_CHOOSE_OVF_RANGE, n};
    sync();
    // ---- the reference's stable descending sort: a survivor's rank is the number of those before it ----
    for (int x = lane; x < n; x += nl) {
        const double fx = fin[x]; const uint32_t kx = key[x];
        int r = 0;
        for (int y = 0; y < n; y++) r += sq_choose_before(fx, kx, fin[y], key[y]) ? 1 : 0;
        ord[r] = (uint16_t)x;
    }
    sync();
    // ---- the conflict filter (:779-789): a survivor joins when it shares a base with every stem taken so far ----
    int nres = 0;
    for (int t = 0; t < n; t++) {
        const int x = ord[t];
        uint32_t ck; int cl; double bps;
        src.get((uint32_t)idx[x], ck, cl, bps);
        const int ci = (int)(ck & 0xFFFFu), cj = (int)(ck >> 16) - ci;
        // (lane l tests the taken stems l, l + nl, ...: for a wave at most one, and without the loop -- it cost
        // sq_pool_round_root_kernel, which runs at its register limit, a spilled SGPR)
        bool mine = true;
        if (nl >= SQ_POOL_CMAX) { if (lane < nres) mine = sq_shares_base(ci, cj, cl, ri[lane], rj[lane], rl[lane]); }
        else for (int r = lane; r < nres; r += nl) mine = mine && sq_shares_base(ci, cj, cl, ri[r], rj[r], rl[r]);
        if (coop.any(!mine)) continue;
        if (nres == SQ_POOL_CMAX || nres == cmax) return SqChoice{SQ_CHOOSE_OVF_PICKS, n};
        if (lane == 0) {
            ri[nres] = ci; rj[nres] = cj; rl[nres] = cl;
            take(nres, ck, cl, bps, fin[x]);
        }
        nres++;
        sync();
    }
    return SqChoice{nres, n};
}
