// sq_state.h -- the pieces of a structure's state that every kernel builds the same way: the strands painted into the partner
// array and the mask codes, the free-position words of the bit-diagonal scan, the skip pointers of ScoreStems' sweep.
//
// Device code for a block of nthr threads = nwv waves (tid = 64 wv + lane); a kernel whose block is one wave passes
// (lane, 64) and (lane, 0, 1).  Callers: sq_state_build and sq_score_body (sq_kernels.hip), sq_pool_round_body and
// sq_pool_root_kernel (sq_pool_round.hip), sq_rounds_kernel (sq_rounds.hip).  The barriers around the calls are the callers';
// so are the prefix counts, whose multi-wave form needs LDS totals the one-wave form does not.
#pragma once
#include <hip/hip_runtime.h>
#include "sq_device.h"

// the positions of the strands: partner in P (:634-635), mask code 255 in E (:446-451: row and column of a paired base)
__device__ __forceinline__ void sq_state_paint(int16_t *P, uint8_t *E, const SqStrand *strands, int nstrand, int tid, int nthr)
{
    for (int k = tid; k < nstrand; k += nthr) {
        const SqStrand x = strands[k];
        for (int t = 0; t < x.len; t++) {
            const int pos = x.start + t;
            P[pos] = (int16_t)(x.pstart - t);
            E[pos] = 255;
        }
    }
}

// Free-position words for the bit-diagonal scan, fbh words each: F bit p = (E[p] == 0); G bit k + SQ_GPAD = F bit n - 1 - k.
// G lies behind F in every caller (G = F + fbh); as a pointer of its own it cost sq_rounds_kernel six spilled SGPRs.
// One ballot = two words: a wave takes the pairs of words (2 m2, 2 m2 + 1) of either array, m2 = wv, wv + nwv, ...
__device__ __forceinline__ void sq_free_words(const uint8_t *E, int n, int fbh, uint32_t *F, int lane, int wv, int nwv)
{
    for (int m2 = wv; 2 * m2 < fbh; m2 += nwv) {
        const int pf = 64 * m2 + lane;                       // forward array: position
        const unsigned long long bf = __ballot(pf < n && E[pf] == 0);
        const int pr = n - 1 - (64 * m2 + lane - SQ_GPAD);   // reversed array: bit 64 m2 + lane <-> position n - 1 - (bit - pad)
        const unsigned long long br = __ballot(pr >= 0 && pr < n && E[pr] == 0);
        if (lane == 0) {
            F[2 * m2] = (uint32_t)bf; F[fbh + 2 * m2] = (uint32_t)br;
            if (2 * m2 + 1 < fbh) { F[2 * m2 + 1] = (uint32_t)(bf >> 32); F[fbh + 2 * m2 + 1] = (uint32_t)(br >> 32); }
        }
    }
}

// Once the sweep of ScoreStems has registered the block [start, partner] of a 5' strand, the strands that start inside it
// are inert unless they are 5' strands whose partner lies beyond the block's end (they extend it or are wings); skip[k] =
// the first strand behind k that starts outside the block or is such a strand.
__device__ __forceinline__ void sq_skip_pointers(const SqStrand *strands, int nstrand, uint16_t *skip, int tid, int nthr)
{
    for (int k = tid; k < nstrand; k += nthr) {
        const SqStrand x = strands[k];
        int q = k + 1;
        if (x.left) {
            const int pf = x.pstart;
            while (q < nstrand) {
                const SqStrand y = strands[q];
                if (y.start > pf || (y.left && y.pstart > pf)) break;
                q++;
            }
        }
        skip[k] = (uint16_t)q;
    }
}
