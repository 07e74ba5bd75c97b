// Greedy conflict-free selection from a ranked candidate list, in rounds (sq_first_fit_dev; the host form is
// sq_align_first_fit, sq_parse.cpp -- MatrixToDBNs' first structure SQRNdbnali.py:121-192 and Consensus :271-304).
//
// The sequential pass goes down the ranked list and takes a pair iff both of its columns are still free.  The same set comes
// out of rounds in which the order of the work inside a round does not matter:
//   post    every live candidate posts its rank to both of its columns with a minimum;
//   take    a candidate whose rank is the minimum at BOTH columns is taken (the sequential pass takes it too: every
//           candidate ranked before it that touches one of its columns is dead already);
//   retire  a candidate that touches a taken column dies; the others reset their columns and stay live.
// Every round takes at least the best live candidate and a matching over L columns holds at most L / 2 pairs (v < w), so
// there are at most L / 2 + 1 rounds; the loop is bounded by that number and ends with status 1 beyond it, never spins.
//
// This header compiles for the device and for the host: the logic is written against a work-sharing policy X (which thread am
// I, how many are we, barrier, the accesses to the shared words).  The device policy is one workgroup (sq_align_dev.hip): no
// word is ever handed from one workgroup to another, a barrier is the workgroup's own.  SqFitSerial runs the same code as
// one thread (tests/native/firstfit_host.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SQ_FF_HD __host__ __device__
#else
#define SQ_FF_HD
#endif

#define SQ_FF_FREE 0x7fffffff            // no live candidate has posted to the column
enum { SQ_FF_STATUS = 0, SQ_FF_ROUNDS = 1, SQ_FF_PAIRS = 2, SQ_FF_LIVE = 3 };   // info[4] of sq_first_fit_dev

struct SqFitSerial {                      // the host's policy: one thread, the barrier is the program order
    int tid() const { return 0; }
    int nthreads() const { return 1; }
    void barrier() const {}
    int32_t load(const int32_t *p) const { return *p; }
    void store(int32_t *p, int32_t v) const { *p = v; }
    void min_at(int32_t *p, int32_t v) const { if (v < *p) *p = v; }
    int32_t add_at(int32_t *p, int32_t v) const { const int32_t old = *p; *p += v; return old; }
};

struct SqFirstFit {
    const int64_t *flat;                  // [n] candidates v * L + w in rank order (read only)
    int64_t n;
    int32_t L, minspan;
    int32_t *partner;                     // [L] out: the column's partner, -1 where free
    int32_t *colmin;                      // [L] scratch
    int32_t *list[2];                     // [n] each: the ranks of the live candidates, this round's and the next's
    int32_t *ctl;                         // [8] scratch: the two lists' lengths, then info[4]

    SQ_FF_HD static size_t scratch_ints(int64_t n, int32_t L) { return (size_t)L + 2 * (size_t)n + 8; }

    SQ_FF_HD void bind(int32_t *scratch)
    {
        ctl = scratch; colmin = scratch + 8; list[0] = colmin + L; list[1] = list[0] + n;
    }

    // a candidate's columns; false: not a candidate (outside the matrix, v >= w, span below minspan: MatrixToDBNs :147)
    SQ_FF_HD bool columns(int32_t k, int32_t &v, int32_t &w) const
    {
        const int64_t f = flat[k];
        if (f < 0 || f >= (int64_t)L * L) return false;
        v = (int32_t)(f / L); w = (int32_t)(f - (int64_t)v * L);
        return w > v && w - v >= minspan;
    }

    template <class X> SQ_FF_HD void run(X &x) const
    {
        const int tid = x.tid(), nt = x.nthreads();
        for (int32_t c = tid; c < L; c += nt) { x.store(&partner[c], -1); x.store(&colmin[c], SQ_FF_FREE); }
        if (tid == 0) for (int q = 0; q < 8; q++) x.store(&ctl[q], 0);
        x.barrier();
        for (int64_t k = tid; k < n; k += nt) {
            int32_t v, w;
            if (columns((int32_t)k, v, w)) x.store(&list[0][x.add_at(&ctl[0], 1)], (int32_t)k);
        }
        const int32_t max_rounds = L / 2 + 1;
        int32_t rounds = 0, status = 0, live = 0;
        for (int cur = 0;; cur ^= 1) {
            x.barrier();
            live = x.load(&ctl[cur]);                                  // (the same for every thread: written before the barrier)
            if (live == 0) break;
            if (rounds == max_rounds) { status = 1; break; }
            rounds++;
            const int32_t *mine = list[cur];
            int32_t *next = list[cur ^ 1];
            if (tid == 0) x.store(&ctl[cur ^ 1], 0);
            for (int32_t q = tid; q < live; q += nt) {                  // post
                int32_t v, w;
                const int32_t k = x.load(&mine[q]);
                columns(k, v, w);
                x.min_at(&colmin[v], k); x.min_at(&colmin[w], k);
            }
            x.barrier();
            for (int32_t q = tid; q < live; q += nt) {                  // take
                int32_t v, w;
                const int32_t k = x.load(&mine[q]);
                columns(k, v, w);
                if (x.load(&colmin[v]) == k && x.load(&colmin[w]) == k) {
                    x.store(&partner[v], w); x.store(&partner[w], v);
                    x.add_at(&ctl[4 + SQ_FF_PAIRS], 1);
                }
            }
            x.barrier();
            for (int32_t q = tid; q < live; q += nt) {                  // retire
                int32_t v, w;
                const int32_t k = x.load(&mine[q]);
                columns(k, v, w);
                if (x.load(&partner[v]) >= 0 || x.load(&partner[w]) >= 0) continue;
                x.store(&colmin[v], SQ_FF_FREE); x.store(&colmin[w], SQ_FF_FREE);
                x.store(&next[x.add_at(&ctl[cur ^ 1], 1)], k);
            }
        }
        if (tid == 0) {
            x.store(&ctl[4 + SQ_FF_STATUS], status); x.store(&ctl[4 + SQ_FF_ROUNDS], rounds); x.store(&ctl[4 + SQ_FF_LIVE], live);
        }
    }
};
