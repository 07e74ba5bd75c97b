// sq_nussinov.h -- Nussinov DP + BackTrack (SQRNalgos.py:6-93): the layout of a job's scratch and the algorithm, fp64,
// first-best-k tie rule.  Part of sq_match.h (which defines the job records, SQ_HD and sq_take); include that.
//
// Host+device inline code, as sq_blossom.h: the product runs sq_nussinov_run in sq_nussinov_kernel, one block per job
// (SqCoopWave's atomics, block barriers); tests/native/nussinov_host.cpp runs it on one thread (SqCoopSingle, no barrier)
// against the oracle.
#pragma once
#include "sq_match.h"

struct SqNussLayout {
    // SCORES is sparse (the cells of the stems): per column j the list of (k, SCORES[(k, j)]) in ascending k,
    // so a cell of the DP only visits the k that can pair with j (:73-74) instead of all of i..j-2
    double *cs;                      // [m] scores
    int32_t *ck;                     // [m] row k
    int32_t *col_off, *cursor;       // [n + 1] the columns' starts, [n] fill cursors
    double *D;                       // [n][n] column-major: D[j * n + i] = D[i, j]
    int32_t *K;                      // [n][n] column-major: the k cell (i, j) pairs j with, -2: none
    uint8_t *has;                    // [n][n] BackTrack's "already queued" marks
    int32_t *cur, *nxt;              // [2 (n + 2)] each: BackTrack's two queues of (i, j) cells
    size_t lists_end, lists_room;    // bytes the column lists take, and have
    size_t end;
};

SQ_HD static inline SqNussLayout sq_nuss_carve(char *scratch, int n, int m)
{
    SqNussLayout L;
    const size_t N = (size_t)n, M = (size_t)m;
    size_t o = 0;
    // The first n * n doubles of the scratch (the S table of the reference, which the DP by columns does not keep) hold the
    // column lists.  They fit: the m cells of a job are distinct (v < w), m <= n (n - 1) / 2, so for n >= 2
    //   12 m + 4 (2 n + 1) <= 6 n^2 + 2 n + 4 <= 8 n^2
    // (n < 2 has no DP).  A caller that hands over repeated cells has to count them against this bound itself.
    sq_take(scratch, o, L.cs, M); sq_take(scratch, o, L.ck, M); sq_take(scratch, o, L.col_off, N + 1); sq_take(scratch, o, L.cursor, N);
    L.lists_end = o;
    o = L.lists_room = N * N * sizeof(double);
    sq_take(scratch, o, L.D, N * N);
    sq_take(scratch, o, L.K, N * N);
    sq_take(scratch, o, L.has, (N * N + 15) & ~(size_t)15);
    sq_take(scratch, o, L.cur, 2 * (N + 2)); sq_take(scratch, o, L.nxt, 2 * (N + 2));
    L.end = o;
    return L;
}

// global scratch of one job
static inline size_t sq_nussinov_scratch_bytes(int n) { return sq_nuss_carve(nullptr, n, 0).end + 64; }

// One job on nthr threads (every thread calls it with the same arguments and its own `tid`).  edges: the job's m cells
// (v, w, score), distinct; cd: the sequence's codes (separators: 26, 27); n >= 2.  The pairs (k, j) go to out[0 .. 2 * count).
template <class Sync, class Coop>
SQ_HD_INLINE void sq_nussinov_run(const SqNussLayout &L, int n, int m, const SqMatchEdge *edges, const uint8_t *cd, int32_t *out,
                                  int32_t *count, int tid, int nthr, Sync sync, Coop coop)
{
    double *const cs = L.cs;
    int32_t *const ck = L.ck, *const col_off = L.col_off, *const cursor = L.cursor;
    uint8_t *const has = L.has;
    // (the DP writes D and K of every cell above the main diagonal before anything reads them: only the diagonal of D and
    // BackTrack's marks start at zero -- zeroing all three tables was 21 bytes per cell of traffic per job)
    for (size_t q = tid; q < (size_t)n * n; q += nthr) has[q] = 0;
    for (int q = tid; q < n; q += nthr) L.D[(size_t)q * n + q] = 0.0;
    for (int q = tid; q <= n; q += nthr) col_off[q] = 0;
    sync();
    for (int e = tid; e < m; e += nthr) coop.add_i32(&col_off[edges[e].w + 1], 1);
    sync();
    if (tid == 0) for (int j = 0; j < n; j++) col_off[j + 1] += col_off[j];
    sync();
    for (int q = tid; q < n; q += nthr) cursor[q] = col_off[q];
    sync();
    for (int e = tid; e < m; e += nthr) {                               // SCORES[(v,w)] = -stem[2]  (:49)
        const SqMatchEdge ed = edges[e];
        const int pos = coop.fetch_add_i32(&cursor[ed.w], 1);
        ck[pos] = ed.v; cs[pos] = -ed.weight;
    }
    sync();
    for (int j = tid; j < n; j += nthr) {                               // ascending k inside every column (short lists)
        const int a = col_off[j], b = col_off[j + 1];
        for (int x = a + 1; x < b; x++) {
            const int kk = ck[x]; const double vv = cs[x];
            int y = x - 1;
            while (y >= a && ck[y] > kk) { ck[y + 1] = ck[y]; cs[y + 1] = cs[y]; y--; }
            ck[y + 1] = kk; cs[y + 1] = vv;
        }
    }
    sync();
    // The DP by COLUMNS (round 4; the reference and the kernel until then: by diagonals, :65-83).  Cell (i, j) reads
    // D[i, k-1] (k <= j - 2), D[k+1, j-1] and D[i, j-1]: columns before j only, so the columns can be taken one after the
    // other with all rows of a column at once -- the same values in any such order.  What the order buys: the list of
    // column j -- the k that can pair with j, :73-74 -- is the same for every row (uniform loads, fetched while the column
    // before is computed), D[k+1, j-1] is one value per list entry, and with D and K stored column-major the rows' reads of
    // D[., k-1] and D[., j-1] are consecutive doubles.  By diagonals every cell chased column list -> k -> two cells of D
    // through L2, three dependent trips per diagonal; now one per column.
    // Dc[j * n + i] = D[i, j], Kc[j * n + i] = K[i, j].
    double *const Dc = L.D;
    int32_t *const Kc = L.K;
    for (int j = 1; j < n; j++) {
        const int x0 = col_off[j], x1 = col_off[j + 1];
        const double *const dprevcol = Dc + (size_t)(j - 1) * n;
        for (int i = tid; i < j; i += nthr) {
            int bestk = -1; double best = 1e9;                          // :70
            // k in range(i, j - 1) with (k, j) in SCORES, ascending (first best k, :77); four list entries per trip
            for (int x = x0; x < x1; x += 4) {
                int kk[4]; double d1[4], d2[4], cw[4]; bool ok[4];
                // (the loads are unconditional -- an entry past the list reads the trip's first one again -- so that the four
                // are in flight together however the compiler treats the wave-uniform k)
                SQ_UNROLL
                for (int t = 0; t < 4; t++) { const int k = ck[x + t < x1 ? x + t : x]; kk[t] = x + t < x1 ? k : 0x7fffffff; }
                SQ_UNROLL
                for (int t = 0; t < 4; t++) {
                    ok[t] = kk[t] >= i && kk[t] < j - 1;
                    d1[t] = 0.0; d2[t] = 0.0; cw[t] = 0.0;
                    if (ok[t]) {
                        // D[i, k-1] with k == i is numpy's D[i, -1] = D[i, n-1], which no cell has written yet at this point: 0 (:76)
                        if (kk[t] > i) d1[t] = Dc[(size_t)(kk[t] - 1) * n + i];
                        d2[t] = dprevcol[kk[t] + 1];
                        cw[t] = cs[x + t];
                    }
                }
                SQ_UNROLL
                for (int t = 0; t < 4; t++)
                    if (ok[t]) {
                        const double sc = d1[t] + d2[t] + cw[t];
                        if (sc < best) { bestk = kk[t]; best = sc; }
                    }
                if (kk[3] >= j - 1) break;
            }
            const double dprev = dprevcol[i];                           // D[i, j-1] (i == j - 1: the diagonal, 0)
            const bool take = best <= dprev;                            // :80-83
            Kc[(size_t)j * n + i] = take ? bestk : -2;
            Dc[(size_t)j * n + i] = take ? best : dprev;
        }
        sync();
    }
    // BackTrack(0, N-1) (:6-41): level-synchronous set of cells; one thread, O(N) cells
    if (tid == 0) {
        const int minloop = 3;
        int32_t *const cur = L.cur, *const nxt = L.nxt;
        uint8_t *inq = has;            // zeroed above
        int qn = 1, np = 0;
        cur[0] = 0; cur[1] = n - 1;
        auto sep = [&](int p) { return cd[p] == 26 || cd[p] == 27; };
        auto anysep = [&](int a, int b) { for (int x = a; x < b; x++) if (x >= 0 && x < n && sep(x)) return true; return false; };
        while (qn) {
            int nn = 0;
            for (int t = 0; t < qn; t++) {
                const int i = cur[2 * t], j = cur[2 * t + 1];
                if (i < 0 || j < 0 || i >= n || j >= n) continue;
                auto push = [&](int a, int b) {
                    if (!inq[(size_t)a * n + b]) { inq[(size_t)a * n + b] = 1; nxt[2 * nn] = a; nxt[2 * nn + 1] = b; nn++; }
                };
                const int kk = Kc[(size_t)j * n + i];
                if (kk != -2) {
                    const int k = kk;
                    if (((k - 1) - i > minloop) || ((k - 1) - i > 0 && anysep(i + 1, k - 1))) push(i, k - 1);
                    if (((j - 1) - (k + 1) > minloop) || ((j - 1) - (k + 1) > 0 && anysep(k + 2, j - 1))) push(k + 1, j - 1);
                    out[2 * np] = k; out[2 * np + 1] = j; np++;
                } else {
                    if (((j - 1) - i > minloop) || ((j - 1) - i > 0 && anysep(i + 1, j - 1))) push(i, j - 1);
                }
            }
            for (int t = 0; t < nn; t++) inq[(size_t)nxt[2 * t] * n + nxt[2 * t + 1]] = 0;
            for (int t = 0; t < 2 * nn; t++) cur[t] = nxt[t];
            qn = nn;
        }
        *count = np;
    }
}
