// sq_lsap.h -- Hungarian for a-8 (SQRNalgos.py:113-135): the layout of a job's state, the storage form it takes, and the
// algorithm.  Part of sq_match.h (which defines the job records, SQ_HD and sq_take); include that.
//
// The reference calls scipy.optimize.linear_sum_assignment (scipy 1.15.3, un-vendored C++: Crouse 2016 shortest augmenting
// path).  Restated step by step -- same column order, same tie-break towards unassigned columns -- so the assignment is the
// one scipy returns, not just an optimal one.
//
// Host+device inline code, as sq_blossom.h: the product runs sq_lsap_run in sq_lsap_kernel, one wave per job (W = 64,
// SqCoopWave, block barriers); tests/native/lsap_host.cpp runs it on one lane (W = 1, SqCoopSingle, SqLsapSyncNone) against
// scipy, in all three storage forms.
#pragma once
#include "sq_match.h"

// Where a job keeps its state.  The cost matrix is zero except for the 2m stem cells: when it fits, LDS holds it in sparse
// form -- a step of the shortest-path scan never leaves the CU, and a zero cell costs one mask word.
enum SqLsapForm {
    SQ_LSAP_A,            // sparse cost matrix and the row / column vectors in LDS
    SQ_LSAP_B,            // dense cost matrix in global scratch, vectors in LDS
    SQ_LSAP_C             // everything in global scratch
};

struct SqLsapLayout {
    double *cost;                                       // [n][n] dense matrix: global scratch (forms b, c)
    // the row / column vectors, touched in every step of the augmenting path (42 bytes per position): LDS, or behind cost
    double *u, *v, *spc;                                // [n] duals, shortest path costs
    int32_t *path, *col4row, *row4col, *remaining;      // [n]
    uint8_t *SR, *SC;                                   // [n]
    // the sparse matrix (form a), in LDS behind the vectors: per row a bit mask of its non-zero columns with per-word prefix
    // counts, the edge ids of a row's cells in column order (16 bits each) and the m edge weights.  150 nt / 1,320 edges:
    // 27 KB (the dense form -- 16-bit ids for all n^2 cells -- took 62 KB, and LDS a job holds for its milliseconds is LDS
    // the other kernels on the chip do not get)
    double *wts;                                        // [m]
    uint32_t *mask;                                     // [n][nw] non-zero columns of a row
    uint16_t *rowstart;                                 // [n + 1] into cids
    uint16_t *pre;                                      // [n][nw] cells of the row in earlier words
    uint16_t *cids;                                     // [2m] edge ids, row by row in column order
    int nw;                                             // mask words of a row
    size_t sparse_off;                                  // where in LDS the sparse matrix starts: behind the vectors of forms a, b
    size_t lds_end, scratch_end;                        // bytes carved from the two bases
};

// THE layout: every size below is read from it, the kernel and the host harness address a job through it.
// scratch: cost, then (form c) the vectors.  lds: (forms a, b) the vectors, then on a 16-byte boundary the sparse matrix.
SQ_HD static inline SqLsapLayout sq_lsap_carve(char *scratch, char *lds, SqLsapForm form, int n, int m)
{
    SqLsapLayout L;
    const size_t N = (size_t)n, M = (size_t)m;
    L.nw = (n + 31) >> 5;
    size_t os = 0, ol = 0;
    sq_take(scratch, os, L.cost, N * N);
    const bool glob = form == SQ_LSAP_C;
    char *const vb = glob ? scratch + os : lds;
    size_t ov = 0;
    sq_take(vb, ov, L.u, N); sq_take(vb, ov, L.v, N); sq_take(vb, ov, L.spc, N);
    sq_take(vb, ov, L.path, N); sq_take(vb, ov, L.col4row, N); sq_take(vb, ov, L.row4col, N); sq_take(vb, ov, L.remaining, N);
    sq_take(vb, ov, L.SR, N); sq_take(vb, ov, L.SC, N);
    if (glob) os += ov;
    ol = ov;
    sq_take(lds, ol, L.wts, M, 16);
    L.sparse_off = (size_t)(reinterpret_cast<char *>(L.wts) - lds);
    sq_take(lds, ol, L.mask, N * L.nw);
    sq_take(lds, ol, L.rowstart, N + 1);
    sq_take(lds, ol, L.pre, N * L.nw, 4);               // (pre and cids start on words: the byte counts are part of which job
    sq_take(lds, ol, L.cids, 2 * M, 4);                 // ends a chunk and of the launch order)
    L.lds_end = ol; L.scratch_end = os;
    return L;
}

SQ_HD static inline size_t sq_lsap_vec_bytes(int n) { return sq_lsap_carve(nullptr, nullptr, SQ_LSAP_A, n, 0).sparse_off; }
SQ_HD static inline size_t sq_lsap_sparse_bytes(int n, int m)
{
    const SqLsapLayout L = sq_lsap_carve(nullptr, nullptr, SQ_LSAP_A, n, m);
    return L.lds_end - L.sparse_off + 16;
}
// dynamic LDS of one job in form a
SQ_HD static inline size_t sq_lsap_lds_bytes(int n, int m) { return sq_lsap_vec_bytes(n) + sq_lsap_sparse_bytes(n, m) + 64; }
// global scratch of one job: what form c takes (Edmonds: sq_mwm_scratch_bytes, sq_algo_plan.h)
SQ_HD static inline size_t sq_lsap_scratch_bytes(int n) { return sq_lsap_carve(nullptr, nullptr, SQ_LSAP_C, n, 0).scratch_end + 64; }

// The form of a job in a launch whose blocks have lds_bytes of dynamic LDS (sq_lsap_launch_lds, sq_algo_plan.h).
// Form a needs 2m <= 65,534: rowstart counts the 2m cells, and cids names the m edges, in 16 bits.
SQ_HD static inline SqLsapForm sq_lsap_form(int n, int m, size_t lds_bytes)
{
    const bool vec_lds = sq_lsap_vec_bytes(n) + 64 <= lds_bytes;
    const bool mat_lds = vec_lds && m < 32767 && sq_lsap_lds_bytes(n, m) <= lds_bytes;
    return mat_lds ? SQ_LSAP_A : vec_lds ? SQ_LSAP_B : SQ_LSAP_C;
}

// the barriers of a one-lane run (host): none
struct SqLsapSyncNone {
    SQ_HD void operator()() const {}
    SQ_HD void after_lane0(bool) const {}
};

// One job on W lanes (every lane calls it with the same arguments and its own `lane`).  The column scan of every
// augmentation step is parallel over the lanes, everything else is scalar work on lane 0.  edges: the job's m cells
// (v, w, weight), distinct.  sync(): the lanes' barrier; sync.after_lane0(glob): the same behind lane 0's stores to the
// vectors, which the other lanes read next (glob: the vectors are in global memory, form c).  The result is L.col4row.
template <int W, class Sync, class Coop>
SQ_HD_INLINE void sq_lsap_run(const SqLsapLayout &L, SqLsapForm form, int n, int m, const SqMatchEdge *edges, int lane, Sync sync, Coop coop)
{
    const double inf = __builtin_huge_val();
    const bool mat_lds = form == SQ_LSAP_A;
    const int nw = L.nw;
    double *const cost = L.cost, *const u = L.u, *const v = L.v, *const spc = L.spc, *const wts = L.wts;
    int32_t *const path = L.path, *const col4row = L.col4row, *const row4col = L.row4col, *const remaining = L.remaining;
    uint8_t *const SR = L.SR, *const SC = L.SC;
    uint32_t *const mask = L.mask;
    uint16_t *const rowstart = L.rowstart, *const pre = L.pre, *const cids = L.cids;

    // mat = zeros; mat[v,w] = mat[w,v] = -(score**power)   (SQRNalgos.py:119-123)
    if (mat_lds) {
        for (int q = lane; q < n * nw; q += W) mask[q] = 0u;
    } else {
        for (size_t q = lane; q < (size_t)n * n; q += W) cost[q] = 0.0;
    }
    for (int q = lane; q < n; q += W) { u[q] = 0.0; v[q] = 0.0; path[q] = -1; col4row[q] = -1; row4col[q] = -1; }
    sync();
    // (the cells of the stems are distinct, so the order of these writes does not matter)
    if (mat_lds) {
        for (int e = lane; e < m; e += W) {
            const SqMatchEdge ed = edges[e];
            wts[e] = ed.weight;
            coop.or_u32(&mask[ed.v * nw + (ed.w >> 5)], 1u << (ed.w & 31));
            coop.or_u32(&mask[ed.w * nw + (ed.v >> 5)], 1u << (ed.v & 31));
        }
        sync();
        // per-word prefix counts of every row, the rows' starts (a scan over the lanes' chunks of rows)
        const int per = (n + W - 1) / W, r0 = lane * per < n ? lane * per : n, r1 = r0 + per < n ? r0 + per : n;
        int mine = 0;
        for (int r = r0; r < r1; r++) {
            int acc = 0;
            for (int w = 0; w < nw; w++) { pre[r * nw + w] = (uint16_t)acc; acc += __builtin_popcount(mask[r * nw + w]); }
            mine += acc;
        }
        int total = 0;
        int run = coop.excl_scan(mine, total);
        for (int r = r0; r < r1; r++) {
            rowstart[r] = (uint16_t)run;
            run += (int)pre[r * nw + nw - 1] + __builtin_popcount(mask[r * nw + nw - 1]);
        }
        if (lane == W - 1) rowstart[n] = (uint16_t)total;
        sync();
        for (int e = lane; e < m; e += W) {
            const SqMatchEdge ed = edges[e];
            const int a = ed.v, c = ed.w;
            cids[rowstart[a] + pre[a * nw + (c >> 5)] + __builtin_popcount(mask[a * nw + (c >> 5)] & ((1u << (c & 31)) - 1u))] = (uint16_t)e;
            cids[rowstart[c] + pre[c * nw + (a >> 5)] + __builtin_popcount(mask[c * nw + (a >> 5)] & ((1u << (a & 31)) - 1u))] = (uint16_t)e;
        }
    } else {
        for (int e = lane; e < m; e += W) {
            const SqMatchEdge ed = edges[e];
            cost[(size_t)ed.v * n + ed.w] = -ed.weight;
            cost[(size_t)ed.w * n + ed.v] = -ed.weight;
        }
    }
    sync();

    // The state of a path -- the row in hand, the columns left, the sink, the distance -- lives in registers: every lane
    // takes lane 0's decision from the same broadcast reads (until late round 4 it went through four words of LDS and two
    // barriers per step).  The scan of a step takes up to three columns per lane with the loads of one dependency level
    // issued together (remaining -> mask word, v, shortest path, owner -> edge id -> weight).
    for (int cur = 0; cur < n; cur++) {
        // ---- augmenting_path(cur)
        for (int q = lane; q < n; q += W) { remaining[q] = n - q - 1; SR[q] = 0; SC[q] = 0; spc[q] = inf; }
        int i = cur, sink = -1, nrem = n;
        double minval = 0.0;
        sync();
        while (sink == -1) {
            const double ui = u[i];
            const int rs_i = mat_lds ? (int)rowstart[i] : 0;
            double lowest = inf;
            int first = -1, lastun = -1;
            for (int it0 = 0; it0 < nrem; it0 += 3 * W) {
                int jj[3]; bool have[3];
                SQ_UNROLL
                for (int t = 0; t < 3; t++) { const int it = it0 + W * t + lane; have[t] = it < nrem; jj[t] = remaining[have[t] ? it : 0]; }
                uint32_t wd[3]; int pw[3], r4[3]; double vj[3], spj[3], cij[3];
                SQ_UNROLL
                for (int t = 0; t < 3; t++) {
                    const int j = jj[t];
                    vj[t] = v[j]; spj[t] = spc[j]; r4[t] = row4col[j];
                    if (mat_lds) { wd[t] = mask[i * nw + (j >> 5)]; pw[t] = (int)pre[i * nw + (j >> 5)]; cij[t] = 0.0; }
                    else { wd[t] = 0u; pw[t] = 0; cij[t] = cost[(size_t)i * n + j]; }
                }
                if (mat_lds) {
                    int cid[3];
                    SQ_UNROLL
                    for (int t = 0; t < 3; t++) {
                        const int j = jj[t];
                        const bool nz = (wd[t] >> (j & 31)) & 1u;
                        cid[t] = nz ? (int)cids[rs_i + pw[t] + __builtin_popcount(wd[t] & ((1u << (j & 31)) - 1u))] : -1;
                    }
                    SQ_UNROLL
                    for (int t = 0; t < 3; t++) cij[t] = cid[t] >= 0 ? -wts[cid[t]] : 0.0;
                }
                SQ_UNROLL
                for (int t = 0; t < 3; t++) {                       // (a lane's columns in scan order)
                    if (!have[t]) continue;
                    const int it = it0 + W * t + lane, j = jj[t];
                    const double r = minval + cij[t] - ui - vj[t];
                    double sp = spj[t];
                    if (r < sp) { path[j] = i; spc[j] = r; sp = r; }
                    const bool un = r4[t] == -1;
                    if (sp < lowest) { lowest = sp; first = it; lastun = un ? it : -1; }
                    else if (sp == lowest && un) lastun = it;       // sequential rule: later unassigned ties win
                }
            }
            // lane combine == the sequential scan over it = 0..nrem-1
            // (on a wave DPP row shifts / broadcasts as in the blossom kernel: the three butterfly reductions over the LDS
            // crossbar they replace -- 30 ds_bpermute per step of the path -- were the longest part of a step)
            double mn = lowest;
            coop.min_plain(mn);
            int f = (lowest == mn && first >= 0) ? first : 0x7fffffff;
            coop.min_i32(f);
            int lu = -((lowest == mn) ? lastun : -1);
            coop.min_i32(lu);
            lu = -lu;
            minval = mn;
            if (mn == inf) { if (lane == 0) SR[i] = 1; sink = -2; break; }   // infeasible (cannot happen: finite costs)
            const int index = lu >= 0 ? lu : f;
            const int j = remaining[index], lastj = remaining[nrem - 1];
            const int owner = row4col[j];
            sync();                                                 // (every lane has read what lane 0 overwrites)
            if (lane == 0) { SR[i] = 1; SC[j] = 1; remaining[index] = lastj; }
            nrem--;
            if (owner == -1) sink = j; else i = owner;
            sync.after_lane0(form == SQ_LSAP_C);
        }
        if (sink < 0) break;
        // ---- dual update
        if (lane == 0) u[cur] += minval;
        for (int q = lane; q < n; q += W) {
            if (SR[q] && q != cur) u[q] += minval - spc[col4row[q]];
            if (SC[q]) v[q] -= minval - spc[q];
        }
        sync();
        // ---- augment
        if (lane == 0) {
            int j = sink;
            for (;;) {
                const int i2 = path[j];
                row4col[j] = i2;
                const int t = col4row[i2]; col4row[i2] = j; j = t;
                if (i2 == cur) break;
            }
        }
        sync();
    }
}
