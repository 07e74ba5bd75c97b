// sq_elements_dev.hip -- the loop and pseudoknot annotation of GIVEN structures on the device (Elements): for any number of
// partner rows per record the pseudoknot level of every pair (PairsToDBN's rule, SQRNdbnseq.py:104-150), the structural
// element of every column and the list of the loops with their sizes.  No sq_batch: the caller hands over the records'
// arrays and the rows, all in its device memory.  The rules of the annotation itself are sq_elements.h.
//
// One wave per row, two passes because the loops are ragged:
//   sq_elements_levels_kernel  validates the row as sq_score_count_kernel does, forms its stems in gap-free coordinates as
//                              sq_score_fill_kernel does, takes their crossing weights and levels as the ranking tail does
//                              (sq_stem_levels_wave), writes level, STEM / PK / GAP / BREAK, status, npairs, nlevels, and
//                              the positions of the nested openers that close a listed loop, in order: nloops = 1 + their number
//   (the caller scans nloops into loop_off)
//   sq_elements_loops_kernel   lane t walks the row's t-th, t + 64-th, ... loop (the exterior loop is loop 0) with the levels
//                              as pass 0 left them in global memory: its record, loop_of and the type of its unpaired columns
// sq_extend.h is written for a block that is one wave, so the levels kernel is launched with 64-THREAD BLOCKS (its
// SQ_EXTEND_SYNC() stays the block barrier, which also orders the wave's global stores and loads); the loops kernel has
// SQ_ELEM_WAVES waves per block and no barrier.  A row is read as sq_score_dev.hip reads it: position g of the record is column
// gfcol[g] of the row and the partner of a column is the position colmap[partner] (-1: a gap column, the pair is dropped).
// A row with more stems than the launch's LDS holds (SQ_CHAIN_TMAX at most) or more than SQ_MAXLEVELS levels leaves with
// status 2: the caller annotates it on the host.
#include "sq_host_int.h"
#include "sq_extend.h"
#include "sq_elements.h"

struct SqElemArgs {
    // records
    const int64_t *pos_off; const uint8_t *codes;
    const int64_t *col_off; const int32_t *colmap, *gfcol;          // null: no record has a gap column
    // rows
    long long nrows; const int32_t *partner; const int64_t *row_start; const int32_t *row_rec; const int64_t *cell_off;
    int tmax;                                                        // stems the levels kernel's LDS holds
    int8_t *element; int16_t *level; int32_t *loop_of;
    int32_t *status, *npairs, *nlevels, *nloops;
    int32_t *openers;                                                // scratch, row q's from cell_off[q] on: its listed openers
    const int64_t *loop_off; int32_t *loops; long long loop_cap;
};

// one row as its record's gap-free positions see it: the accessor of sq_elements.h
struct SqElemRow {
    const int32_t *row, *colmap, *gfcol;
    const uint8_t *codes;
    const int16_t *lev;                                              // the row's levels by input column
    int lin, len;
    __device__ __forceinline__ int n() const { return len; }
    __device__ __forceinline__ int col(int g) const { return gfcol ? gfcol[g] : g; }
    __device__ __forceinline__ int pos(int c) const { return colmap ? colmap[c] : c; }
    __device__ __forceinline__ int partner(int g) const
    {
        const int p = row[col(g)];
        return p < 0 ? -1 : pos(p);
    }
    __device__ __forceinline__ int level(int g) const { return lev[col(g)]; }
    __device__ __forceinline__ bool sep(int g) const { return codes[g] == SQ_CODE_SEP1 || codes[g] == SQ_CODE_SEP2; }
};

__device__ __forceinline__ SqElemRow sq_elem_row(const SqElemArgs &a, long long q)
{
    SqElemRow R;
    const int rec = a.row_rec[q];
    const long long pos0 = a.pos_off[rec];
    R.len = (int)(a.pos_off[rec + 1] - pos0);
    R.codes = a.codes + pos0;
    if (!a.colmap) { R.colmap = nullptr; R.gfcol = nullptr; R.lin = R.len; }
    else {
        const long long c0 = a.col_off[rec];
        R.lin = (int)(a.col_off[rec + 1] - c0);
        R.colmap = a.colmap + c0; R.gfcol = a.gfcol + pos0;
    }
    R.row = a.partner + a.row_start[q];
    R.lev = a.level + a.cell_off[q];
    return R;
}

extern "C" __global__ __launch_bounds__(64) void sq_elements_levels_kernel(SqElemArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char sq_elem_dyn[];    // [sq_extend_lds_bytes(tmax)][the level overflow word]
    SqExtendLds L = sq_extend_lds(sq_elem_dyn, a.tmax);
    uint32_t *const ovf = reinterpret_cast<uint32_t *>(sq_elem_dyn + sq_extend_lds_bytes(a.tmax));
    const int lane = threadIdx.x;
    const long long q = blockIdx.x;
    const SqElemRow R = sq_elem_row(a, q);
    const long long c00 = a.cell_off[q];
    int8_t *const el = a.element + c00;
    int16_t *const lv = a.level + c00;
    int32_t *const lo = a.loop_of + c00;
    const int n = R.len;
    // a row that is not annotated here: no element, no level, no loop
    auto leave = [&](int st) {
        for (int c = lane; c < R.lin; c += 64) { el[c] = -1; lv[c] = 0; lo[c] = -1; }
        if (lane == 0) { a.status[q] = st; a.npairs[q] = 0; a.nlevels[q] = 0; a.nloops[q] = 0; }
    };
    bool bad = false;
    for (int c = lane; c < R.lin; c += 64) {
        const int p = R.row[c];
        if (p == -1) continue;
        if (p < 0 || p >= R.lin || p == c) { bad = true; continue; }
        if (R.row[p] != c) { bad = true; continue; }
        const int g = R.pos(c);
        if (g >= 0 && R.sep(g)) bad = true;
    }
    if (__ballot(bad) != 0ull) { leave(1); return; }                 // (wave-uniform, as every branch around a barrier below)
    // pairs and stem starts: a pair (g, pq), g < pq, starts a stem unless position g - 1 pairs with pq + 1
    int np = 0, T = 0, carry = -1;
    for (int g0 = 0; g0 < n; g0 += 64) {
        const int g = g0 + lane;
        const int pq = g < n ? R.partner(g) : -1;
        int prev = __shfl_up(pq, 1, 64);
        if (lane == 0) prev = carry;
        carry = __builtin_amdgcn_readlane(pq, 63);
        const bool opener = pq > g;
        np += (int)__popcll(__ballot(opener));
        T += (int)__popcll(__ballot(opener && prev != pq + 1));
    }
    if (T > a.tmax) { leave(2); return; }
    // the stems, in the order of their starts
    int nst = 0;
    carry = -1;
    for (int g0 = 0; g0 < n; g0 += 64) {
        const int g = g0 + lane;
        const int pq = g < n ? R.partner(g) : -1;
        int prev = __shfl_up(pq, 1, 64);
        if (lane == 0) prev = carry;
        carry = __builtin_amdgcn_readlane(pq, 63);
        const bool start = pq > g && prev != pq + 1;
        const unsigned long long sm = __ballot(start);
        if (start) {
            int len = 0, gg = g, qq = pq;
            do { len++; gg++; qq--; } while (gg < qq && R.partner(gg) == qq);
            const int at = nst + (int)__popcll(sm & ((1ull << lane) - 1ull));
            L.i[at] = (int16_t)g; L.j[at] = (int16_t)pq; L.len[at] = (int16_t)len;
        }
        nst += (int)__popcll(sm);
    }
    if (lane == 0) *ovf = 0u;
    __syncthreads();
    bool anyc = false;
    for (int s = lane; s < T; s += 64) {                             // crossing weights (:121-124)
        const int si = L.i[s], sj = L.j[s];
        int cc = 0;
        for (int p = 0; p < T; p++) if (sq_chain_cross(si, sj, L.i[p], L.j[p])) cc += L.len[p];
        L.cc[s] = cc;
        anyc |= cc != 0;
    }
    const bool cross = __ballot(anyc) != 0ull;
    __syncthreads();
    int nlev = T ? 1 : 0;
    if (cross) nlev = sq_stem_levels_wave(L, T, lane, ovf);
    if (*ovf) { leave(2); return; }                                  // (more than SQ_MAXLEVELS levels)
    // what a column is before the loops are known; an unpaired column gets its loop's type from the loops kernel
    for (int c = lane; c < R.lin; c += 64) {
        const int g = R.pos(c);
        el[c] = (int8_t)(g < 0 ? SQ_ELEM_GAP : R.sep(g) ? SQ_ELEM_BREAK : SQ_ELEM_EXTERIOR);
        lv[c] = 0; lo[c] = -1;
    }
    __syncthreads();
    for (int s = lane; s < T; s += 64) {
        const int l = cross ? L.lvl[s] : 1;
        const int si = L.i[s], sj = L.j[s], sl = L.len[s];
        const int8_t what = (int8_t)(l == 1 ? SQ_ELEM_STEM : SQ_ELEM_PK);
        for (int k = 0; k < sl; k++) {
            const int c = R.col(si + k), d = R.col(sj - k);
            lv[c] = (int16_t)l; lv[d] = (int16_t)-l;
            el[c] = what; el[d] = what;
        }
    }
    __syncthreads();                                                 // (the levels are read back by other lanes)
    // the nested openers that close a listed loop, in order
    int32_t *const openers = a.openers + c00;
    int nl = 0;
    for (int g0 = 0; g0 < n; g0 += 64) {
        const int g = g0 + lane;
        const bool listed = g < n && sq_elem_listed(R, g);
        const unsigned long long m = __ballot(listed);
        if (listed) openers[nl + (int)__popcll(m & ((1ull << lane) - 1ull))] = g;
        nl += (int)__popcll(m);
    }
    if (lane == 0) { a.status[q] = 0; a.npairs[q] = np; a.nlevels[q] = nlev; a.nloops[q] = 1 + nl; }
}

extern "C" __global__ __launch_bounds__(64 * SQ_ELEM_WAVES) void sq_elements_loops_kernel(SqElemArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * SQ_ELEM_WAVES + (threadIdx.x >> 6);
    if (q >= a.nrows) return;                                        // (wave-uniform; the kernel has no block barrier)
    if (a.status[q] != 0) return;
    const SqElemRow R = sq_elem_row(a, q);
    const long long c00 = a.cell_off[q], l0 = a.loop_off[q];
    int8_t *const el = a.element + c00;
    int32_t *const lo = a.loop_of + c00;
    const int32_t *const openers = a.openers + c00;
    const int nl = a.nloops[q];
    for (int k = lane; k < nl; k += 64) {                            // loop 0: the exterior loop, "closed" by (-1, n)
        const bool ext = k == 0;
        const int g = ext ? -1 : openers[k - 1];
        const int w = ext ? R.len : R.partner(g);
        const SqElemLoop lp = sq_elem_walk(R, g, w, [](int) {});
        const int type = sq_elem_type(ext, lp);                      // (never a stack: no listed opener closes one)
        if (l0 + k < a.loop_cap) {
            int32_t *const rec = a.loops + 6 * (l0 + k);
            rec[0] = type; rec[1] = ext ? -1 : R.col(g); rec[2] = ext ? R.lin : R.col(w);
            rec[3] = lp.branches; rec[4] = lp.unpaired; rec[5] = lp.side5;
        }
        sq_elem_walk(R, g, w, [&](int p) {
            const int c = R.col(p);
            lo[c] = k;
            if (R.level(p) == 0) el[c] = (int8_t)type;               // (a column of a pair of level >= 2 stays PK)
        });
    }
}

static size_t elements_scratch_ints(int64_t cells) { return align_up((size_t)std::max<int64_t>(cells, 1), 4); }

extern "C" size_t sq_elements_scratch(int64_t cells)
{
    return cells >= 0 ? sizeof(int32_t) * elements_scratch_ints(cells) : 0;
}

extern "C" int sq_elements_rows(const sq_elements_desc *d, const sq_elements_rowset *o, int32_t pass, void *d_scratch, size_t scratch_bytes,
                                void *hip_stream)
{
    if (!d || !o || (pass != 0 && pass != 1) || d->nrec < 0 || o->nrows < 0 || o->cells < 0 || d->max_len < 0 || d->max_len > 32768 ||
        !d_scratch) { sq_set_error("bad argument"); return -1; }
    if (o->nrows && (!d->nrec || !d->d_pos_off || !d->d_codes || (d->d_colmap && (!d->d_col_off || !d->d_gfcol)) || !o->d_partner ||
                     !o->d_row_start || !o->d_row_rec || !o->d_cell_off || !o->d_element || !o->d_level || !o->d_loop_of || !o->d_status ||
                     !o->d_npairs || !o->d_nlevels || !o->d_nloops ||
                     (pass == 1 && (!o->d_loop_off || o->loop_cap < 0 || (o->loop_cap && !o->d_loops)))))
        { sq_set_error("bad argument"); return -1; }
    if (scratch_bytes < sq_elements_scratch(o->cells)) {
        sq_set_error("sq_elements_rows: scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(sq_elements_scratch(o->cells)) +
                     " needed");
        return -1;
    }
    if (o->nrows > 0x7fffffffll) { sq_set_error("sq_elements_rows: too many rows"); return -1; }
    if (!o->nrows) return 0;
    hipStream_t st = (hipStream_t)hip_stream;
    SqElemArgs a{};
    a.pos_off = d->d_pos_off; a.codes = d->d_codes; a.col_off = d->d_col_off; a.colmap = d->d_colmap; a.gfcol = d->d_gfcol;
    a.nrows = o->nrows; a.partner = o->d_partner; a.row_start = o->d_row_start; a.row_rec = o->d_row_rec; a.cell_off = o->d_cell_off;
    // (a structure of n positions has at most n / 2 stems; rows beyond what 160 KB of LDS hold go back to the caller)
    a.tmax = std::min(std::max(d->max_len / 2, 8), SQ_CHAIN_TMAX);
    a.element = o->d_element; a.level = o->d_level; a.loop_of = o->d_loop_of;
    a.status = o->d_status; a.npairs = o->d_npairs; a.nlevels = o->d_nlevels; a.nloops = o->d_nloops;
    a.openers = (int32_t *)d_scratch;
    a.loop_off = o->d_loop_off; a.loops = o->d_loops; a.loop_cap = o->loop_cap;
    if (pass == 0) {
        const size_t lds = sq_extend_lds_bytes(a.tmax) + 16;
        if (lds > 64 * 1024) sq_max_dynamic_lds((const void *)sq_elements_levels_kernel, 160 * 1024);
        hipLaunchKernelGGL(sq_elements_levels_kernel, dim3((unsigned)o->nrows), dim3(64), lds, st, a);
        return sq_check(hipGetLastError(), "sq_elements_levels_kernel");
    }
    const dim3 grid((unsigned)((o->nrows + SQ_ELEM_WAVES - 1) / SQ_ELEM_WAVES)), block(64 * SQ_ELEM_WAVES);
    hipLaunchKernelGGL(sq_elements_loops_kernel, grid, block, 0, st, a);
    return sq_check(hipGetLastError(), "sq_elements_loops_kernel");
}
