// sq_score_dev.hip -- ScoreStruct and the metrics of GIVEN structures on the device (Score): what the reference computes for a
// `reference` line, ReferenceScores (SQRNdbnseq.py:958-970) = ScoreStruct(shortseq, PairsToStems(sorted(pairs)), shortreacts)
// (:861-899, :498-517), and TP / FP / FN / FS / PR / RC against the record's known structure (:1249-1258), for any number of
// partner rows per record.  No sq_batch: the caller hands over the records' arrays and the rows, all in its device memory.
//
// One wave per row, two passes because the stems are ragged:
//   sq_score_count_kernel   validates the row (partner in range, p[p[i]] == i, p[i] != i, no pair on a separator), drops the
//                           pairs that touch a gap column, counts pairs and stem starts: status, npairs, nstems
//   (the caller scans nstems into stem_off)
//   sq_score_fill_kernel    the stems in input coordinates, every stem's pair-value sum and its power from the host libm's
//                           table, the sum over the stems in ascending order, the position-order reactivity sum, round(., 3),
//                           TP against the known structure's partner row
// A row is read in gap-free coordinates: position g of the record is column gfcol[g] of the row, and the partner of a
// column is the position colmap[partner] (-1: a gap column, the pair is dropped -- UnAlign, :243-249).  A pair (g, q), g < q,
// starts a stem unless position g - 1 pairs with q + 1; a stem's lane walks its stack.  The records' known structures go
// through the same kernels as one more row each (already gap-free: no maps), which fills ref_scores.
#include "sq_host_int.h"
#include "sq_scoring.h"

#define SQ_SCORE_WAVES 4                // waves (rows) of a block

struct SqScoreArgs {
    // records
    const int64_t *pos_off; const uint8_t *codes; const double *reacts; const uint8_t *has_reacts; const int32_t *nsep;
    const int64_t *col_off; const int32_t *colmap, *gfcol;          // null: no record has a gap column
    const int32_t *known, *known_n;                                  // the known structures for TP (null: not compared)
    const double *pow17; int pow_len;
    // rows
    long long nrows; const int32_t *partner; const int64_t *row_start; const int32_t *row_rec;   // row_start null: a record's known structure
    int check_sep, bitwords;
    int32_t *status, *npairs, *nstems;
    const int64_t *stem_off; int32_t *stems; long long stem_cap;
    double *scores, *metrics;
};

// one row as its record's gap-free positions see it
struct SqScoreRow {
    const int32_t *row, *colmap, *gfcol;
    const uint8_t *codes;
    int lin, n, rec;
    long long pos0;
    __device__ __forceinline__ int col(int g) const { return gfcol ? gfcol[g] : g; }
    // partner of position g in gap-free coordinates; -1: unpaired, or its pair touches a gap column
    __device__ __forceinline__ int partner(int g) const
    {
        const int p = row[col(g)];
        return p < 0 ? -1 : (colmap ? colmap[p] : p);
    }
};

__device__ __forceinline__ bool sq_score_row(const SqScoreArgs &a, long long q, SqScoreRow &R)
{
    const bool own = a.row_start == nullptr;
    R.rec = own ? (int)q : a.row_rec[q];
    R.pos0 = a.pos_off[R.rec];
    R.n = (int)(a.pos_off[R.rec + 1] - R.pos0);
    R.codes = a.codes + R.pos0;
    if (own || !a.colmap) { R.colmap = nullptr; R.gfcol = nullptr; R.lin = R.n; }
    else {
        const long long c0 = a.col_off[R.rec];
        R.lin = (int)(a.col_off[R.rec + 1] - c0);
        R.colmap = a.colmap + c0; R.gfcol = a.gfcol + R.pos0;
    }
    R.row = a.partner + (own ? R.pos0 : a.row_start[q]);
    return !(own && a.known_n[R.rec] < 0);                           // false: the record has no known structure, no row
}

extern "C" __global__ __launch_bounds__(64 * SQ_SCORE_WAVES) void sq_score_count_kernel(SqScoreArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * SQ_SCORE_WAVES + (threadIdx.x >> 6);
    if (q >= a.nrows) return;                                        // (wave-uniform)
    SqScoreRow R;
    int st = 0, np = 0, ns = 0;
    if (sq_score_row(a, q, R)) {
        bool bad = false;
        for (int c0 = 0; c0 < R.lin; c0 += 64) {
            const int c = c0 + lane;
            if (c >= R.lin) continue;
            const int p = R.row[c];
            if (p == -1) continue;
            if (p < 0 || p >= R.lin || p == c) { bad = true; continue; }
            if (R.row[p] != c) { bad = true; continue; }
            if (a.check_sep) {
                const int g = R.colmap ? R.colmap[c] : c;
                if (g >= 0 && (R.codes[g] == SQ_CODE_SEP1 || R.codes[g] == SQ_CODE_SEP2)) bad = true;
            }
        }
        if (__ballot(bad) != 0ull || R.n - a.nsep[R.rec] <= 0) st = 1;      // (no position to score: the reference divides by zero)
        else {
            int carry = -1;                                          // the partner of the position before the chunk
            for (int g0 = 0; g0 < R.n; g0 += 64) {
                const int g = g0 + lane;
                const int pq = g < R.n ? R.partner(g) : -1;
                int prev = __shfl_up(pq, 1, 64);
                if (lane == 0) prev = carry;
                carry = __builtin_amdgcn_readlane(pq, 63);
                const bool opener = pq > g;
                np += (int)__popcll(__ballot(opener));
                ns += (int)__popcll(__ballot(opener && prev != pq + 1));
            }
        }
    }
    if (lane == 0) { a.status[q] = st; a.npairs[q] = np; a.nstems[q] = ns; }
}

extern "C" __global__ __launch_bounds__(64 * SQ_SCORE_WAVES) void sq_score_fill_kernel(SqScoreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bits_dyn[];     // [waves of the block][bitwords]: paired positions
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * SQ_SCORE_WAVES + wave;
    if (q >= a.nrows) return;                                        // (wave-uniform; the kernel has no block barrier)
    SqScoreRow R;
    const bool have = sq_score_row(a, q, R);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (!have || a.status[q] != 0) {
        if (lane < 3) a.scores[3 * q + lane] = nan;
        if (a.metrics && lane < 6) a.metrics[6 * q + lane] = nan;
        return;
    }
    const int n = R.n;
    const bool marks = a.has_reacts[R.rec] != 0 && n <= 32 * a.bitwords;
    uint32_t *const s_bits = s_bits_dyn + (size_t)wave * a.bitwords;
    if (marks) {
        for (int w = lane; w < (n + 31) / 32; w += 64) s_bits[w] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    const int32_t *known = a.known && a.known_n[R.rec] >= 0 ? a.known + R.pos0 : nullptr;
    const long long s0 = a.stems ? a.stem_off[q] : 0;
    uint32_t inexact = a.has_reacts[R.rec] != 0 && !marks ? 1u : 0u;   // (a record beyond the bitmap: cannot happen below 32,768 nt)
    double thescore = 0;
    int nst = 0, np = 0, tp = 0, carry = -1;
    for (int g0 = 0; g0 < n; g0 += 64) {
        const int g = g0 + lane;
        const int pq = g < n ? R.partner(g) : -1;
        int prev = __shfl_up(pq, 1, 64);
        if (lane == 0) prev = carry;
        carry = __builtin_amdgcn_readlane(pq, 63);
        const bool opener = pq > g;
        const bool start = opener && prev != pq + 1;
        np += (int)__popcll(__ballot(opener));
        tp += (int)__popcll(__ballot(opener && known && known[g] == pq));
        const unsigned long long sm = __ballot(start);
        double f = 0;
        if (start) {
            // the stem's stack: (g, pq), (g + 1, pq - 1), ... while the next position pairs with the position before the last closer
            int len = 0, gg = g, qq = pq;
            double bpsum = 0;
            do {
                bpsum += sq_pair_value(R.codes[gg], R.codes[qq]);      // (multiples of 1/2: exact in any order)
                if (marks) { atomicOr(&s_bits[gg >> 5], 1u << (gg & 31)); atomicOr(&s_bits[qq >> 5], 1u << (qq & 31)); }
                len++; gg++; qq--;
            } while (gg < qq && R.partner(gg) == qq);
            if (bpsum > 0) {                                           // :884  bpsum ** 1.7 through the host libm's table
                const int idx = (int)(bpsum * 2.0);
                if (idx < a.pow_len) f = a.pow17[idx]; else inexact = 1u;
            }
            if (a.stems) {
                const long long at = s0 + nst + (long long)__popcll(sm & ((1ull << lane) - 1ull));
                if (at < a.stem_cap) { const int c = R.col(g); a.stems[3 * at] = c; a.stems[3 * at + 1] = R.row[c]; a.stems[3 * at + 2] = len; }
            }
        }
        nst += (int)__popcll(sm);
        const int flo = __double2loint(f), fhi = __double2hiint(f);
        for (unsigned long long m = sm; m != 0ull; m &= m - 1ull) {  // the reference's order of additions (u is uniform: v_readlane)
            const int u = (int)__ffsll((long long)m) - 1;
            thescore += __hiloint2double(__builtin_amdgcn_readlane(fhi, u), __builtin_amdgcn_readlane(flo, u));
        }
    }
    const int nsep = a.nsep[R.rec];
    double reactscore;
    if (a.has_reacts[R.rec] == 0) {
        // every term is exactly 0.5: the sum is 0.5 (n - nsep) whatever the order
        reactscore = 1 - (0.5 * (double)(n - nsep)) / (double)(n - nsep);
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const double *reacts = a.reacts + R.pos0;
        // :894-896, position by position: the reference's order of additions, so the sum is serial.  Every lane runs it with
        // the same addresses -- a wave-wide load of ONE address is one broadcast request, not 64 -- and ends with the same value,
        // so no lane has to hand it on (the ranking tail's form).  n steps per row: the cost of a row with reactivities; a
        // record scored under thousands of rows would gain from staging codes and reactivities in LDS once per block.
        double acc = 0;
        if (marks)
            for (int i = 0; i < n; i++) {
                const int cd = R.codes[i];
                if (cd == SQ_CODE_SEP1 || cd == SQ_CODE_SEP2) continue;
                const double r = reacts[i];
                acc += ((s_bits[i >> 5] >> (i & 31)) & 1u) ? r : 1 - r;
            }
        reactscore = 1 - acc / (double)(n - nsep);
    }
    inexact = __ballot(inexact != 0u) != 0ull ? 1u : 0u;
    double sc[3], m[6];
    sc[0] = sq_round3(thescore * reactscore, &inexact);
    sc[1] = sq_round3(thescore, &inexact);
    sc[2] = sq_round3(reactscore, &inexact);
    if (a.metrics) {
        if (known) sq_prf_counts(tp, np, a.known_n[R.rec], m, &inexact);
        else for (int k = 0; k < 6; k++) m[k] = nan;
    }
    if (lane == 0) {
        for (int k = 0; k < 3; k++) a.scores[3 * q + k] = sc[k];
        if (a.metrics) for (int k = 0; k < 6; k++) a.metrics[6 * q + k] = m[k];
        if (inexact) a.status[q] = 2;                                  // the caller recomputes the row on the host
    }
}

static size_t score_scratch_ints(int32_t nrec) { return align_up((size_t)std::max(nrec, 1), 4); }

extern "C" size_t sq_score_scratch(int32_t nrec)
{
    return nrec >= 0 ? 2 * sizeof(int32_t) * score_scratch_ints(nrec) : 0;
}

extern "C" int sq_score_structs_dev(const sq_score_desc *d, const sq_score_rows *o, int32_t pass, void *d_scratch, size_t scratch_bytes,
                                    void *hip_stream)
{
    if (!d || !o || (pass != 0 && pass != 1) || d->nrec < 0 || o->nrows < 0 || d->max_react_len < 0 || d->max_react_len > 32768 ||
        d->pow_len < 1 || !d_scratch) { sq_set_error("bad argument"); return -1; }
    if (d->nrec && (!d->d_pos_off || !d->d_codes || !d->d_has_reacts || !d->d_nsep || !d->d_known || !d->d_known_n || !d->d_pow ||
                    !o->d_ref_scores || !o->d_ref_status || (d->max_react_len && !d->d_reacts) ||
                    (d->d_colmap && (!d->d_col_off || !d->d_gfcol)))) { sq_set_error("bad argument"); return -1; }
    if (o->nrows && (!d->nrec || !o->d_partner || !o->d_row_start || !o->d_row_rec || !o->d_status || !o->d_npairs || !o->d_nstems ||
                     !o->d_scores || !o->d_metrics || (pass == 1 && (!o->d_stem_off || o->stem_cap < 0 || (o->stem_cap && !o->d_stems)))))
        { sq_set_error("bad argument"); return -1; }
    if (scratch_bytes < sq_score_scratch(d->nrec)) {
        sq_set_error("sq_score_structs_dev: scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(sq_score_scratch(d->nrec)) +
                     " needed");
        return -1;
    }
    if ((o->nrows + SQ_SCORE_WAVES - 1) / SQ_SCORE_WAVES > 0x7fffffffll) { sq_set_error("sq_score_structs_dev: too many rows"); return -1; }
    hipStream_t st = (hipStream_t)hip_stream;
    SqScoreArgs a{};
    a.pos_off = d->d_pos_off; a.codes = d->d_codes; a.reacts = d->d_reacts; a.has_reacts = d->d_has_reacts; a.nsep = d->d_nsep;
    a.col_off = d->d_col_off; a.colmap = d->d_colmap; a.gfcol = d->d_gfcol;
    a.known = d->d_known; a.known_n = d->d_known_n; a.pow17 = d->d_pow; a.pow_len = d->pow_len;
    // (one bitmap of the record's positions per wave, sized for the call's longest record with reactivities; 16-byte rows)
    a.bitwords = (int)align_up((size_t)(d->max_react_len + 31) / 32, 4);
    const size_t lds = pass == 1 ? sizeof(uint32_t) * SQ_SCORE_WAVES * (size_t)a.bitwords : 0;
    auto launch = [&](long long nrows) {
        const dim3 grid((unsigned)((nrows + SQ_SCORE_WAVES - 1) / SQ_SCORE_WAVES)), block(64 * SQ_SCORE_WAVES);
        if (pass == 0) hipLaunchKernelGGL(sq_score_count_kernel, grid, block, 0, st, a);
        else hipLaunchKernelGGL(sq_score_fill_kernel, grid, block, lds, st, a);
        return sq_check(hipGetLastError(), pass == 0 ? "sq_score_count_kernel" : "sq_score_fill_kernel");
    };
    if (o->nrows) {
        a.nrows = o->nrows; a.partner = o->d_partner; a.row_start = o->d_row_start; a.row_rec = o->d_row_rec; a.check_sep = 1;
        a.status = o->d_status; a.npairs = o->d_npairs; a.nstems = o->d_nstems;
        a.stem_off = o->d_stem_off; a.stems = o->stem_cap ? o->d_stems : nullptr; a.stem_cap = o->stem_cap;
        a.scores = o->d_scores; a.metrics = o->d_metrics;
        if (int rc = launch(o->nrows)) return rc;
    }
    if (d->nrec) {
        // the known structures: one row per record, in gap-free coordinates already (a record without one: NaN)
        int32_t *const cnt = (int32_t *)d_scratch;
        a.nrows = d->nrec; a.partner = d->d_known; a.row_start = nullptr; a.row_rec = nullptr; a.check_sep = 0;
        a.known = nullptr;
        a.status = o->d_ref_status; a.npairs = cnt; a.nstems = cnt + score_scratch_ints(d->nrec);
        a.stem_off = nullptr; a.stems = nullptr; a.stem_cap = 0;
        a.scores = o->d_ref_scores; a.metrics = nullptr;
        if (int rc = launch(d->nrec)) return rc;
    }
    return 0;
}
