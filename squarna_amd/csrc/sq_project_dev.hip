// Structures between the columns of an alignment and the residues of its rows (Project, Lift), on the device.  Gap map, pair
// classes, predicates and the kept rule: sq_project.h.
//
//   sq_project_kernel   per alignment row: the gap map, col_of / pos_of, and per structure line over the columns the projected
//                       partners in residue coordinates, the class of every pair in that row and the counts
//   sq_lift_kernel      per alignment row: the gap map, col_of / pos_of, and per structure line over the row's residues the
//                       partners over the columns
//
// One block of SQ_PROJ_THREADS threads takes the rows blockIdx.x, + gridDim.x, ...  The gap map of the row in hand lives in
// LDS as the 64-bit ballot words of "is a residue" per chunk of 64 columns and the chunks' exclusive bases (6 KB at the
// largest L), beside the row's class bytes (32 KB at the largest L): 38.3 KB of static LDS.  Every output cell of a row is
// written by the kernel, padding included; nothing is cleared beforehand and there is no global atomic.  All buffers are the
// caller's device memory; nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_project.h"

namespace {

struct RowMap {                       // the LDS of a block
    uint64_t word[SQ_PROJ_MAX_WORDS];
    int32_t base[SQ_PROJ_MAX_WORDS + 1];
    uint8_t cls[SQ_PROJ_MAX_COLS];
    uint8_t tab[256];
    int32_t cnt[SQ_PROJ_COUNTS];
    int32_t bad;
};
static_assert(sizeof(RowMap) <= 64 * 1024, "static LDS stays at or below 64 KB");

// The chunk walk of one row: a wave per chunk of 64 columns, lane = column.  The bytes are loaded coalesced and classed
// through the table; the ballot of "is a residue" is the chunk's word, its popcount goes to base[], which wave 0 then turns
// into exclusive bases (lane l sums the chunks l * per .. l * per + per - 1, per = ceil(nW / 64) <= 8, and the lanes' sums
// are scanned with shuffles).  Returns the row's residues; ends with the map visible to the block.
__device__ int32_t walk_row(RowMap &m, const uint8_t *row, int32_t L)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t nW = SqProject::words(L);
    __syncthreads();                                                 // (the row before this one has been read)
    for (int32_t j = wave; j < nW; j += SQ_PROJ_THREADS / 64) {      // (wave-uniform)
        const int32_t c = j * 64 + lane;
        const uint8_t k = c < L ? m.tab[row[c]] : (uint8_t)SQ_COV_GAP;
        if (c < L) m.cls[c] = k;
        const unsigned long long mask = __ballot(SqProject::is_residue(k));
        if (lane == 0) {
            m.word[j] = mask;
            m.base[j] = __popcll(mask);
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int32_t per = (nW + 63) / 64, first = lane * per;
        int32_t mine = 0;
        for (int32_t j = first; j < first + per && j < nW; j++) mine += m.base[j];
        int32_t run = mine;                                          // inclusive scan over the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(run, d);
            if (lane >= d) run += up;
        }
        int32_t at = run - mine;
        for (int32_t j = first; j < first + per && j < nW; j++) {
            const int32_t n = m.base[j];
            m.base[j] = at;
            at += n;
        }
        if (lane == 63) m.base[nW] = run;
    }
    __syncthreads();
    return m.base[nW];
}

// length, col_of (with its padding up to Lmax; of a row with more residues than Lmax, the first Lmax) and pos_of of row r
// from the map.
__device__ void write_maps(const RowMap &m, int64_t r, int32_t L, int32_t Lmax, int32_t length, int32_t *d_length, int32_t *d_col_of,
                           int32_t *d_pos_of)
{
    const int tid = threadIdx.x;
    if (tid == 0) d_length[r] = length;
    for (int32_t c = tid; c < L; c += SQ_PROJ_THREADS) {
        const bool res = SqProject::residue_at(m.word, c);
        const int32_t i = SqProject::pos(m.word, m.base, c);
        d_pos_of[r * L + c] = res ? i : -1;
        if (res && i < Lmax) d_col_of[r * Lmax + i] = c;
    }
    for (int32_t i = length + tid; i < Lmax; i += SQ_PROJ_THREADS) d_col_of[r * Lmax + i] = -1;
}

}  // namespace

// structs: line k of row r is the L partners at structs[r * row_stride + k * L ..]; row_stride = 0: the K lines are shared
// by all rows (they stay in L2), else K * L.
extern "C" __global__ __launch_bounds__(SQ_PROJ_THREADS) void sq_project_kernel(const uint8_t *rows, int32_t R, int32_t L,
                                                                               const int32_t *structs, int64_t row_stride, int32_t K,
                                                                               int32_t Lmax, int32_t canonical_only, int32_t min_loop,
                                                                               int32_t *d_length, int32_t *d_col_of, int32_t *d_pos_of,
                                                                               int32_t *d_partner, uint8_t *d_cls, int32_t *d_counts,
                                                                               int32_t *d_status)
{
    __shared__ RowMap m;
    const int tid = threadIdx.x, lane = tid & 63;
    m.tab[tid] = SqProject::table_entry(tid);                        // (256 threads, 256 entries; walk_row begins with a barrier)
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {            // (block-uniform)
        const int32_t length = walk_row(m, rows + r * L, L);
        const bool fits = length <= Lmax;
        write_maps(m, r, L, Lmax, length, d_length, d_col_of, d_pos_of);
        for (int32_t k = 0; k < K; k++) {
            const int32_t *line = structs + r * row_stride + (int64_t)k * L;
            int32_t *out = d_partner + (r * K + k) * (int64_t)Lmax;
            uint8_t *out_cls = d_cls + (r * K + k) * (int64_t)L;
            if (tid < SQ_PROJ_COUNTS) m.cnt[tid] = 0;
            if (tid == 0) m.bad = 0;
            __syncthreads();
            bool bad = false;
            for (int32_t c = tid; c < L; c += SQ_PROJ_THREADS) {
                const int32_t p = line[c];
                const int32_t back = p >= 0 && SqProject::partner_in_range(p, L) ? line[p] : c;
                bad |= SqProject::column_bad(c, p, back, L);
            }
            if (__any(bad) && lane == 0) m.bad = 1;                  // (every writer stores the same value)
            __syncthreads();
            const bool valid = !m.bad && fits;                       // (block-uniform)
            if (valid) {
                int32_t cnt[SQ_PROJ_COUNTS] = {};                    // (wave-uniform: sums of popcounts of ballots)
                for (int32_t c0 = (tid >> 6) * 64; c0 < L; c0 += SQ_PROJ_THREADS) {   // (wave-uniform)
                    const int32_t c = c0 + lane;
                    const int32_t p = c < L ? line[c] : -1;
                    int pc = SQ_PROJ_NONE;
                    bool keep = false, loop_drop = false;
                    if (p >= 0) pc = SqProject::judge(m.cls, m.word, m.base, c, p, canonical_only != 0, min_loop, keep, loop_drop);
                    const bool opens = p > c;
                    if (c < L) {
                        out_cls[c] = (uint8_t)(opens ? pc : SQ_PROJ_NONE);
                        if (SqProject::residue_at(m.word, c))
                            out[SqProject::pos(m.word, m.base, c)] = keep ? SqProject::pos(m.word, m.base, p) : -1;
                    }
                    const unsigned long long open_mask = __ballot(opens);
                    if (open_mask) {                                 // (wave-uniform)
                        cnt[SQ_PROJ_CNT_PAIRS] += __popcll(open_mask);
                        for (int q = SQ_PROJ_AU; q <= SQ_PROJ_BOTH_GAP; q++) cnt[q] += __popcll(__ballot(opens && pc == q));
                        cnt[SQ_PROJ_CNT_DROPPED] += __popcll(__ballot(opens && loop_drop));
                        cnt[SQ_PROJ_CNT_KEPT] += __popcll(__ballot(opens && keep));
                    }
                }
                if (lane < SQ_PROJ_COUNTS) {
                    int32_t v = 0;
                    for (int q = 0; q < SQ_PROJ_COUNTS; q++) v = lane == q ? cnt[q] : v;
                    atomicAdd(&m.cnt[lane], v);                      // (LDS: the four waves' sums)
                }
                for (int32_t i = length + tid; i < Lmax; i += SQ_PROJ_THREADS) out[i] = -1;
            } else {
                for (int32_t i = tid; i < Lmax; i += SQ_PROJ_THREADS) out[i] = -1;
                for (int32_t c = tid; c < L; c += SQ_PROJ_THREADS) out_cls[c] = SQ_PROJ_NONE;
            }
            __syncthreads();
            if (tid < SQ_PROJ_COUNTS) d_counts[(r * K + k) * SQ_PROJ_COUNTS + tid] = m.cnt[tid];
            if (tid == 0) d_status[r * K + k] = !fits ? SQ_PROJ_NO_ROOM : m.bad ? SQ_PROJ_INVALID : SQ_PROJ_OK;
            __syncthreads();                                         // (cnt and bad are cleared next)
        }
    }
}

// short_rows: line k < nstruct[r] of row r is the partners, in residue coordinates, at short_rows[start[r] + k * stride[r] ..],
// of which the row's `length` first are read.  A lane at a residue column c reads the partner i of residue pos(c) and writes
// col(i): a search over the chunk bases, then a select within the chunk's word, all from LDS.
extern "C" __global__ __launch_bounds__(SQ_PROJ_THREADS) void sq_lift_kernel(const uint8_t *rows, int32_t R, int32_t L,
                                                                            const int32_t *short_rows, int64_t short_len,
                                                                            const int64_t *start, const int32_t *stride,
                                                                            const int32_t *nstruct, int32_t K, int32_t Lmax,
                                                                            int32_t *d_length, int32_t *d_col_of, int32_t *d_pos_of,
                                                                            int32_t *d_partner, int32_t *d_status)
{
    __shared__ RowMap m;
    const int tid = threadIdx.x, lane = tid & 63;
    m.tab[tid] = SqProject::table_entry(tid);
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {            // (block-uniform)
        const int32_t length = walk_row(m, rows + r * L, L), nW = SqProject::words(L);
        const bool fits = length <= Lmax;
        write_maps(m, r, L, Lmax, length, d_length, d_col_of, d_pos_of);
        const int64_t first = start[r];
        const int32_t step = stride[r];
        const int32_t n = nstruct[r] < 0 ? 0 : nstruct[r] > K ? K : nstruct[r];
        const bool room = fits && first >= 0 && step >= length && first <= short_len - (int64_t)n * step;   // (step >= 0 then)
        for (int32_t k = 0; k < K; k++) {
            int32_t *out = d_partner + (r * K + k) * (int64_t)L;
            const bool given = k < n;
            const int32_t *line = given && room ? short_rows + first + (int64_t)k * step : short_rows;   // (read only when both hold)
            if (tid == 0) m.bad = 0;
            __syncthreads();
            if (given && room) {
                bool bad = false;
                for (int32_t i = tid; i < length; i += SQ_PROJ_THREADS) {
                    const int32_t p = line[i];
                    const int32_t back = p >= 0 && SqProject::partner_in_range(p, length) ? line[p] : i;
                    bad |= SqProject::column_bad(i, p, back, length);
                }
                if (__any(bad) && lane == 0) m.bad = 1;
            }
            __syncthreads();
            const bool valid = given && room && !m.bad;              // (block-uniform)
            for (int32_t c = tid; c < L; c += SQ_PROJ_THREADS) {
                int32_t to = -1;
                if (valid && SqProject::residue_at(m.word, c)) {
                    const int32_t p = line[SqProject::pos(m.word, m.base, c)];
                    if (p >= 0) to = SqProject::col(m.word, m.base, nW, p);
                }
                out[c] = to;
            }
            if (tid == 0) d_status[r * K + k] = !given ? SQ_PROJ_OK : !room ? SQ_PROJ_NO_ROOM : m.bad ? SQ_PROJ_INVALID : SQ_PROJ_OK;
            __syncthreads();                                         // (bad is cleared next)
        }
    }
}

static bool sizes_ok(int32_t R, int32_t L, int32_t K, int32_t Lmax)
{
    return R >= 1 && R <= SQ_PROJ_MAX_ROWS && L >= 1 && L <= SQ_PROJ_MAX_COLS && K >= 1 && Lmax >= 1 && Lmax <= SQ_PROJ_MAX_COLS;
}

extern "C" int sq_project_rows(const uint8_t *d_rows, int32_t R, int32_t L, const int32_t *d_structs, int64_t row_stride, int32_t K,
                               int32_t Lmax, int32_t canonical_only, int32_t min_loop, int32_t *d_length, int32_t *d_col_of,
                               int32_t *d_pos_of, int32_t *d_partner, uint8_t *d_cls, int32_t *d_counts, int32_t *d_status,
                               void *hip_stream)
{
    if (!d_rows || !d_structs || !d_length || !d_col_of || !d_pos_of || !d_partner || !d_cls || !d_counts || !d_status ||
        !sizes_ok(R, L, K, Lmax) || (row_stride != 0 && row_stride != (int64_t)K * L) || min_loop < 0 ||
        (canonical_only != 0 && canonical_only != 1)) {
        sq_set_error("sq_project_rows: bad argument");
        return -1;
    }
    const dim3 grid((unsigned)std::min<int32_t>(R, SQ_PROJ_MAX_BLOCKS)), block(SQ_PROJ_THREADS);
    hipLaunchKernelGGL(sq_project_kernel, grid, block, 0, (hipStream_t)hip_stream, d_rows, R, L, d_structs, row_stride, K, Lmax,
                       canonical_only, min_loop, d_length, d_col_of, d_pos_of, d_partner, d_cls, d_counts, d_status);
    return sq_check(hipGetLastError(), "sq_project_kernel");
}

extern "C" int sq_lift_rows(const uint8_t *d_rows, int32_t R, int32_t L, const int32_t *d_short, int64_t short_len, const int64_t *d_start,
                            const int32_t *d_stride, const int32_t *d_nstruct, int32_t K, int32_t Lmax, int32_t *d_length,
                            int32_t *d_col_of, int32_t *d_pos_of, int32_t *d_partner, int32_t *d_status, void *hip_stream)
{
    if (!d_rows || !d_short || short_len < 1 || !d_start || !d_stride || !d_nstruct || !d_length || !d_col_of || !d_pos_of ||
        !d_partner || !d_status || !sizes_ok(R, L, K, Lmax)) {
        sq_set_error("sq_lift_rows: bad argument");
        return -1;
    }
    const dim3 grid((unsigned)std::min<int32_t>(R, SQ_PROJ_MAX_BLOCKS)), block(SQ_PROJ_THREADS);
    hipLaunchKernelGGL(sq_lift_kernel, grid, block, 0, (hipStream_t)hip_stream, d_rows, R, L, d_short, short_len, d_start, d_stride,
                       d_nstruct, K, Lmax, d_length, d_col_of, d_pos_of, d_partner, d_status);
    return sq_check(hipGetLastError(), "sq_lift_kernel");
}
