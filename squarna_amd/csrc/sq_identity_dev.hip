// Row identities of an alignment (RowIdentity): all-pairs identity of the rows, the rows within a threshold of every row and
// the greedy redundancy filter, on the device.  Counts, layout and predicates: sq_identity.h.
//
//   sq_identity_planes_kernel   the ASCII rows as four bit planes (two code bits, base, residue) of 64 columns per word, the
//                               row fastest; len and bases of every row
//   sq_identity_pairs_kernel    same / both of every pair of rows, tile by tile from LDS with the counters in registers; the
//                               R x R matrices when the caller wants them, the neighbour bit matrix, the neighbour counts
//   sq_identity_filter_kernel   the greedy filter over the bit matrix, as one wave
//
// The three are launched one after the other on the caller's stream: a phase that needs another's results is a launch of
// its own, and no block waits for another.  All buffers are the caller's device memory; nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_identity.h"

// One block per 64 rows x 64 columns of the alignment.  A wave reads 64 contiguous bytes of a row (a row of rows[] starts at
// r * L, aligned to nothing: bytes, not words) with lane = column, and a plane's word of the row is the wave's ballot of
// "my byte sets the plane": every wave takes 16 of the block's rows.  Rows >= R and columns >= L set no plane.  The popcounts
// of the residue and base words are added to len and bases (cleared before the launch; integer sums, whatever the order).
// The 4 x 64 words leave 64 consecutive rows at a time.
extern "C" __global__ __launch_bounds__(256) void sq_identity_planes_kernel(const uint8_t *rows, int32_t R, int32_t L, uint64_t *plane,
                                                                           int32_t *len, int32_t *bases)
{
    __shared__ uint64_t s_word[SQ_ID_PLANES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t Wc = SqIdentity::col_words(L), Rpad = SqIdentity::rpad(R);
    const int64_t cw = blockIdx.x % Wc, r0 = blockIdx.x / Wc * 64;    // (block-uniform: the grid has Rpad / 64 * Wc blocks)
    const int64_t c = cw * 64 + lane;
    for (int k = wave; k < 64; k += 4) {
        const int64_t r = r0 + k;
        const uint32_t bits = r < R && c < L ? SqIdentity::plane_bits(SqCovar::cls(rows[r * L + c])) : 0u;
        unsigned long long m[SQ_ID_PLANES];
        for (int p = 0; p < SQ_ID_PLANES; p++) m[p] = __ballot(bits >> p & 1u);
        if (lane < SQ_ID_PLANES) s_word[lane][k] = lane == 0 ? m[0] : lane == 1 ? m[1] : lane == 2 ? m[2] : m[3];
        if (lane == 0 && r < R) {
            if (m[SQ_ID_RES]) atomicAdd(&len[r], __popcll(m[SQ_ID_RES]));
            if (m[SQ_ID_BASE]) atomicAdd(&bases[r], __popcll(m[SQ_ID_BASE]));
        }
    }
    __syncthreads();
    plane[SqIdentity::at(wave, cw, r0 + lane, Wc, Rpad)] = s_word[wave][lane];   // (256 threads = 4 planes x 64 rows; r0 + lane < Rpad)
}

// All pairs of rows.  A block takes the upper-triangle tiles k = blockIdx.x, + gridDim.x, ... (SqIdentity::tile_of) of 64 x 64
// cells: rows a in tile ta, rows b in tile tb.  Thread t has the sixteen cells b = t % 64, a = 16 * (t / 64) .. + 15: the lanes
// of a wave read 64 consecutive words of the b planes, and the whole wave reads the same word of the a planes (a
// broadcast).  Per SQ_ID_WORD_CHUNK words of columns the planes of both row ranges are loaded into LDS, 64 consecutive words
// of global memory at a time, and every thread adds two popcounts per cell and word to its 32 counters, which stay in
// registers over the whole of L.  Every trip count is block-uniform: words beyond Wc are staged as zero, rows beyond R have
// all-zero planes and are never neighbours.
// At the end of a tile: the two counters go to the R x R matrices when the caller gave them (and to the mirror cell when
// the tile lies off the diagonal); the neighbour word of (row a, the 64 rows of tile tb) is one ballot and one 8-byte store;
// the word of (row b, the 64 rows of tile ta) is put together from the waves' 16-bit pieces in LDS.  Every word of the bit
// matrix is written by exactly one tile.  neighbours[] (cleared before the launch) gets the popcounts, and 1 for the row
// itself from its diagonal tile.
extern "C" __global__ __launch_bounds__(256) void sq_identity_pairs_kernel(const uint64_t *plane, int32_t R, int32_t L, int32_t kind,
                                                                          int32_t T, const int32_t *len, int32_t *same_out,
                                                                          int32_t *both_out, uint64_t *nbr, int32_t *neighbours)
{
    constexpr int TL = SQ_ID_TILE, CH = SQ_ID_WORD_CHUNK, CELLS = 16;
    static_assert(TL == 64 && CELLS * 4 == TL, "sixteen cells per thread of a 256-thread block, a wave per 16 rows a");
    __shared__ uint64_t s_a[SQ_ID_PLANES][CH][TL], s_b[SQ_ID_PLANES][CH][TL];
    __shared__ uint16_t s_mirror[TL][4];                             // [row b][wave]: the neighbour bits of the wave's 16 rows a
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, al = wave * CELLS;
    const int64_t Wc = SqIdentity::col_words(L), Rpad = SqIdentity::rpad(R), Wr = SqIdentity::row_words(R);
    const int64_t nT = SqIdentity::tiles(R), ntiles = SqIdentity::tile_count(nT);
    for (int64_t k = blockIdx.x; k < ntiles; k += gridDim.x) {
        int32_t ta, tb;
        SqIdentity::tile_of(k, nT, ta, tb);
        const int64_t a0 = (int64_t)ta * TL, b0 = (int64_t)tb * TL;  // (a0 + 63, b0 + 63 < Rpad)
        int32_t same[CELLS] = {}, both[CELLS] = {};
        for (int64_t wb = 0; wb < Wc; wb += CH) {
            __syncthreads();                                         // (the last chunk, and the last tile's mirror, have been read)
            for (int i = tid; i < SQ_ID_PLANES * CH * TL; i += 256) {
                const int p = i / (CH * TL), wd = i / TL % CH, r = i % TL;
                const bool have = wb + wd < Wc;
                s_a[p][wd][r] = have ? plane[SqIdentity::at(p, wb + wd, a0 + r, Wc, Rpad)] : 0ull;
                s_b[p][wd][r] = have ? plane[SqIdentity::at(p, wb + wd, b0 + r, Wc, Rpad)] : 0ull;
            }
            __syncthreads();
#pragma unroll 1
            for (int wd = 0; wd < CH; wd++) {
                uint64_t b[SQ_ID_PLANES];
                for (int p = 0; p < SQ_ID_PLANES; p++) b[p] = s_b[p][wd][lane];
#pragma unroll
                for (int c = 0; c < CELLS; c++) {
                    uint64_t a[SQ_ID_PLANES];
                    for (int p = 0; p < SQ_ID_PLANES; p++) a[p] = s_a[p][wd][al + c];
                    SqIdentity::accumulate(a, b, same[c], both[c]);
                }
            }
        }
        const int64_t b = b0 + lane;
        const int32_t len_b = b < R ? len[b] : 0;
        uint32_t mine = 0;                                           // bit c: my row b is a neighbour of row a0 + al + c
#pragma unroll
        for (int c = 0; c < CELLS; c++) {
            const int64_t a = a0 + al + c;                           // (wave-uniform)
            const int32_t len_a = a < R ? len[a] : 0;
            const bool near = SqIdentity::neighbours(a, b, R, same[c], both[c], len_a, len_b, L, kind, T);
            const unsigned long long word = __ballot(near);
            mine |= (uint32_t)near << c;
            if (a < R) {
                if (lane == 0) {
                    nbr[a * Wr + tb] = word;
                    const int n = __popcll(word) + (ta == tb);
                    if (n) atomicAdd(&neighbours[a], n);
                }
                if (same_out && b < R) {
                    same_out[a * R + b] = same[c];
                    both_out[a * R + b] = both[c];
                    if (ta != tb) {
                        same_out[b * R + a] = same[c];
                        both_out[b * R + a] = both[c];
                    }
                }
            }
        }
        if (ta != tb) {                                              // (block-uniform)
            s_mirror[lane][wave] = (uint16_t)mine;
            __syncthreads();
            const int64_t row = b0 + tid;
            if (tid < TL && row < R) {
                const uint64_t word = (uint64_t)s_mirror[tid][0] | (uint64_t)s_mirror[tid][1] << 16 | (uint64_t)s_mirror[tid][2] << 32 |
                                      (uint64_t)s_mirror[tid][3] << 48;
                nbr[row * Wr + ta] = word;
                if (word) atomicAdd(&neighbours[row], __popcll(word));
            }
        }
    }
}

// The greedy filter, one wave: the rows in their order, row a kept iff kept & nbr[a] is empty over the words that hold the
// rows below a.  The lanes take the words of row a: lane l has the words l, l + 64, ... of the row, NW <= 16 of them.  The kept
// mask lives in LDS, where lane 0 sets a kept row's bit with an LDS atomic that returns nothing; lane l also mirrors its words
// of the mask in registers, so that the test of a row is NW ANDs and one vote, with no trip to memory on the chain from one
// row's verdict to the next.
// The words of a row do not depend on the verdicts, so they are loaded far ahead: a lane holds SQ_ID_FILTER_WORDS = 64 words in
// K groups of G rows of NW words, a ring.  The rows of a group are judged, then the group's registers take the loads of the
// rows K groups further on, and the other K - 1 groups' loads are in flight behind them (a first form that waited for eight
// rows' loads at a time before judging them spent the load latency once per eight rows: 0.2 us a row, and 0.74 us a row
// beyond 4096 rows, where it read the words from 64 on when their row's turn came).  Words at or above words_below(a) are
// not loaded: they read as zero.  Every loop is bounded by R.  keep[] leaves at the end, 64 rows at a time.
template <int NW, int G>
__global__ __launch_bounds__(64) void sq_identity_filter_kernel(const uint64_t *nbr, int32_t R, uint8_t *keep)
{
    constexpr int K = SQ_ID_FILTER_WORDS / (NW * G);
    static_assert(K >= 2 && K * G * NW == SQ_ID_FILTER_WORDS, "a ring of K groups of G rows of NW words");
    __shared__ unsigned long long s_kept[(SQ_ID_MAX_ROWS + 63) / 64];
    const int lane = threadIdx.x;
    const int64_t Wr = SqIdentity::row_words(R);                      // (<= 64 NW: the launch chooses NW so)
    for (int64_t w = lane; w < Wr; w += 64) s_kept[w] = 0ull;
    __syncthreads();
    // Every load is unconditional, from a clamped address inside the bit matrix (a branch around a load made the compiler
    // wait for all loads at once).  No word needs masking: the words of a row at or above words_below(a) meet kept bits that
    // are still zero, a lane whose word index is clamped (>= Wr) never sets a bit of `mine`, and a row >= R is not judged.
    auto load = [&](int64_t a, int j) {
        const int64_t w = (int64_t)j * 64 + lane;
        return nbr[(a < R ? a : R - 1) * Wr + (w < Wr ? w : Wr - 1)];
    };
    uint64_t mine[NW] = {}, ring[K][G][NW];
#pragma unroll
    for (int q = 0; q < K; q++)
#pragma unroll
        for (int i = 0; i < G; i++)
#pragma unroll
            for (int j = 0; j < NW; j++) ring[q][i][j] = load(q * G + i, j);
    for (int64_t a0 = 0; a0 < R; a0 += K * G) {
#pragma unroll
        for (int q = 0; q < K; q++) {
#pragma unroll
            for (int i = 0; i < G; i++) {
                const int64_t a = a0 + q * G + i;
                bool hit = false;
#pragma unroll
                for (int j = 0; j < NW; j++) hit |= SqIdentity::word_hits(mine[j], ring[q][i][j]);
                const bool kept = !__any(hit) && a < R;              // (wave-uniform)
                const uint64_t bit = kept ? SqIdentity::row_bit(a) : 0ull;
                const int64_t w = a / 64;
                if (kept && lane == 0) atomicOr(&s_kept[w], (unsigned long long)bit);
#pragma unroll
                for (int j = 0; j < NW; j++) mine[j] |= w == (int64_t)j * 64 + lane ? bit : 0ull;
            }
#pragma unroll
            for (int i = 0; i < G; i++)
#pragma unroll
                for (int j = 0; j < NW; j++) ring[q][i][j] = load(a0 + (int64_t)(K + q) * G + i, j);
        }
    }
    __syncthreads();
    for (int64_t r = lane; r < R; r += 64) keep[r] = (uint8_t)(s_kept[r / 64] >> (r % 64) & 1ull);
}

// The filter kernel for R rows: the fewest words per lane that hold a row's ceil(R / 64) words, a power of two.
static void launch_filter(const uint64_t *nbr, int32_t R, uint8_t *keep, hipStream_t st)
{
    static_assert(16 * 64 * 64 >= SQ_ID_MAX_ROWS, "sixteen words per lane hold the longest row of the bit matrix");
    const int64_t Wr = SqIdentity::row_words(R);
    if (Wr <= 64) hipLaunchKernelGGL((sq_identity_filter_kernel<1, 8>), dim3(1), dim3(64), 0, st, nbr, R, keep);
    else if (Wr <= 128) hipLaunchKernelGGL((sq_identity_filter_kernel<2, 4>), dim3(1), dim3(64), 0, st, nbr, R, keep);
    else if (Wr <= 256) hipLaunchKernelGGL((sq_identity_filter_kernel<4, 2>), dim3(1), dim3(64), 0, st, nbr, R, keep);
    else if (Wr <= 512) hipLaunchKernelGGL((sq_identity_filter_kernel<8, 1>), dim3(1), dim3(64), 0, st, nbr, R, keep);
    else hipLaunchKernelGGL((sq_identity_filter_kernel<16, 1>), dim3(1), dim3(64), 0, st, nbr, R, keep);   // (SQ_ID_MAX_ROWS: 1024 words)
}

extern "C" size_t sq_row_identity_scratch(int32_t R, int32_t L)
{
    if (R < 1 || L < 1 || R > SQ_ID_MAX_ROWS || L > SQ_ID_MAX_COLS) return 0;
    return (size_t)(SqIdentity::plane_words(R, L) + SqIdentity::nbr_words(R)) * sizeof(uint64_t);
}

// The checks, and the kernels of `phases` (bit 0: the planes with len and bases, bit 1: the pairs, bit 2: the filter).
static int row_identity(const char *who, int32_t phases, const uint8_t *d_rows, int32_t R, int32_t L, int32_t denominator,
                        int32_t threshold_bp, void *d_scratch, size_t scratch_bytes, int32_t *d_len, int32_t *d_bases, int32_t *d_same,
                        int32_t *d_both, int32_t *d_neighbours, uint8_t *d_keep, uint64_t *d_out, hipStream_t st)
{
    if (!d_rows || !d_scratch || !d_len || !d_bases || !d_neighbours || !d_keep || !d_out || R < 1 || L < 1 || R > SQ_ID_MAX_ROWS ||
        L > SQ_ID_MAX_COLS || denominator < 0 || denominator >= SQ_ID_DENS || threshold_bp < 0 || threshold_bp > 10000 ||
        !d_same != !d_both || phases < 1 || phases > 7) {
        sq_set_error(std::string(who) + ": bad argument");
        return -1;
    }
    if (scratch_bytes < sq_row_identity_scratch(R, L)) {
        sq_set_error(std::string(who) + ": scratch too small");
        return -1;
    }
    uint64_t *plane = (uint64_t *)d_scratch, *nbr = plane + SqIdentity::plane_words(R, L);
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    if (phases & 1) {
        HIPCK(hipMemsetAsync(d_len, 0, sizeof(int32_t) * (size_t)R, st));
        HIPCK(hipMemsetAsync(d_bases, 0, sizeof(int32_t) * (size_t)R, st));
        // (at most 1024 words of rows x 32768 words of columns: the grid stays below 2^31)
        const unsigned blocks = (unsigned)(SqIdentity::row_words(R) * SqIdentity::col_words(L));
        hipLaunchKernelGGL(sq_identity_planes_kernel, dim3(blocks), dim3(256), 0, st, d_rows, R, L, plane, d_len, d_bases);
        if (int rc = sq_check(hipGetLastError(), "sq_identity_planes_kernel")) return rc;
    }
    if (phases & 2) {
        HIPCK(hipMemsetAsync(d_neighbours, 0, sizeof(int32_t) * (size_t)R, st));
        // At most SQ_ID_MAX_BLOCKS = 2048 blocks, the rest by grid stride: the kernel's 107 VGPRs admit four blocks of 4 waves
        // on each of the 256 CUs (its 16.5 KB of LDS would admit nine), so 2048 blocks are twice what the chip holds at once
        // and a larger grid would only queue behind them.
        const unsigned blocks = (unsigned)std::min<int64_t>(SqIdentity::tile_count(SqIdentity::tiles(R)), SQ_ID_MAX_BLOCKS);
        hipLaunchKernelGGL(sq_identity_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)plane, R, L, denominator,
                           threshold_bp, (const int32_t *)d_len, d_same, d_both, nbr, d_neighbours);
        if (int rc = sq_check(hipGetLastError(), "sq_identity_pairs_kernel")) return rc;
    }
    if (phases & 4) {
        launch_filter(nbr, R, d_keep, st);
        if (int rc = sq_check(hipGetLastError(), "sq_identity_filter_kernel")) return rc;
    }
    return 0;
}

extern "C" int sq_row_identity(const uint8_t *d_rows, int32_t R, int32_t L, int32_t denominator, int32_t threshold_bp, void *d_scratch,
                               size_t scratch_bytes, int32_t *d_len, int32_t *d_bases, int32_t *d_same, int32_t *d_both,
                               int32_t *d_neighbours, uint8_t *d_keep, uint64_t *d_out, void *hip_stream)
{
    return row_identity("sq_row_identity", 7, d_rows, R, L, denominator, threshold_bp, d_scratch, scratch_bytes, d_len, d_bases, d_same, d_both,
                        d_neighbours, d_keep, d_out, (hipStream_t)hip_stream);
}

extern "C" int sq_row_identity_phases(int32_t phases, const uint8_t *d_rows, int32_t R, int32_t L, int32_t denominator, int32_t threshold_bp,
                                      void *d_scratch, size_t scratch_bytes, int32_t *d_len, int32_t *d_bases, int32_t *d_same,
                                      int32_t *d_both, int32_t *d_neighbours, uint8_t *d_keep, uint64_t *d_out, void *hip_stream)
{
    return row_identity("sq_row_identity_phases", phases, d_rows, R, L, denominator, threshold_bp, d_scratch, scratch_bytes, d_len, d_bases,
                        d_same, d_both, d_neighbours, d_keep, d_out, (hipStream_t)hip_stream);
}
