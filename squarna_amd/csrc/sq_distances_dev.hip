// Base-pair distances of structures (Distances): the pairs every two structures of a group share, the structures within a
// radius of every structure and the greedy filter in row order with its leaders, on the device.  Counts, layout, tile plan
// and predicates: sq_distances.h.
//
//   sq_distances_planes_kernel   the partner rows as bit planes (`open` and the bits of the span) of 64 columns per word, the
//                                row fastest; status and npairs of every row
//   sq_distances_pairs_kernel    common of every pair of rows of the planned tiles, from LDS with the counters in registers;
//                                the block-diagonal matrix when the caller wants it, the neighbour bit matrix, the counts
//   sq_distances_filter_kernel   the greedy filter over the bit matrix with the leaders, one wave per group
//
// The three are launched one after the other on the caller's stream: a phase that needs another's results is a launch of
// its own, and no block waits for another.  All buffers are the caller's device memory; nothing is allocated or waited for.
#include "sq_host_int.h"
#include "sq_distances.h"

// One block per 64 rows, a wave per 16 of them.  Row q is read at partner[row_start[q] ..] with row_width[q] columns, lane =
// column.  A first pass judges the row (a row whose place in partner[] is not inside it is invalid and is not read) and
// counts its opening columns; a second pass forms the words of all planes, one word of columns at a time, as the wave's
// ballots of "my column sets the plane", and the np x 64 words leave 64 consecutive rows at a time.  An invalid row, a row
// >= S and the columns beyond a row's width set no plane.
extern "C" __global__ __launch_bounds__(256) void sq_distances_planes_kernel(const int32_t *partner, int64_t partner_len,
                                                                            const int64_t *row_start, const int32_t *row_width, int32_t S,
                                                                            int32_t Wmax, uint64_t *plane, int32_t *status, int32_t *npairs)
{
    __shared__ uint64_t s_word[SQ_DIST_MAX_PLANES][64];
    __shared__ int64_t s_start[64];
    __shared__ int32_t s_width[64];                                  // (0 for a row that sets no plane)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t Wc = SqDistances::col_words(Wmax), Spad = SqDistances::spad(S), r0 = (int64_t)blockIdx.x * 64;
    const int np = SqDistances::planes(Wmax);
    for (int k = wave; k < 64; k += 4) {
        const int64_t q = r0 + k;                                    // (wave-uniform)
        int64_t start = 0;
        int32_t width = 0, n = 0;
        bool bad = false;
        if (q < S) {
            start = row_start[q];
            width = row_width[q];
            bad = start < 0 || width < 0 || width > Wmax || start > partner_len - width;
            for (int32_t c0 = 0; !bad && c0 < width; c0 += 64) {
                const int32_t c = c0 + lane;
                const int32_t p = c < width ? partner[start + c] : -1;
                const int32_t back = p >= 0 && SqDistances::partner_in_range(p, width) ? partner[start + p] : c;
                bad = __any(c < width && SqDistances::column_bad(c, p, back, width));
                n += __popcll(__ballot(p > c));
            }
            if (lane == 0) {
                status[q] = bad;
                npairs[q] = bad ? 0 : n;
            }
        }
        if (lane == 0) {
            s_start[k] = start;
            s_width[k] = bad ? 0 : width;
        }
    }
    __syncthreads();
    for (int64_t cw = 0; cw < Wc; cw++) {                            // (block-uniform)
        for (int k = wave; k < 64; k += 4) {
            const int32_t c = (int32_t)(cw * 64) + lane;
            const uint32_t bits = c < s_width[k] ? SqDistances::plane_bits(c, partner[s_start[k] + c]) : 0u;
            for (int p = 0; p < np; p++) {
                const unsigned long long m = __ballot(bits >> p & 1u);
                if (lane == p) s_word[p][k] = m;
            }
        }
        __syncthreads();
        for (int i = tid; i < np * 64; i += 256) plane[SqIdentity::at(i / 64, cw, r0 + i % 64, Wc, Spad)] = s_word[i / 64][i % 64];   // (r0 + 63 < Spad)
        __syncthreads();
    }
}

// All pairs of rows of the planned tiles.  A block takes the entries k = blockIdx.x, + gridDim.x, ... of tiles[T][2]: rows a in
// tile ta, rows b in tile tb, 64 x 64 cells.  Thread t has the sixteen cells b = t % 64, a = 16 * (t / 64) .. + 15, as in
// sq_identity_pairs_kernel: the lanes of a wave read 64 consecutive words of the b planes, and the whole wave reads the same
// word of the a planes.  Per SQ_DIST_WORD_CHUNK words of columns the np planes of both row ranges are loaded into LDS; per word a
// thread starts its sixteen masks from the `open` planes and narrows them plane after plane, and adds their popcounts to
// its sixteen counters, which stay in registers over the whole width.  Every trip count is block-uniform: words beyond Wc
// are staged as zero.
// At the end of a tile a cell is a pair of neighbours only between two different valid rows < S of one group.  common goes to
// the block-diagonal matrix when the caller gave one (cells: its size), and to the mirror cell off the diagonal; a cell of
// two groups, of a row >= S or of an invalid row is never written, nor is one whose address the offsets put outside the
// matrix.  The neighbour word of (row a, the 64 rows of tile tb) is one ballot and one 8-byte store; the word of (row b, the
// 64 rows of tile ta) is put together from the waves' 16-bit pieces in LDS.  neighbours[] (cleared before the launch) gets
// the popcounts, and 1 for a valid row itself from its diagonal tile.  An entry of tiles[] outside the tile range is skipped
// and sets SQ_DIST_BAD_TILE in the status word.
extern "C" __global__ __launch_bounds__(256) void sq_distances_pairs_kernel(const uint64_t *plane, int32_t S, int32_t Wmax,
                                                                           const int32_t *row_group, const int32_t *group_off,
                                                                           const int64_t *mat_off, int32_t G, const int32_t *tiles, int32_t T,
                                                                           int32_t mode, int32_t threshold, const int32_t *status,
                                                                           const int32_t *npairs, int32_t *common_out, int64_t cells,
                                                                           uint64_t *nbr, int32_t *neighbours, unsigned long long *out)
{
    constexpr int TL = SQ_DIST_TILE, CH = SQ_DIST_WORD_CHUNK, CELLS = 16;
    static_assert(TL == 64 && CELLS * 4 == TL, "sixteen cells per thread of a 256-thread block, a wave per 16 rows a");
    static_assert(2 * SQ_DIST_MAX_PLANES * CH * TL * 8 + TL * 4 * 2 <= 65536, "static LDS within 64 KB at 16 planes");
    __shared__ uint64_t s_a[SQ_DIST_MAX_PLANES * CH * TL], s_b[SQ_DIST_MAX_PLANES * CH * TL];   // [plane][word][row]
    __shared__ uint16_t s_mirror[TL][4];                             // [row b][wave]: the neighbour bits of the wave's 16 rows a
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, al = wave * CELLS;
    const int np = SqDistances::planes(Wmax);
    const int64_t Wc = SqDistances::col_words(Wmax), Spad = SqDistances::spad(S), Wr = SqDistances::row_words(S), nT = SqDistances::tiles(S);
    for (int64_t k = blockIdx.x; k < T; k += gridDim.x) {
        const int32_t ta = tiles[2 * k], tb = tiles[2 * k + 1];
        if (!SqDistances::tile_in_range(ta, tb, nT)) {               // (block-uniform)
            if (tid == 0) atomicOr(out + 1, (unsigned long long)SQ_DIST_BAD_TILE);
            continue;
        }
        const int64_t a0 = (int64_t)ta * TL, b0 = (int64_t)tb * TL;  // (a0 + 63, b0 + 63 < Spad)
        int32_t common[CELLS] = {};
        for (int64_t wb = 0; wb < Wc; wb += CH) {
            __syncthreads();                                         // (the last chunk, and the last tile's mirror, have been read)
            for (int i = tid; i < np * CH * TL; i += 256) {
                const int p = i / (CH * TL), wd = i / TL % CH, r = i % TL;
                const bool have = wb + wd < Wc;
                s_a[i] = have ? plane[SqIdentity::at(p, wb + wd, a0 + r, Wc, Spad)] : 0ull;
                s_b[i] = have ? plane[SqIdentity::at(p, wb + wd, b0 + r, Wc, Spad)] : 0ull;
            }
            __syncthreads();
#pragma unroll 1
            for (int wd = 0; wd < CH; wd++) {
                const uint64_t open_b = s_b[wd * TL + lane];
                uint64_t m[CELLS];
#pragma unroll
                for (int c = 0; c < CELLS; c++) m[c] = s_a[wd * TL + al + c] & open_b;
#pragma unroll 1
                for (int p = SQ_DIST_SPAN0; p < np; p++) {
                    const uint64_t b = s_b[(p * CH + wd) * TL + lane];
#pragma unroll
                    for (int c = 0; c < CELLS; c++) m[c] &= ~(s_a[(p * CH + wd) * TL + al + c] ^ b);
                }
#pragma unroll
                for (int c = 0; c < CELLS; c++) common[c] += __popcll(m[c]);
            }
        }
        // my row b: its group, where the group's cells lie, and whether they lie inside the matrix
        const int64_t b = b0 + lane;
        int32_t gb = -1, nb = 0;
        bool valid_b = false, cells_b = false;
        int64_t first = 0, n_g = 0, off = 0;
        if (b < S) {
            gb = row_group[b];
            nb = npairs[b];
            valid_b = status[b] == 0;
            if (gb < 0 || gb >= G) gb = -1;
            if (gb >= 0) {
                first = group_off[gb];
                n_g = (int64_t)group_off[gb + 1] - first;
                off = mat_off[gb];
                cells_b = common_out && valid_b && first >= 0 && b >= first && b - first < n_g && off >= 0 && off <= cells && n_g * n_g <= cells - off;
            }
        }
        uint32_t mine = 0;                                           // bit c: my row b is a neighbour of row a0 + al + c
#pragma unroll
        for (int c = 0; c < CELLS; c++) {
            const int64_t a = a0 + al + c;                           // (wave-uniform)
            int32_t ga = -1, na = 0;
            bool valid_a = false;
            if (a < S) {
                ga = row_group[a];
                na = npairs[a];
                valid_a = status[a] == 0;
                if (ga < 0 || ga >= G) ga = -1;
            }
            const bool near = SqDistances::neighbours(a, b, ga, gb, valid_a, valid_b, mode, threshold, na, nb, common[c]);
            const unsigned long long word = __ballot(near);
            mine |= (uint32_t)near << c;
            if (a < S) {
                if (lane == 0) {
                    nbr[a * Wr + tb] = word;
                    const int n = __popcll(word) + (ta == tb && valid_a);
                    if (n) atomicAdd(&neighbours[a], n);
                }
                if (cells_b && ga == gb && valid_a && a >= first && a - first < n_g) {
                    common_out[SqDistances::cell(off, first, n_g, a, b)] = common[c];
                    if (ta != tb) common_out[SqDistances::cell(off, first, n_g, b, a)] = common[c];
                }
            }
        }
        if (ta != tb) {                                              // (block-uniform)
            s_mirror[lane][wave] = (uint16_t)mine;
            __syncthreads();
            const int64_t row = b0 + tid;
            if (tid < TL && row < S) {
                const uint64_t word = (uint64_t)s_mirror[tid][0] | (uint64_t)s_mirror[tid][1] << 16 | (uint64_t)s_mirror[tid][2] << 32 |
                                      (uint64_t)s_mirror[tid][3] << 48;
                nbr[row * Wr + ta] = word;
                if (word) atomicAdd(&neighbours[row], __popcll(word));
            }
        }
    }
}

// The greedy filter, one wave per group, the groups g = blockIdx.x, + gridDim.x, ...: the rows first .. last - 1 of the group in
// their order, row a kept iff kept & nbr[a] is empty over the words w0 = first / 64 .. a / 64.  As in sq_identity_filter_kernel
// the lanes take the words of a row -- lane l has the words w0 + l, w0 + l + 64, ... of it, NW <= 16 of them --, the kept mask
// lives in LDS (word 0 = word w0 of the rows) and every lane mirrors its words of it in registers, so that the test of a row
// is NW ANDs and one vote; the words of the rows ahead are loaded into a ring of K groups of GR rows, SQ_DIST_FILTER_WORDS
// words a lane, while the rows before them are judged.  Every load is unconditional, from a clamped address inside the bit
// matrix.  No word needs masking: a word of row a above a / 64 (which no planned tile may have written) meets kept bits that
// are still zero, the bits of another group's rows in word w0 are never set in either mask, and a lane whose word index
// is clamped never sets a bit of `mine`.
// A dropped row's leader leaves at its verdict: the lowest word with a hit belongs to the first lane of the first vote that
// has one, and that lane stores the row of its lowest common bit.  keep[] and the leaders of the kept rows leave at the end,
// where a kept row that is invalid (it has no neighbour bit, so the chain kept it, and protects nobody) gets keep 0 and
// leader -1.  A group whose offsets are not 0 <= first <= last <= S, or that spans more than 64 NW words, is left alone and
// sets SQ_DIST_BAD_GROUP in the status word.
template <int NW, int GR>
__global__ __launch_bounds__(64) void sq_distances_filter_kernel(const uint64_t *nbr, int32_t S, const int32_t *group_off, int32_t G,
                                                                 const int32_t *status, uint8_t *keep, int32_t *leader, unsigned long long *out)
{
    constexpr int K = SQ_DIST_FILTER_WORDS / (NW * GR);
    static_assert(K >= 2 && K * GR * NW == SQ_DIST_FILTER_WORDS, "a ring of K groups of GR rows of NW words");
    __shared__ unsigned long long s_kept[(SQ_DIST_MAX_ROWS + 63) / 64];
    const int lane = threadIdx.x;
    const int64_t Wr = SqDistances::row_words(S);
    for (int32_t g = blockIdx.x; g < G; g += gridDim.x) {
        const int64_t first = group_off[g], last = group_off[g + 1];
        const int64_t w0 = SqDistances::first_word(first), words = SqDistances::group_words(first, last);
        if (first < 0 || last < first || last > S || words > (int64_t)NW * 64) {   // (wave-uniform)
            if (lane == 0) atomicOr(out + 1, (unsigned long long)SQ_DIST_BAD_GROUP);
            continue;
        }
        if (last == first) continue;
        __syncthreads();                                             // (the last group's mask has been read)
        for (int64_t w = lane; w < words; w += 64) s_kept[w] = 0ull;
        __syncthreads();
        auto load = [&](int64_t a, int j) {
            const int64_t w = w0 + (int64_t)j * 64 + lane;
            return nbr[(a < last ? a : last - 1) * Wr + (w < Wr ? w : Wr - 1)];
        };
        uint64_t mine[NW] = {}, ring[K][GR][NW];
#pragma unroll
        for (int q = 0; q < K; q++)
#pragma unroll
            for (int i = 0; i < GR; i++)
#pragma unroll
                for (int j = 0; j < NW; j++) ring[q][i][j] = load(first + q * GR + i, j);
        for (int64_t a0 = first; a0 < last; a0 += K * GR) {
#pragma unroll
            for (int q = 0; q < K; q++) {
#pragma unroll
                for (int i = 0; i < GR; i++) {
                    const int64_t a = a0 + q * GR + i;
                    bool hit = false;
#pragma unroll
                    for (int j = 0; j < NW; j++) hit |= SqIdentity::word_hits(mine[j], ring[q][i][j]);
                    const bool dropped = __any(hit) && a < last;     // (wave-uniform)
                    const bool kept = !dropped && a < last;
                    if (dropped) {
                        bool done = false;
#pragma unroll
                        for (int j = 0; j < NW; j++) {
                            const unsigned long long v = done ? 0ull : __ballot(SqIdentity::word_hits(mine[j], ring[q][i][j]));
                            if (v) {
                                if (lane == __builtin_ctzll(v))
                                    leader[a] = (int32_t)SqDistances::lowest_hit(w0 + (int64_t)j * 64 + lane, mine[j], ring[q][i][j]);
                                done = true;
                            }
                        }
                    }
                    const uint64_t bit = kept ? SqIdentity::row_bit(a) : 0ull;
                    const int64_t w = a / 64 - w0;
                    if (kept && lane == 0) atomicOr(&s_kept[w], (unsigned long long)bit);
#pragma unroll
                    for (int j = 0; j < NW; j++) mine[j] |= w == (int64_t)j * 64 + lane ? bit : 0ull;
                }
#pragma unroll
                for (int i = 0; i < GR; i++)
#pragma unroll
                    for (int j = 0; j < NW; j++) ring[q][i][j] = load(a0 + (int64_t)(K + q) * GR + i, j);
            }
        }
        __syncthreads();
        for (int64_t r = first + lane; r < last; r += 64) {
            const bool kept = s_kept[r / 64 - w0] >> (r % 64) & 1ull, valid = status[r] == 0;
            keep[r] = (uint8_t)(kept && valid);
            if (kept) leader[r] = valid ? (int32_t)r : -1;
        }
    }
}

// The filter kernel for groups of at most max_group_rows rows among S: the fewest words per lane that hold the words such a
// group can span (it may begin anywhere in its first word), a power of two.
static void launch_filter(const uint64_t *nbr, int32_t S, const int32_t *group_off, int32_t G, int32_t max_group_rows, const int32_t *status,
                          uint8_t *keep, int32_t *leader, unsigned long long *out, hipStream_t st)
{
    static_assert(16 * 64 * 64 >= SQ_DIST_MAX_ROWS, "sixteen words per lane hold the longest row of the bit matrix");
    const int64_t words = std::min<int64_t>(((int64_t)max_group_rows + 62) / 64 + 1, SqDistances::row_words(S));
    const dim3 grid((unsigned)std::min<int32_t>(G, SQ_DIST_MAX_BLOCKS)), block(64);
    if (words <= 64) hipLaunchKernelGGL((sq_distances_filter_kernel<1, 8>), grid, block, 0, st, nbr, S, group_off, G, status, keep, leader, out);
    else if (words <= 128) hipLaunchKernelGGL((sq_distances_filter_kernel<2, 4>), grid, block, 0, st, nbr, S, group_off, G, status, keep, leader, out);
    else if (words <= 256) hipLaunchKernelGGL((sq_distances_filter_kernel<4, 2>), grid, block, 0, st, nbr, S, group_off, G, status, keep, leader, out);
    else if (words <= 512) hipLaunchKernelGGL((sq_distances_filter_kernel<8, 1>), grid, block, 0, st, nbr, S, group_off, G, status, keep, leader, out);
    else hipLaunchKernelGGL((sq_distances_filter_kernel<16, 1>), grid, block, 0, st, nbr, S, group_off, G, status, keep, leader, out);
}

// (T, the planned tiles, is checked against the tile range; the plan itself adds nothing to the scratch)
extern "C" size_t sq_structure_distances_scratch(int32_t S, int32_t Wmax, int32_t T)
{
    if (S < 1 || Wmax < 1 || S > SQ_DIST_MAX_ROWS || Wmax > SQ_DIST_MAX_COLS || T < 0 ||
        T > SqIdentity::tile_count(SqDistances::tiles(S)))
        return 0;
    return (size_t)SqDistances::scratch_words(S, Wmax) * sizeof(uint64_t);
}

// The checks, and the kernels of `phases` (bit 0: the planes with status and npairs, bit 1: the pairs, bit 2: the filter).
static int structure_distances(const char *who, int32_t phases, const int32_t *d_partner, int64_t partner_len, const int64_t *d_row_start,
                               const int32_t *d_row_width, const int32_t *d_row_group, int32_t S, int32_t Wmax, const int32_t *d_group_off,
                               const int64_t *d_mat_off, int32_t G, int32_t max_group_rows, const int32_t *d_tiles, int32_t T, int32_t mode,
                               int32_t threshold, void *d_scratch, size_t scratch_bytes, int32_t *d_status, int32_t *d_npairs,
                               int32_t *d_common, int64_t common_cells, int32_t *d_neighbours, int32_t *d_leader, uint8_t *d_keep,
                               uint64_t *d_out, hipStream_t st)
{
    if (!d_partner || partner_len < 1 || !d_row_start || !d_row_width || !d_row_group || S < 1 || S > SQ_DIST_MAX_ROWS || Wmax < 1 ||
        Wmax > SQ_DIST_MAX_COLS || !d_group_off || !d_mat_off || G < 1 || G > (1 << 24) || max_group_rows < 1 || max_group_rows > S ||
        !d_tiles || T < 1 || T > SqIdentity::tile_count(SqDistances::tiles(S)) || mode < 0 || mode >= SQ_DIST_MODES || threshold < 0 ||
        (mode == SQ_DIST_RELATIVE && threshold > 10000) || !d_scratch || !d_status || !d_npairs || common_cells < 0 ||
        !d_common != !common_cells || !d_neighbours || !d_leader || !d_keep || !d_out || phases < 1 || phases > 7) {
        sq_set_error(std::string(who) + ": bad argument");
        return -1;
    }
    if (scratch_bytes < sq_structure_distances_scratch(S, Wmax, T)) {
        sq_set_error(std::string(who) + ": scratch too small");
        return -1;
    }
    uint64_t *plane = (uint64_t *)d_scratch, *nbr = plane + SqDistances::plane_words(S, Wmax);
    unsigned long long *out = (unsigned long long *)d_out;
    HIPCK(hipMemsetAsync(d_out, 0, 16, st));
    if (phases & 1) {
        hipLaunchKernelGGL(sq_distances_planes_kernel, dim3((unsigned)SqDistances::row_words(S)), dim3(256), 0, st, d_partner, partner_len,
                           d_row_start, d_row_width, S, Wmax, plane, d_status, d_npairs);
        if (int rc = sq_check(hipGetLastError(), "sq_distances_planes_kernel")) return rc;
    }
    if (phases & 2) {
        HIPCK(hipMemsetAsync(d_neighbours, 0, sizeof(int32_t) * (size_t)S, st));
        if (d_common) HIPCK(hipMemsetAsync(d_common, 0, sizeof(int32_t) * (size_t)common_cells, st));
        const unsigned blocks = (unsigned)std::min<int32_t>(T, SQ_DIST_MAX_BLOCKS);
        hipLaunchKernelGGL(sq_distances_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const uint64_t *)plane, S, Wmax, d_row_group, d_group_off,
                           d_mat_off, G, d_tiles, T, mode, threshold, (const int32_t *)d_status, (const int32_t *)d_npairs, d_common,
                           common_cells, nbr, d_neighbours, out);
        if (int rc = sq_check(hipGetLastError(), "sq_distances_pairs_kernel")) return rc;
    }
    if (phases & 4) {
        launch_filter(nbr, S, d_group_off, G, max_group_rows, d_status, d_keep, d_leader, out, st);
        if (int rc = sq_check(hipGetLastError(), "sq_distances_filter_kernel")) return rc;
    }
    return 0;
}

extern "C" int sq_structure_distances(const int32_t *d_partner, int64_t partner_len, const int64_t *d_row_start, const int32_t *d_row_width,
                                      const int32_t *d_row_group, int32_t S, int32_t Wmax, const int32_t *d_group_off,
                                      const int64_t *d_mat_off, int32_t G, int32_t max_group_rows, const int32_t *d_tiles, int32_t T,
                                      int32_t mode, int32_t threshold, void *d_scratch, size_t scratch_bytes, int32_t *d_status,
                                      int32_t *d_npairs, int32_t *d_common, int64_t common_cells, int32_t *d_neighbours, int32_t *d_leader,
                                      uint8_t *d_keep, uint64_t *d_out, void *hip_stream)
{
    return structure_distances("sq_structure_distances", 7, d_partner, partner_len, d_row_start, d_row_width, d_row_group, S, Wmax, d_group_off,
                               d_mat_off, G, max_group_rows, d_tiles, T, mode, threshold, d_scratch, scratch_bytes, d_status, d_npairs, d_common,
                               common_cells, d_neighbours, d_leader, d_keep, d_out, (hipStream_t)hip_stream);
}

extern "C" int sq_structure_distances_phases(int32_t phases, const int32_t *d_partner, int64_t partner_len, const int64_t *d_row_start,
                                             const int32_t *d_row_width, const int32_t *d_row_group, int32_t S, int32_t Wmax,
                                             const int32_t *d_group_off, const int64_t *d_mat_off, int32_t G, int32_t max_group_rows,
                                             const int32_t *d_tiles, int32_t T, int32_t mode, int32_t threshold, void *d_scratch,
                                             size_t scratch_bytes, int32_t *d_status, int32_t *d_npairs, int32_t *d_common,
                                             int64_t common_cells, int32_t *d_neighbours, int32_t *d_leader, uint8_t *d_keep, uint64_t *d_out,
                                             void *hip_stream)
{
    return structure_distances("sq_structure_distances_phases", phases, d_partner, partner_len, d_row_start, d_row_width, d_row_group, S, Wmax,
                               d_group_off, d_mat_off, G, max_group_rows, d_tiles, T, mode, threshold, d_scratch, scratch_bytes, d_status,
                               d_npairs, d_common, common_cells, d_neighbours, d_leader, d_keep, d_out, (hipStream_t)hip_stream);
}
