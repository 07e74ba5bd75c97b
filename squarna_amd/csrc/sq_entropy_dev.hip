// sq_entropy_dev.hip -- the reference's entropy mode as data (Entropy; SQRNdbnseq.py:520-545, 1087-1089): for every listed job
// the stems of AnnotateStems with no selected stem (the survivor list the scoring kernel leaves in device memory in mode 2:
// len >= minlen, bpscore >= minbpscore) form a symmetric N x N matrix -- every cell (v, w) of a stem and its mirror hold the
// stem's TOTAL score -- and row i with S = sum_j m[i][j] != 0 has the entropy H_i = -sum_{m != 0} p log2 p, p = m[i][j] / S,
// else 0.  Out: H_i per position, their mean over the N positions, the number of stems.
//
// One dense fp64 tile per job in the caller's scratch (8 N^2 bytes), four kernels per round chunk, all order-free:
//   (memset)                 the chunk's tiles := 0
//   sq_entropy_scatter_kernel  every stem's score to its cells and their mirrors with PLAIN stores: the stems are maximal runs
//                            of their anti-diagonals, so their cells are pairwise disjoint -- no cell is written twice, whatever
//                            order the (unordered) survivor list has
//   sq_entropy_rows_kernel   one wave per row: lanes stride the columns and sum in column order, a fixed DPP reduction forms S,
//                            a second pass over the row (it is in L2: <= 256 KB) forms H_i the same way
//   sq_entropy_mean_kernel   one block per job: threads stride the rows in order, a fixed tree in LDS, / N
// A value depends on the job's own tile alone and every sum has one fixed order: the same record gives the same bits alone, in
// any batch and in any chunk.  Algorithmic bytes: 8 N^2 zeroed + 16 per stem cell + 2 x 8 N^2 read.
#include "sq_host_int.h"

#define SQ_ENT_WAVES 4                  // rows (waves) of a block of sq_entropy_rows_kernel

// every lane gets the sum of the 64 lanes' values, added in one fixed order (the gfx9 scan sequence; lanes that shift in
// nothing add +0.0)
__device__ __forceinline__ double sq_wave_sum_f64(double v)
{
    v += sq_dpp_f64<0x111, 0xf>(0.0, v);
    v += sq_dpp_f64<0x112, 0xf>(0.0, v);
    v += sq_dpp_f64<0x114, 0xf>(0.0, v);
    v += sq_dpp_f64<0x118, 0xf>(0.0, v);
    v += sq_dpp_f64<0x142, 0xa>(0.0, v);
    v += sq_dpp_f64<0x143, 0xc>(0.0, v);
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63), hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

// structure blockIdx.x of the chunk = list entry first + blockIdx.x
extern "C" __global__ __launch_bounds__(256) void sq_entropy_scatter_kernel(SqDevCtx c, const SqStruct *structs, SqScanArgs a, int first,
                                                                           SqEntropySink e)
{
    const SqStruct st = structs[blockIdx.x];
    const SqJob jb = c.jobs[st.job];
    const int n = jb.n;
    // (a list that outgrew its slice is reported by the round's counters; what was stored ends at the slice's end)
    const uint32_t ok_cap = (uint32_t)(((size_t)jb.cand_cap * (sizeof(SqCand) - sizeof(SqKey))) / sizeof(SqOk));
    const uint32_t cnt = a.ok_cnt[st.slot], nok = cnt < ok_cap ? cnt : ok_cap;
    const SqOk *oks = sq_oks(a, st, jb.cand_cap);
    double *tile = e.d_tiles + e.d_tile_off[first + blockIdx.x];
    for (uint32_t q = blockIdx.y * 256 + threadIdx.x; q < nok; q += gridDim.y * 256) {
        const SqOk cd = oks[q];
        const int s = (int)(cd.key >> 16), i0 = (int)(cd.key & 0xFFFFu), j0 = s - i0;
        for (int t = 0; t < (int)cd.len; t++) {
            const int v = i0 + t, w = j0 - t;
            if (v >= n || w < 0 || w >= n) break;              // (never: a stem lies inside its sequence)
            tile[(int64_t)v * n + w] = cd.bps;
            tile[(int64_t)w * n + v] = cd.bps;
        }
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) e.d_nstems[first + blockIdx.x] = (int32_t)nok;
}

extern "C" __global__ __launch_bounds__(64 * SQ_ENT_WAVES) void sq_entropy_rows_kernel(SqDevCtx c, const SqStruct *structs, int first,
                                                                                      SqEntropySink e)
{
    const int k = first + blockIdx.x;
    const int n = c.jobs[structs[blockIdx.x].job].n;
    const int row = blockIdx.y * SQ_ENT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t p0 = e.d_pos_off[k];
    if (row >= n || row >= e.d_pos_off[k + 1] - p0) return;     // (wave-uniform)
    const double *m = e.d_tiles + e.d_tile_off[k] + (int64_t)row * n;
    double part = 0.0;
    for (int j = lane; j < n; j += 64) part += m[j];
    const double S = sq_wave_sum_f64(part);
    double H = 0.0;
    if (S != 0.0) {                                             // :541 (`if row.sum()`: a NaN sum is true as well)
        part = 0.0;
        for (int j = lane; j < n; j += 64) {
            const double x = m[j];
            if (x == 0.0 && S == S) continue;                   // (0 / S == 0 for every S but a NaN: no division for the empty cells)
            const double p = x / S;
            if (p != 0.0) part += -(p * log2(p));               // :543 (`if q` on the quotient)
        }
        H = sq_wave_sum_f64(part);
    }
    if (lane == 0) e.d_position[p0 + row] = H;
}

extern "C" __global__ __launch_bounds__(256) void sq_entropy_mean_kernel(SqDevCtx c, const SqStruct *structs, int first, SqEntropySink e)
{
    __shared__ double s_sum[256];
    const int k = first + blockIdx.x;
    const int n = c.jobs[structs[blockIdx.x].job].n;
    const int64_t p0 = e.d_pos_off[k];
    const int64_t given = e.d_pos_off[k + 1] - p0;
    const int rows = given < n ? (int)given : n;
    double part = 0.0;
    for (int i = threadIdx.x; i < rows; i += 256) part += e.d_position[p0 + i];
    s_sum[threadIdx.x] = part;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) e.d_mean[k] = s_sum[0] / (double)n;   // (no position: 0 / 0 = NaN)
}

// The entropy kernels of one round chunk: structures [0, S) of d_structs = list entries [first, first + S); enqueued on st
// behind the round's scoring kernel.  h_tile_off: the entries' tile offsets on the host (the chunk's tiles are contiguous).
int sq_entropy_launch(sq_batch *b, hipStream_t st, const SqStruct *d_structs, const SqScanArgs &scan, int S, int first, int maxn,
                      int64_t maxcap, const SqEntropySink &e)
{
    const int64_t t0 = e.h_tile_off[first], t1 = e.h_tile_off[first + S];
    if (t1 > t0) HIPCK(hipMemsetAsync(e.d_tiles + t0, 0, (size_t)(t1 - t0) * sizeof(double), st));
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(maxcap / 4096, 1), 64);
    const unsigned rowblocks = (unsigned)std::max(1, (maxn + SQ_ENT_WAVES - 1) / SQ_ENT_WAVES);
    hipLaunchKernelGGL(sq_entropy_scatter_kernel, dim3(S, blocks), dim3(256), 0, st, b->ctx, d_structs, scan, first, e);
    hipLaunchKernelGGL(sq_entropy_rows_kernel, dim3(S, rowblocks), dim3(64 * SQ_ENT_WAVES), 0, st, b->ctx, d_structs, first, e);
    hipLaunchKernelGGL(sq_entropy_mean_kernel, dim3(S), dim3(256), 0, st, b->ctx, d_structs, first, e);
    return sq_check(hipGetLastError(), "sq_entropy kernels");
}

static size_t entropy_header_bytes(int32_t njob) { return align_up(sizeof(int64_t) * ((size_t)std::max(njob, 0) + 1), 256); }

extern "C" size_t sq_entropy_scratch(int32_t njob, int64_t cells)
{
    return njob >= 0 && cells >= 0 ? entropy_header_bytes(njob) + sizeof(double) * (size_t)cells : 0;
}

extern "C" int sq_entropy_rows(sq_batch *b, int32_t njob, const int32_t *job_ids, const int64_t *d_pos_off, double *d_position,
                               double *d_mean, int32_t *d_nstems, void *d_scratch, size_t scratch_bytes)
{
    SqSlackGuard slack_guard;
    if (!b || njob < 0 || (njob && (!job_ids || !d_pos_off || !d_position || !d_mean || !d_nstems || !d_scratch))) {
        sq_set_error("bad argument");
        return -1;
    }
    if (!njob) return 0;
    std::vector<int64_t> tile_off((size_t)njob + 1, 0);
    std::vector<HStruct> hs(njob);
    std::vector<SView> views(njob);
    for (int k = 0; k < njob; k++) {
        const int j = job_ids[k];
        if (j < 0 || j >= b->njobs) { sq_set_error("bad job index"); return -1; }
        const int n = b->jobs[j].n;
        if (n > 32768) {                                          // (a stem's key packs i and i + j in 16 bits each)
            sq_set_error("sq_entropy_rows: a sequence of " + std::to_string(n) + " nt; at most 32768 are supported");
            return -1;
        }
        tile_off[k + 1] = tile_off[k] + (int64_t)n * n;
        hs[k].job = j; views[k] = SView{j, 1.0, &hs[k]};
    }
    const size_t need = sq_entropy_scratch(njob, tile_off[njob]);
    if (scratch_bytes < need) {
        sq_set_error("sq_entropy_rows: scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(need) + " needed");
        return -1;
    }
    // (tile_off outlives the copy: every round chunk below waits for the stream)
    HIPCK(hipMemcpyAsync(d_scratch, tile_off.data(), sizeof(int64_t) * tile_off.size(), hipMemcpyHostToDevice, b->stream));
    SqEntropySink ent{tile_off.data(), (const int64_t *)d_scratch, (double *)((char *)d_scratch + entropy_header_bytes(njob)),
                      d_pos_off, d_position, d_mean, d_nstems};
    AlignSink sink{nullptr, nullptr, 0, nullptr, &ent};
    std::vector<std::vector<HStem>> unused;
    return sq_run_round_impl(b, b->lane_full, views, 2, unused, &sink);
}
