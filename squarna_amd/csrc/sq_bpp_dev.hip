// sq_bpp_dev.hip -- the bpp term of bpp != 0 paramsets from base-pair probabilities that already live on the device.
//
// The reference scales the score matrix by (bppm / max(bppm)) ** |bpp| (SQRNdbnseq.py:341-364).  With sq_batch_desc::bpp_term the
// caller forms that term on the host, once per job, and the batch uploads 8 N^2 bytes per job.  With
// sq_batch_desc::bpp_matrix_dev the caller hands over ONE N x N fp64 matrix per sequence in device memory (rows `ld` doubles
// apart) and two kernels form every job's term where the fill reads it (SqDevCtx::mat64 + SqJob::mat64_off, dense N x N):
//   * sq_bpp_max_kernel: the maximum of every sequence's matrix.  Many blocks per sequence; a block reduces what it read in
//     registers, across its waves through LDS, and issues ONE 64-bit unsigned atomicMax on the bit pattern -- the order of
//     non-negative doubles is the order of their bit patterns, so the result is exact whatever the order of arrival.  No
//     block waits for another.
//   * sq_bpp_term_kernel: every element b once, q = b / max (one IEEE division), and per bpp job of the sequence q
//     (|bpp| == 1) or sqrt(q) (|bpp| == 0.5, correctly rounded): the two operations numpy performs for these exponents.
//     max == 0 ("the matrix stays as it is", :350,360): the neutral term -- 1.0 for multiplied jobs; for added jobs -0.0
//     where the fill adds it (x + -0.0 keeps every x bit for bit, -0.0 included) and +0.0 in the cells the fill leaves
//     alone (bpboolmatrix == 0: the term stays there as the cell's value, and the reference's cell is +0.0).
// Both kernels walk a matrix in chunks of SQ_BPP_CHUNK doubles of one row (a dense matrix, ld == N, is one row of N^2), with
// 16-byte loads and stores where the address allows: the base and ld are only 8-byte aligned and N^2 may be odd, so a chunk
// has a scalar head when it starts on an odd double and a scalar tail when an odd one is left; a job's destination may sit
// on the other parity, then its pairs are stored as two doubles.  8 N^2 (2 + J) bytes per sequence with J bpp jobs: HBM-bound.
#include <hip/hip_runtime.h>
#include "sq_device.h"
#include "sq_cells.h"

static_assert(SQ_BPP_CHUNK == 2 * 4 * 256, "a chunk is four pairs per thread of a 256-thread block");

// the chunks of one sequence's matrix
struct SqBppWalk {
    int64_t len, sstride, dstride;   // doubles per row; between rows of the source / of a destination
    int32_t cpr;                     // chunks per row
    int64_t units;                   // rows x cpr
    __device__ explicit SqBppWalk(const SqBppSeq &q)
    {
        const bool dense = q.ld == q.n;
        len = dense ? (int64_t)q.n * q.n : q.n;
        sstride = q.ld; dstride = q.n;
        cpr = (int32_t)((len + SQ_BPP_CHUNK - 1) / SQ_BPP_CHUNK);
        units = (dense ? 1 : (int64_t)q.n) * cpr;
    }
};

extern "C" __global__ __launch_bounds__(256) void sq_bpp_max_kernel(const SqBppSeq *seqs, unsigned long long *maxbits)
{
    const SqBppSeq q = seqs[blockIdx.y];
    const SqBppWalk w(q);
    const int tid = threadIdx.x;
    double m = 0.0;                                                   // (probabilities are >= 0; -0.0 > 0.0 is false: m stays +0.0 or above)
    for (int64_t u = blockIdx.x; u < w.units; u += gridDim.x) {
        const int64_t r = u / w.cpr, k = u - r * w.cpr;
        const double *p = q.src + r * w.sstride + k * SQ_BPP_CHUNK;
        const int cnt = (int)(w.len - k * SQ_BPP_CHUNK < SQ_BPP_CHUNK ? w.len - k * SQ_BPP_CHUNK : SQ_BPP_CHUNK);
        const int head = (int)(((uintptr_t)p >> 3) & 1), npair = (cnt - head) >> 1;
        if (tid == 0 && head) { const double v = p[0]; m = v > m ? v : m; }
        if (tid == 1 && ((cnt - head) & 1)) { const double v = p[cnt - 1]; m = v > m ? v : m; }
        double2 v[4];                                                 // (a chunk is at most 4 pairs per thread: the loads first)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int pi = tid + 256 * t;
            v[t] = pi < npair ? *reinterpret_cast<const double2 *>(p + head + 2 * pi) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            m = v[t].x > m ? v[t].x : m;
            m = v[t].y > m ? v[t].y : m;
        }
    }
    for (int off = 32; off; off >>= 1) { const double o = __shfl_xor(m, off); m = o > m ? o : m; }
    __shared__ double s_m[4];
    if ((tid & 63) == 0) s_m[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; k++) m = s_m[k] > m ? s_m[k] : m;
        if (m > 0.0) atomicMax(maxbits + blockIdx.y, (unsigned long long)__double_as_longlong(m));   // (the slot was zeroed: +0.0)
    }
}

// one value of the term into every bpp job of the sequence
__device__ __forceinline__ void sq_bpp_store1(double *mat64, const SqBppJob *jobs, int nj, int64_t at, double qv, double sv)
{
    for (int j = 0; j < nj; j++) mat64[jobs[j].dst_off + at] = (jobs[j].mode & 1) ? sv : qv;
}

extern "C" __global__ __launch_bounds__(256) void sq_bpp_term_kernel(SqDevCtx c, const SqBppSeq *seqs, const SqBppJob *jobs,
                                                                     const unsigned long long *maxbits)
{
    const SqBppSeq q = seqs[blockIdx.y];
    const SqBppWalk w(q);
    const SqBppJob *jl = jobs + q.job0;
    const int nj = q.njob, tid = threadIdx.x;
    const double mx = __longlong_as_double((long long)maxbits[blockIdx.y]);
    if (!(mx > 0.0)) {
        // the neutral term (rare: one pass of scalar stores)
        for (int64_t u = blockIdx.x; u < w.units; u += gridDim.x) {
            const int64_t r = u / w.cpr, k = u - r * w.cpr;
            const int64_t at0 = r * w.dstride + k * SQ_BPP_CHUNK;
            const int cnt = (int)(w.len - k * SQ_BPP_CHUNK < SQ_BPP_CHUNK ? w.len - k * SQ_BPP_CHUNK : SQ_BPP_CHUNK);
            for (int e = tid; e < cnt; e += 256) {
                const int64_t at = at0 + e;
                const int i = (int)(at / q.n), j = (int)(at - (int64_t)i * q.n);
                for (int t = 0; t < nj; t++) {
                    double v = 1.0;
                    if (jl[t].mode & 2) {
                        const SqJob jb = c.jobs[jl[t].job];
                        v = (j > i && sq_cell_bool(c, jb, c.psets + jb.pset, i, j)) ? -0.0 : 0.0;
                    }
                    c.mat64[jl[t].dst_off + at] = v;
                }
            }
        }
        return;
    }
    const bool rt = q.any_sqrt != 0;
    for (int64_t u = blockIdx.x; u < w.units; u += gridDim.x) {
        const int64_t r = u / w.cpr, k = u - r * w.cpr;
        const double *p = q.src + r * w.sstride + k * SQ_BPP_CHUNK;
        const int64_t at0 = r * w.dstride + k * SQ_BPP_CHUNK;
        const int cnt = (int)(w.len - k * SQ_BPP_CHUNK < SQ_BPP_CHUNK ? w.len - k * SQ_BPP_CHUNK : SQ_BPP_CHUNK);
        const int head = (int)(((uintptr_t)p >> 3) & 1), npair = (cnt - head) >> 1;
        if (tid == 0 && head) { const double qv = p[0] / mx; sq_bpp_store1(c.mat64, jl, nj, at0, qv, rt ? __dsqrt_rn(qv) : qv); }
        if (tid == 1 && ((cnt - head) & 1)) {
            const double qv = p[cnt - 1] / mx;
            sq_bpp_store1(c.mat64, jl, nj, at0 + cnt - 1, qv, rt ? __dsqrt_rn(qv) : qv);
        }
        double2 in[4];                                                // (a chunk is at most 4 pairs per thread: the loads first)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int pi = tid + 256 * t;
            in[t] = pi < npair ? *reinterpret_cast<const double2 *>(p + head + 2 * pi) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u4 = 0; u4 < 4; u4++) {
            const int pi = tid + 256 * u4;
            if (pi >= npair) break;
            const int e = head + 2 * pi;
            const double2 v = in[u4];
            const double2 qv = make_double2(v.x / mx, v.y / mx);
            const double2 sv = rt ? make_double2(__dsqrt_rn(qv.x), __dsqrt_rn(qv.y)) : qv;
            for (int t = 0; t < nj; t++) {
                double *dst = c.mat64 + jl[t].dst_off + at0 + e;
                const double2 o = (jl[t].mode & 1) ? sv : qv;
                if (((uintptr_t)dst & 15) == 0) *reinterpret_cast<double2 *>(dst) = o;     // (the same for every pair of the chunk)
                else { dst[0] = o.x; dst[1] = o.y; }
            }
        }
    }
}

void sq_launch_bpp_terms(const SqDevCtx &c, const SqBppSeq *d_seqs, int nrec, const SqBppJob *d_jobs, unsigned long long *d_maxbits,
                         int64_t max_units, hipStream_t st)
{
    const unsigned gx = (unsigned)(max_units < 1 ? 1 : max_units > 1024 ? 1024 : max_units);
    for (int r0 = 0; r0 < nrec; r0 += 65535) {                        // (grid.y is limited to 65,535 sequences per launch)
        const unsigned ny = (unsigned)(nrec - r0 < 65535 ? nrec - r0 : 65535);
        hipLaunchKernelGGL(sq_bpp_max_kernel, dim3(gx, ny), dim3(256), 0, st, d_seqs + r0, d_maxbits + r0);
        hipLaunchKernelGGL(sq_bpp_term_kernel, dim3(gx, ny), dim3(256), 0, st, c, d_seqs + r0, d_jobs, (const unsigned long long *)(d_maxbits + r0));
    }
}
