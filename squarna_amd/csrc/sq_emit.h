// The emission stage of a 256-thread block: every thread may produce a record per step; the records are compacted into an
// LDS stage of SQ_EMIT_STAGE entries and written out behind ONE global atomic per flush (an atomic per record -- and per
// wave -- on one address was sq_colselect_kernel's whole 1.8 ms for 100 MB of reads).  Used by sq_colselect_kernel,
// sq_pair_select_kernel and sq_window_count_kernel; the kernels keep their own record arrays (the fields differ) and hand
// flush() a lambda that copies record k of the stage to its place in the results.
//
//     __shared__ SqEmitStage em;  em.init();
//     for every step (block-uniform trip count) {
//         const uint32_t at = em.slot(hit);  if (hit) s_field[at] = ...;
//         em.step(counter, write);
//     }
//     em.finish(counter, write);
//
// Why the flush decision is block-uniform.  flush() contains barriers, so every wave of the block must take it or none.
// The decision is made from staged(): barrier, ONE read of the counter by every thread, barrier.  The first barrier comes
// after every wave's add of this step; the second before any wave's add of the next step (slot() is only called after
// staged() has returned) and before flush()'s reset.  No write to the counter lies between the two barriers, so every
// thread reads the same number, whatever the waves' relative speed.  (Reading the counter in the `if` itself after one
// barrier -- the earlier form of the two select kernels -- is NOT that: a faster wave's next add can land between two
// waves' reads, they disagree about the flush, and its barriers pair with the loop's.)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define SQ_EMIT_STAGE 1024u
#define SQ_EMIT_BLOCK 256u

struct SqEmitStage {
    uint32_t n;                          // records staged since the last flush
    unsigned long long base;             // the flush's place in the results, from thread 0 to the block

    __device__ __forceinline__ void init()
    {
        if (threadIdx.x == 0) n = 0u;
        __syncthreads();
    }

    // The thread's place in the stage (meaningful where `hit`): a wave ballot, one LDS atomic by one lane per wave, the
    // prefix popcount.  Wave-uniform control flow around the call is the caller's; one step adds at most SQ_EMIT_BLOCK.
    __device__ __forceinline__ uint32_t slot(bool hit)
    {
        const int lane = (int)(threadIdx.x & 63u);
        const unsigned long long m = __ballot(hit);
        if (m == 0ull) return 0u;
        uint32_t b0 = 0u;
        if (lane == 0) b0 = atomicAdd(&n, (uint32_t)__popcll(m));
        b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
        return b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    }

    // The number of staged records, the same for every thread of the block (see above).
    __device__ __forceinline__ uint32_t staged()
    {
        __syncthreads();
        const uint32_t k = n;
        __syncthreads();
        return k;
    }

    // Block-uniform call with staged()'s k: one atomicAdd of k on *counter by one thread, write(i, base + i) for every
    // i < k (the caller's lambda stores a record only when base + i is below its capacity: the counter counts them all).
    // The stage is free again on return.
    template <class Write> __device__ __forceinline__ void flush(uint32_t k, unsigned long long *counter, Write write)
    {
        if (threadIdx.x == 0) { base = atomicAdd(counter, (unsigned long long)k); n = 0u; }
        __syncthreads();
        const unsigned long long b = base;
        for (uint32_t i = threadIdx.x; i < k; i += SQ_EMIT_BLOCK) write(i, b + i);
        __syncthreads();
    }

    // After every step: flush when the next step's SQ_EMIT_BLOCK records might not fit.
    template <class Write> __device__ __forceinline__ void step(unsigned long long *counter, Write write)
    {
        const uint32_t k = staged();
        if (k > SQ_EMIT_STAGE - SQ_EMIT_BLOCK) flush(k, counter, write);
    }

    // After the last step: flush when anything is staged.
    template <class Write> __device__ __forceinline__ void finish(unsigned long long *counter, Write write)
    {
        const uint32_t k = staged();
        if (k > 0u) flush(k, counter, write);
    }
};
