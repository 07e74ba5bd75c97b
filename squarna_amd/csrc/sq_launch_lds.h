// sq_launch_lds.h -- the dynamic LDS of the launched kernels (the fill and mask kernels of a-1, the state / scan / score / choose
// kernels of a round, the ranking tail): per kernel ONE function that places its regions and adds up their bytes.  The launch
// site takes `total` from it and the kernel carves with the same call, so a size and its carving cannot drift apart; the
// thresholds that decide whether something is staged at all live here too, once each.  Host + device, nothing of HIP: the
// layouts and decisions are tested on the CPU (tests/test_launch_lds_host.py).
//
// Per job inside per launch.  A launch sizes its LDS for its LONGEST job (n, letters of the batch); a block of a shorter job
// n' <= n places what it stages by its own n' wherever the layout says "by the job" (fill, masks, the codes / reactivities of
// the score body) and by the launch's figures everywhere else.  Every layout below is monotone in its arguments: a region of
// the layout for (n', letters') ends inside the total for (n, letters).  The test states this for every layout.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef SQ_HD
#ifdef __HIPCC__
#define SQ_HD __host__ __device__
#else
#define SQ_HD
#endif
#endif

// ---- what a block may ask for ---------------------------------------------------------------------------------------------
#define SQ_LDS_PLAIN_MAX (64 * 1024)      // dynamic LDS a launch gets without asking; above it the kernel's limit is raised first
#define SQ_LDS_BLOCK_MAX (160 * 1024)     // the LDS of a CU: a launch that wants more is refused
SQ_HD inline bool sq_lds_needs_raise(size_t bytes) { return bytes > SQ_LDS_PLAIN_MAX; }
SQ_HD inline bool sq_lds_fits(size_t bytes) { return bytes <= SQ_LDS_BLOCK_MAX; }

SQ_HD inline size_t sq_lds_up(size_t o, size_t a) { return (o + a - 1) & ~(a - 1); }
SQ_HD inline int32_t sq_bits_nw(int n) { return (n + 31) / 32; }      // word-rows of a job's bit matrix (32 rows each)

// stems per structure the level scratch of sq_extend.h holds: 14 bytes each + the 64 group sizes and ranks
SQ_HD inline size_t sq_extend_lds_bytes(int T) { const size_t t = ((size_t)T + 7) & ~(size_t)7; return t * 14 + 64 * 4 + 64; }

// ---- sq_fill_kernel: attr[np] inc4[np] (uint8) chain[np] (int16) react[np] (double), np = n up to 16 ----------------------
#define SQ_FILL_LDS_N 4096                // the longest job whose O(N) inputs the fill stages
struct SqFillLds { uint32_t attr, inc4, chain, react; size_t total; };
SQ_HD inline bool sq_fill_staged(int n) { return n <= SQ_FILL_LDS_N; }
SQ_HD inline SqFillLds sq_fill_lds(int n)
{
    SqFillLds L;
    const uint32_t np = (uint32_t)((n + 15) & ~15);
    L.attr = 0; L.inc4 = L.attr + np; L.chain = L.inc4 + np; L.react = L.chain + 2u * np;
    L.total = (size_t)L.react + sizeof(double) * (size_t)np + 64;
    return L;
}

// ---- sq_bits_masks_kernel: ccode rcode inc [npad] (uint8); M[letters][nw + 3]; R[nw][letters] (uint32) --------------------
#define SQ_MASKS_LDS_MAX (60 * 1024)      // tables beyond it: sq_bits_direct_kernel
struct SqMasksLds { int32_t nw, mw; uint32_t ccode, rcode, inc, M, R; size_t total; };
SQ_HD inline SqMasksLds sq_bits_masks_lds(int n, int letters)
{
    SqMasksLds L;
    const uint32_t npad = (uint32_t)((n + 3) & ~3);
    L.nw = sq_bits_nw(n); L.mw = L.nw + 3;                                  // (one zero word in front of a column mask, two behind)
    L.ccode = 0; L.rcode = L.ccode + npad; L.inc = L.rcode + npad;
    L.M = L.inc + npad;
    L.R = L.M + (uint32_t)(sizeof(uint32_t) * (size_t)letters * L.mw);
    L.total = (size_t)L.R + sizeof(uint32_t) * (size_t)L.nw * letters + 16;
    return L;
}
SQ_HD inline bool sq_bits_masks_fit(const SqMasksLds &L) { return L.total <= SQ_MASKS_LDS_MAX; }

// ---- sq_state_kernel: P U SU (int16) E (uint8), n + 1 entries each in sections of np = (lds_n + 8) & ~7 -------------------
#define SQ_STATE_LDS_N 8000               // the longest sequence whose state arrays are assembled in LDS
struct SqStateLds { int32_t np; uint32_t P, U, SU, E; size_t total; };
struct SqStateArrays { int16_t *P, *U, *SU; uint8_t *E; };
SQ_HD inline int sq_state_lds_n(int maxn) { return maxn <= SQ_STATE_LDS_N ? maxn : 0; }     // 0: assembled in global memory
SQ_HD inline SqStateLds sq_state_lds(int lds_n)
{
    SqStateLds L;
    L.np = (lds_n + 8) & ~7;
    L.P = 0; L.U = L.P + 2u * (uint32_t)L.np; L.SU = L.U + 2u * (uint32_t)L.np; L.E = L.SU + 2u * (uint32_t)L.np;
    L.total = lds_n ? (size_t)L.E + (size_t)L.np + 64 : 0;
    return L;
}
// the arrays of a block, each section from the one before (four pointers from four offsets cost the state kernels 18 VGPRs); the
// CPU test holds them against the offsets
SQ_HD inline SqStateArrays sq_state_carve(char *base, const SqStateLds &L)
{
    SqStateArrays A;
    A.P = reinterpret_cast<int16_t *>(base + L.P); A.U = A.P + L.np; A.SU = A.U + L.np;
    A.E = reinterpret_cast<uint8_t *>(A.SU + L.np);
    return A;
}

// ---- sq_scan6_kernel: the F words, then the G words of the structure (fbstride uint32 in all) ----------------------------
SQ_HD inline size_t sq_scan6_lds(int fbstride) { return sizeof(uint32_t) * (size_t)fbstride; }

// ---- sq_state_scan_kernel: the state arrays, and once they are written out the scan words in the same bytes ---------------
struct SqStateScanLds {
    SqStateLds state; size_t scan;        // two phases of one block: a union, both from offset 0
    size_t total;
};
SQ_HD inline SqStateScanLds sq_state_scan_lds(int lds_n, int fbstride)
{
    SqStateScanLds L;
    L.state = sq_state_lds(lds_n); L.scan = sq_scan6_lds(fbstride);
    L.total = L.state.total > L.scan ? L.state.total : L.scan;
    return L;
}

// ---- sq_score_kernel / sq_bps_kernel -------------------------------------------------------------------------------------
// by the JOB (sq_score_lds_job): combined indices [n] (uint8) at 0, reactivities [n] (double) at n up to 16
// by the LAUNCH: partner / prefix copies P U SU (int16, sections of (lds_ns + 8) & ~7) behind the codes and reactivities of the
// launch's longest sequence; the cell table (double, 16-byte aligned); the survivor list of a chunk -- bpscore (double), key
// (uint32), length (uint16) for (SQ_SCORE_CHUNK + 1) x threads entries in mode 0 (two phases: a chunk's survivors and the
// remainder carried over from the one before), SQ_SCORE_CHUNK x threads in the one-pass modes; mode 0: the strands (SqStrand, 8
// bytes, 16-byte aligned) and their skip pointers (uint16).
#ifndef SQ_SCORE_CHUNK
#define SQ_SCORE_CHUNK 4                  // candidates per thread and chunk of sq_score_kernel's two-phase loop
#endif
#define SQ_SCORE_LDS_N 16384              // the longest sequence whose combined indices a scoring block keeps in LDS
#define SQ_LDS_STRANDS 1024               // strands of a structure a scoring block keeps in LDS at the most (longer lists: global memory)
#define SQ_STRAND_BYTES 8                 // sizeof(SqStrand) (sq_device.h asserts it)
struct SqScoreLds {
    int32_t lds_n, lds_nr, lds_ns;        // longest sequence whose codes / reactivities / state copies are staged (0: none)
    int32_t state_np, surv_n, str_cap;    // entries of a state section, of the survivor list, of the strand list
    uint32_t P, U, SU, cell, surv_bps, surv_key, surv_len, str, skip;
    size_t total;
};
struct SqScoreJobLds { uint32_t ci, reacts; bool ci_fits, reacts_fit, state_fits; };   // (fits: the launch has room for this job's)
SQ_HD inline uint32_t sq_score_reacts_off(int n) { return (uint32_t)((n + 15) & ~15); }
SQ_HD inline int32_t sq_score_state_np(int lds_ns) { return (lds_ns + 8) & ~7; }
SQ_HD inline uint32_t sq_score_state_off(int lds_n, int lds_nr) { return sq_score_reacts_off(lds_n) + (uint32_t)sizeof(double) * (uint32_t)lds_nr; }
SQ_HD inline int32_t sq_score_surv_n(int threads, int mode) { return (SQ_SCORE_CHUNK + (mode == 0 ? 1 : 0)) * threads; }   // (one-pass modes: no carry-over)
// the three staging decisions of a launch whose longest sequence has maxn nt
SQ_HD inline int sq_score_lds_n(int maxn) { return maxn <= SQ_SCORE_LDS_N ? maxn : 0; }
SQ_HD inline int sq_score_lds_nr(int maxn, bool need_reacts, int nr_lim) { return need_reacts && maxn <= nr_lim ? maxn : 0; }
SQ_HD inline int sq_score_lds_ns(int lds_n, int lds_nr, int maxn, int mode, size_t state_lim)
{
    const size_t with = (size_t)sq_score_state_off(lds_n, lds_nr) + 16 + 3 * sizeof(int16_t) * (size_t)sq_score_state_np(maxn);
    return (lds_n && mode == 0 && with <= state_lim) ? maxn : 0;
}
SQ_HD inline SqScoreLds sq_score_lds(int lds_n, int lds_nr, int lds_ns, int cell_entries, int threads, int mode, int str_cap)
{
    SqScoreLds L;
    L.lds_n = lds_n; L.lds_nr = lds_nr; L.lds_ns = lds_ns;
    L.state_np = sq_score_state_np(lds_ns); L.surv_n = sq_score_surv_n(threads, mode); L.str_cap = mode == 0 ? str_cap : 0;
    L.P = sq_score_state_off(lds_n, lds_nr);
    L.U = L.P + 2u * (uint32_t)L.state_np; L.SU = L.U + 2u * (uint32_t)L.state_np;
    size_t o = lds_n ? (size_t)L.SU + 2 * (size_t)L.state_np + 16 : 0;
    L.cell = (uint32_t)sq_lds_up(o, 16);
    o = (size_t)L.cell + sizeof(double) * (size_t)cell_entries;
    L.surv_bps = (uint32_t)sq_lds_up(o, 16);
    L.surv_key = L.surv_bps + (uint32_t)sizeof(double) * (uint32_t)L.surv_n;
    L.surv_len = L.surv_key + (uint32_t)sizeof(uint32_t) * (uint32_t)L.surv_n;
    o = (size_t)L.surv_len + sizeof(uint16_t) * (size_t)L.surv_n;
    L.str = (uint32_t)sq_lds_up(o, 16);
    L.skip = L.str + (uint32_t)SQ_STRAND_BYTES * (uint32_t)L.str_cap;
    L.total = mode == 0 ? (size_t)L.skip + sizeof(uint16_t) * (size_t)L.str_cap + 16 : o;
    return L;
}

// where a JOB of n nt puts what it stages by its own length, and what of the launch's room it may use
SQ_HD inline SqScoreJobLds sq_score_lds_job(const SqScoreLds &L, int n)
{
    return SqScoreJobLds{0u, sq_score_reacts_off(n), L.lds_n >= n, L.lds_nr >= n, L.lds_ns >= n};
}

// ---- sq_pool_choose_kernel: fin (double), q, key (uint32), ord (uint16), nsurv entries each -------------------------------
struct SqChooseLds { uint32_t fin, q, key, ord; size_t total; };
SQ_HD inline SqChooseLds sq_pool_choose_lds(int nsurv)
{
    SqChooseLds L;
    L.fin = 0; L.q = L.fin + (uint32_t)sizeof(double) * (uint32_t)nsurv; L.key = L.q + (uint32_t)sizeof(uint32_t) * (uint32_t)nsurv;
    L.ord = L.key + (uint32_t)sizeof(uint32_t) * (uint32_t)nsurv;
    L.total = (size_t)L.ord + sizeof(uint16_t) * (size_t)nsurv + 16;
    return L;
}

// ---- sq_tail_rank_kernel: one bitmap [bitwords] (uint32) per wave; keycap x (3 rank keys (double), priority (uint8)); the ------
// sequence's letter codes [32 x bitwords] (uint8); its partners in the known structure [32 x bitwords] (int16) when they fit
#define SQ_TAIL_REFP_WORDS 128            // bitmaps up to it (sequences up to 4,096 nt): the known structure's partners in LDS too
struct SqTailRankLds { uint32_t bits, key, pri, codes, refp; size_t total; };
SQ_HD inline int sq_tail_refp_lds(int bitwords) { return bitwords <= SQ_TAIL_REFP_WORDS ? 1 : 0; }
SQ_HD inline SqTailRankLds sq_tail_rank_lds(int waves, int bitwords, int keycap, int refp_lds)
{
    SqTailRankLds L;
    L.bits = 0;
    L.key = (uint32_t)sizeof(uint32_t) * (((uint32_t)waves * (uint32_t)bitwords + 1u) & ~1u);
    L.pri = L.key + 3u * (uint32_t)sizeof(double) * (uint32_t)keycap;
    L.codes = L.pri + (((uint32_t)keycap + 7u) & ~7u);
    L.refp = L.codes + 32u * (uint32_t)bitwords;
    L.total = (size_t)L.refp + 16 + (refp_lds ? sizeof(int16_t) * 32 * (size_t)bitwords : 0);
    return L;
}

// ---- sq_tail_pack_kernel: a row of levels [rowcap] (int16), the level scratch of sq_extend.h (16-byte aligned) -------------
// (the kernel keeps rowcap as its argument and places the scratch by sq_tail_pack_ext: with maxn and the struct it took a VGPR more)
struct SqTailPackLds { int32_t rowcap; uint32_t row, ext; size_t total; };
SQ_HD inline size_t sq_tail_pack_ext(int rowcap) { return sq_lds_up(sizeof(int16_t) * (size_t)rowcap, 16); }
SQ_HD inline SqTailPackLds sq_tail_pack_lds(int maxn, int tmax)
{
    SqTailPackLds L;
    L.rowcap = (maxn + 8) & ~7;
    L.row = 0; L.ext = (uint32_t)sq_tail_pack_ext(L.rowcap);
    L.total = (size_t)L.ext + sq_extend_lds_bytes(tmax);
    return L;
}

// ---- sq_tail_pairs_kernel: a row of partners [n up to 4] (int32) ----------------------------------------------------------
SQ_HD inline size_t sq_tail_pairs_lds(int maxn) { return (((size_t)maxn + 3) & ~(size_t)3) * sizeof(int32_t) + 16; }
