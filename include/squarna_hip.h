/*
 * squarna_hip.h -- C ABI of libsquarna_hip.so, the MI355X (gfx950) folding core
 * that replaces the single-sequence hot path of febos/SQUARNA v3.2.2.
 *
 * The reference is pure Python and has no FFI of its own; the
 * boundary a maintainer would bind is the Python function surface of
 * src/SQUARNA/SQRNdbnseq.py.  Each entry point below names the reference
 * function(s) it replaces (file:line).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no exceptions across the boundary.
 *   - Every function returns 0 on success, <0 for an invalid argument / capacity
 *     problem, >0 for a HIP error code; sq_last_error() gives the message.
 *   - The caller owns all DEVICE memory: a single workspace (e.g. a torch uint8
 *     tensor) whose size sq_batch_workspace_bytes() reports.  The library never
 *     allocates or frees device memory; it keeps small pinned host staging
 *     buffers per batch.
 *   - All device work is enqueued on the caller's stream (hipStream_t passed as
 *     void*); entry points that return host results synchronise that stream.
 *   - Sequences are passed pre-encoded by the host layer (upper-cased, T->U,
 *     gap-free: SQRNdbnseq.py:1004,1023): code 0..25 = 'A'..'Z', 26 = ';',
 *     27 = '&', 28 = any other symbol.
 */
#ifndef SQUARNA_HIP_H
#define SQUARNA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQ_API __attribute__((visibility("default")))

#define SQ_ALPHABET 32
#define SQ_CODE_SEP1 26   /* ';' */
#define SQ_CODE_SEP2 27   /* '&' */
#define SQ_CODE_OTHER 28

/* position flags (ParseRestraints, SQRNdbnseq.py:370-376) */
#define SQ_FLAG_RX 1      /* '_' or '+': forced unpaired           */
#define SQ_FLAG_RLEFT 2   /* '/' : may not be the 3' partner (j)    */
#define SQ_FLAG_RRIGHT 4  /* '\': may not be the 5' partner (i)     */

/* algorithms bitmask (config key "algorithms", SQUARNA.py:62-63) */
#define SQ_ALGO_G 1
#define SQ_ALGO_N 2
#define SQ_ALGO_H 4
#define SQ_ALGO_E 8

/* One parameter set of a .conf file (SQUARNA.py:15-77; read at SQRNdbnseq.py:1050-1062). */
typedef struct sq_paramset {
    double bpweight[SQ_ALPHABET * SQ_ALPHABET]; /* weight of pair (a,b), both orientations filled (SQRNdbnseq.py:282-284) */
    uint8_t inbps[SQ_ALPHABET * SQ_ALPHABET];   /* 1 iff the pair is a key of bpweights (either orientation)          */
    double bpp;                /* != 0: the batch must carry the job's probability term in sq_batch_desc.bpp_term
                                  (computed by the caller from ViennaRNA, SQRNdbnseq.py:341-364); the fill applies it */
    double suboptmax, suboptmin, suboptsteps;
    double minlen, minbpscore, minfinscorefactor;
    double bracketweight, distcoef, orderpenalty, loopbonus;
    double maxstemnum;
    uint32_t algorithms;       /* SQ_ALGO_* */
    uint32_t reserved;
} sq_paramset;

/* Host-side description of a batch: sequences, per-position inputs, jobs.
 * A job = one (sequence, paramset) pair = one pass of SQRNdbnseq.py:1048-1199. */
typedef struct sq_batch_desc {
    int32_t nseq;
    const int32_t *seq_off;     /* [nseq+1] offsets into the per-position arrays                */
    const uint8_t *codes;       /* letter codes                                                  */
    const uint8_t *flags;       /* SQ_FLAG_*                                                     */
    const double *reacts;       /* per-position reactivities after ProcessReacts (SQRNdbnseq.py:32-59); NULL: 0.5 everywhere
                                 * (SQRNdbnseq.py:1013-1014: no record of the batch came with reactivities) */
    const int32_t *rbp_off;     /* [nseq+1] offsets (in pairs) into rbps                         */
    const int32_t *rbps;        /* restraint base pairs (v,w), v<w, gap-free coordinates; any number, a position in at most one */
    int32_t npset;
    const sq_paramset *psets;
    int32_t njobs;
    const int32_t *job_seq;     /* [njobs] */
    const int32_t *job_pset;    /* [njobs] */
    /* optional dense fp64 inputs, one N x N row-major matrix per job (NULL entries allowed, array may be NULL): */
    const double *const *ext_bool;   /* AnnotateStems/OptimalStems shims: caller-supplied bpboolmatrix   */
    const double *const *ext_score;  /* ... and bpscorematrix (SQRNdbnseq.py:427-428,792-797)            */
    const double *const *mul_score;  /* alignment step-2 weighting, bpscorematrix *= shortsmat (SQRNdbnseq.py:1084-1085) */
    const double *const *bpp_term;   /* paramsets with bpp != 0: (bppm / max(bppm)) ** |bpp| computed by the caller from
                                        ViennaRNA's base-pair probabilities; the fill applies scoremat *= term (bpp > 0)
                                        or scoremat += term (bpp < 0) (SQRNdbnseq.py:341-364).  A job takes either
                                        mul_score or bpp_term, not both.  NULL entry with bpp != 0: max(bppm) was 0,
                                        the matrix stays as it is (:350,360).  Probabilities that are on the device
                                        already: bpp_matrix_dev below, the term is then formed there.                */
    int32_t interchainonly;     /* SQRNdbnseq.py:264-271,301 */
    int32_t max_structs;        /* structures evaluated per round chunk (0 = default 4096); also the structure
                                   slots of the device-side pools / chained rounds: a fold whose pools outgrow
                                   them is repeated by the library's host loop (same results, slower)           */
    int32_t cand_per_nt;        /* candidate capacity per structure = cand_per_nt * N (0 = 32)  */
    int32_t batch_flags;        /* SQ_BATCH_* */
    /* Alignment step 2 without one dense matrix per sequence (SQRNdbnseq.py:1031-1034 deletes the gap rows and columns
     * of the same L x L stem matrix for every sequence, :1084-1085 multiplies): ONE L x L row-major fp64 matrix in
     * DEVICE memory (the step-1 matrix never has to leave the GPU) and, per sequence, the alignment column of each of
     * its gap-free positions.  A job with mul_shared[j] != 0 takes bpscorematrix[a][b] *= M[cols[a]][cols[b]]: at
     * sq_batch_create the library copies M into the workspace in a diagonal-major layout (on the batch's stream: M must
     * be complete there; the caller's matrix is not read afterwards) and the kernels read a cell's weight from that copy
     * through `cols` where they need it -- no per-sequence N x N slice exists (SQ_MUL_GATHER=1 in the environment restores
     * the gathered slices of earlier versions: 8 N^2 bytes per job).  Such a job has no mul_score / bpp_term / caller
     * matrices.  All NULL / 0: not used. */
    const double *mul_matrix_dev;   /* device pointer */
    int32_t mul_L;
    const int32_t *mul_cols;        /* [seq_off[nseq]] host: column of every position (same offsets as codes)   */
    const uint8_t *mul_shared;      /* [njobs] host                                                              */
    double mul_maxabs;              /* max |M| (an upper bound is enough: it only widens the scan's fp32 margin) */
    /* Base-pair probabilities that already live on the device (a GPU predictor or partition function; one upload reused
     * across paramsets and calls): per sequence ONE N x N row-major fp64 matrix `bppm`, values >= 0, in DEVICE memory.
     * Every bpp != 0 job of such a sequence gets its term (bppm / max(bppm)) ** |bpp| formed on the device at
     * sq_batch_create, where bpp_term's upload would have put it (same workspace bytes as a host bpp_term on those jobs):
     * one kernel takes each matrix's maximum, one reads every element once and writes q = b / max (|bpp| == 1) or sqrt(q)
     * (|bpp| == 0.5) to each job -- the IEEE operations numpy performs, so the bytes are those of a host-formed term.
     * max == 0: the neutral term (1.0 multiplied, -0.0 added), the matrix stays as it is (:350,360).  Other exponents
     * return -1: they take the host term (bpp_term), because the host libm's pow is the rule there.  Such a job has no
     * bpp_term / mul_score / caller matrices / mul_shared (-4).  The kernels run on the batch's stream: the matrices must
     * be complete there; they are not read after sq_batch_create returns and never written.  sq_batch_workspace_bytes
     * only compares the entries with NULL.  Appended at the end: descriptors of earlier versions keep their layout. */
    const double *const *bpp_matrix_dev;   /* [nseq] host array of DEVICE pointers; NULL entries allowed, array may be NULL   */
    const int32_t *bpp_matrix_ld;          /* [nseq] host: row stride of each matrix in doubles (>= N); NULL: dense, ld = N */
} sq_batch_desc;

/* No fp32 score matrices in the workspace (4 N^2 bytes per job saved): everything except
 * sq_bpmatrix_fill works, the fold path only needs the 1-bit-per-cell diagonal matrices. */
#define SQ_BATCH_NO_FP32 1
/* The batch will be folded with pools wider than one (poollim > 1) and holds sequences of 257-1,024 nt: the workspace
 * reserves pages for the lists every structure of such a pool hands to its children -- its runs with their bpscores and
 * the finalscores it knew (SQRNdbnseq.py:427-495 and :640-751 are then evaluated for what the child's new stem changed,
 * not for the whole structure; the results are the same).  Without the flag (or with SQ_NO_POOL_KEPT=1 in the environment)
 * such pools run the launched round kernels.  Pages per structure slot: SQ_KEPT_PPS (default 3 of 6 KB per generation at 500 nt, growing with the square of the length),
 * at most SQ_KEPT_GB gigabytes (default 48) in all. */
#define SQ_BATCH_POOL_LISTS 2

typedef struct sq_batch sq_batch;   /* opaque */

/* One stem as the reference's [bps, len, bpscore, finalscore] record
 * (SQRNdbnseq.py:417,747): bps = (i+k, j-k), k = 0..len-1. */
typedef struct sq_stem {
    int32_t i, j, len, reserved;
    double bpscore;
    double finscore;
} sq_stem;

/* Options of the SQRNdbnseq tail (SQRNdbnseq.py:973-980). */
typedef struct sq_fold_opts {
    int32_t poollim;        /* SQRNdbnseq.py:1147,1191 (1: rounds chained on the device; > 1: pools booked on the device) */
    int32_t conslim;        /* :1236 */
    int32_t toplim;         /* :1282 */
    int32_t hardrest;       /* :1226-1228 */
    int32_t rankbydiff;     /* :917-955 */
    int32_t rankby[3];      /* :907 */
    int32_t levellimit;     /* <0: default 3 - (N > 500)  (:1043-1044) */
    uint32_t algos;         /* SQ_ALGO_* override, 0 = use each paramset's own (:1065-1066) */
    uint64_t priority_mask; /* bit p set: paramset p is prioritised (:912-913) */
} sq_fold_opts;

/* ---- library -------------------------------------------------------------- */
SQ_API int sq_version(void);
SQ_API const char *sq_last_error(void);
/* Status -3 means "a capacity the batch was created with did not hold the fold" (the reference has no capacities: its lists are
 * Python lists, SQRNdbnseq.py:427-495).  sq_last_capacity() says which one the calling thread's last -3 was about, so that a
 * caller can repeat the fold with a larger batch without reading the message:
 *   SQ_CAP_CANDIDATES  candidate records per structure (sq_batch_desc.cand_per_nt)
 *   SQ_CAP_STRUCTS     structure slots / the log of final structures (sq_batch_desc.max_structs)
 *   SQ_CAP_OUTPUT      the output records of a round (sized from the candidate arena: grows with cand_per_nt)
 *   SQ_CAP_FIXED       a limit no descriptor field moves (64 pseudoknot levels, a chain's stem list, the blossom arrays)
 * 0 when the last error was not a capacity. */
#define SQ_CAP_CANDIDATES 1
#define SQ_CAP_STRUCTS 2
#define SQ_CAP_OUTPUT 3
#define SQ_CAP_FIXED 4
SQ_API int sq_last_capacity(void);
/* The library keeps idle pinned host buffers of destroyed batches for the next ones (hipHostMalloc / hipHostFree cost
 * milliseconds; SQ_PINNED_CACHE_MB bounds the cache).  sq_host_cache_trim() gives every idle buffer back to the driver
 * -- what torch.cuda.empty_cache() is for device memory: a process that changes its workload (a bench between its legs,
 * a server between tenants) calls it so that the next batches do not pay for evicting buffers of sizes nobody asks for
 * again.  Returns the number of bytes released.  No reference counterpart (the reference has no device). */
SQ_API long long sq_host_cache_trim(void);

/* ---- batch lifecycle ------------------------------------------------------- */
/* Bytes of device workspace sq_batch_create() needs for this description. */
SQ_API int sq_batch_workspace_bytes(const sq_batch_desc *desc, size_t *bytes);
/* Uploads the O(N) inputs; the N x N matrices are produced on device by sq_bpmatrix_fill. */
SQ_API int sq_batch_create(sq_batch **out, const sq_batch_desc *desc, void *dev_workspace, size_t workspace_bytes,
                    void *hip_stream);
SQ_API void sq_batch_destroy(sq_batch *b);

/* ---- a-1  BPMatrix (SQRNdbnseq.py:258-367) -------------------------------------
 * Fills the fp32 scan matrix of every job (row pitch ld = 32*ceil((N-1)/32)+1 floats,
 * quiet-NaN sentinel where bpboolmatrix == 0).  Asynchronous on the stream. */
SQ_API int sq_bpmatrix_fill(sq_batch *b);
/* Returns job's (bpboolmatrix, bpscorematrix) exactly as the reference would:
 * dense N x N fp64, computed on device in fp64.  Synchronises. */
SQ_API int sq_bpmatrix_read(sq_batch *b, int32_t job, double *boolmat, double *scoremat);

/* ---- a-2..a-6  AnnotateStems / ScoreStems / ChooseStems / OptimalStems ------------
 * (SQRNdbnseq.py:427-495, 607-751, 754-789, 792-833)
 * Evaluates one greedy round for `nstruct` partial structures at once.
 * struct s belongs to job struct_job[s]; its already-selected stems are
 * stems[stem_off[s] .. stem_off[s+1]) (only i, j, len are read).
 * mode 0 (OptimalStems): out receives the stems ChooseStems would return for
 *        subopt[s], in its order, with bpscore and finalscore.
 * mode 1 (AnnotateStems): out receives every stem with len >= minlen and
 *        bpscore >= minbpscore in the reference's emission order
 *        (anti-diagonal i+j ascending, then i ascending); finscore = 0.
 * out_off[nstruct+1] delimits each structure's slice of out[0..out_cap).
 * Synchronises the stream. */
SQ_API int sq_optimal_stems(sq_batch *b, int32_t nstruct, const int32_t *struct_job, const int32_t *stem_off,
                     const sq_stem *stems, const double *subopt, int32_t mode,
                     sq_stem *out, int32_t out_cap, int32_t *out_off);

/* ---- a-8 / a-9 (+ Nussinov)  RunAlgo with Hungarian / Edmonds / Nussinov -------------------
 * (SQRNdbnseq.py:548-595, SQRNalgos.py:44-135).  For each listed job: AnnotateStems with no
 * selected stems, then the matching / DP on the device -- scipy's linear_sum_assignment and
 * networkx's max_weight_matching restated step by step, so ties resolve as in the reference --
 * then RunAlgo's stem filters.  algo is ONE of SQ_ALGO_E / SQ_ALGO_H / SQ_ALGO_N;
 * levellimit < 0 selects the default 3 - (N > 500).  out gets each job's stemset
 * (bpscore = finscore = raw stem score).  Synchronises the stream. */
SQ_API int sq_run_algos(sq_batch *b, int32_t njob, const int32_t *job_ids, int32_t algo, int32_t levellimit,
                        sq_stem *out, int32_t out_cap, int32_t *out_off);

/* ---- a-8 / a-9 at graph level: the reference's SQRNalgos.Hungarian / Edmonds / Nussinov called on their own -----
 * (a maintainer patches `Edmonds(stems)` etc. one for one).  No batch: the inputs are plain host
 * arrays, the results come back in host arrays, `dev_workspace` is caller-owned DEVICE scratch of at least
 * sq_*_workspace_bytes() bytes (256-byte aligned), work is enqueued on hip_stream and the call synchronises it.
 *
 * sq_mwm -- Edmonds (SQRNalgos.py:96-110): networkx.max_weight_matching (3.4.2, maxcardinality=False) of `ngraph`
 * graphs given as weighted edge lists; graph g owns edges [edge_off[g], edge_off[g+1]) of (eu, ev, ew).  Vertex
 * labels are arbitrary non-negative ints (sequence positions in the reference).  As in networkx: nodes are ordered
 * by first appearance, a repeated edge keeps its first position and takes the last weight.  pairs[2k], pairs[2k+1]:
 * graph g's matched pairs are k in [pair_off[g], pair_off[g+1]), each oriented (u, v) as networkx returns it and
 * sorted as Edmonds() sorts them (:109); ties between optimal matchings resolve as in networkx (step-exact). */
SQ_API int sq_mwm_workspace_bytes(int32_t ngraph, const int64_t *edge_off, const int32_t *eu, const int32_t *ev,
                                  size_t *bytes);
SQ_API int sq_mwm(int32_t ngraph, const int64_t *edge_off, const int32_t *eu, const int32_t *ev, const double *ew,
                  int32_t *pairs, int64_t pair_cap, int64_t *pair_off, void *dev_workspace, size_t workspace_bytes,
                  void *hip_stream);
/* sq_lsap -- the assignment step of Hungarian (SQRNalgos.py:119-127): scipy.optimize.linear_sum_assignment(mat)
 * (1.15.3) for `nprob` symmetric n[g] x n[g] matrices that are zero except mat[cv, cw] = mat[cw, cv] = -weight for
 * the listed cells (a repeated cell takes the last weight).  col4row: concatenated, n[g] ints per problem --
 * col4row[r] is the column assigned to row r, the `col_ind` scipy returns (ties resolve as in scipy). */
SQ_API int sq_lsap_workspace_bytes(int32_t nprob, const int32_t *n, const int64_t *cell_off, size_t *bytes);
SQ_API int sq_lsap(int32_t nprob, const int32_t *n, const int64_t *cell_off, const int32_t *cv, const int32_t *cw,
                   const double *weight, int32_t *col4row, void *dev_workspace, size_t workspace_bytes,
                   void *hip_stream);
/* sq_nussinov -- Nussinov + BackTrack (SQRNalgos.py:6-93, minloop = 3) for `nprob` sequences: SCORES[(cv, cw)] =
 * -score for the listed cells (cv < cw); codes: the sequences' letter codes, concatenated (n[g] each; only the
 * separators SQ_CODE_SEP1/2 matter).  pairs / pair_off as for sq_mwm, each problem's pairs sorted (:41). */
SQ_API int sq_nussinov_workspace_bytes(int32_t nprob, const int32_t *n, const int64_t *cell_off, size_t *bytes);
SQ_API int sq_nussinov(int32_t nprob, const int32_t *n, const uint8_t *codes, const int64_t *cell_off,
                       const int32_t *cv, const int32_t *cw, const double *score, int32_t *pairs, int64_t pair_cap,
                       int64_t *pair_off, void *dev_workspace, size_t workspace_bytes, void *hip_stream);

/* ---- a-7 + a-10  greedy pool loop and the ranking tail of SQRNdbnseq ---------------
 * (SQRNdbnseq.py:1048-1286).  Folds every sequence of the batch under its jobs and
 * keeps the per-sequence results inside the batch for the getters below.
 * refs: optional per-sequence known structure as pairs (NULL = no metrics). */
SQ_API int sq_fold(sq_batch *b, const sq_fold_opts *opts, const int32_t *ref_off, const int32_t *ref_pairs,
            const uint8_t *has_ref);

/* The same for several independent batches at once, one host thread per batch: while one batch's host code books a
 * round, the kernels of the others keep the GPU busy (S1000: two batches of 512 fold in 9 ms instead of 12.4 ms as
 * one batch of 1,024).  Give the batches different streams if their kernels should overlap on the GPU as well.
 * ref_off / ref_pairs / has_ref: per batch, as for sq_fold (each entry, or the arrays themselves, may be NULL).
 * Returns the first non-zero status (its text is available from sq_last_error on the calling thread). */
SQ_API int sq_fold_concurrent(sq_batch *const *batches, int32_t nbatch, const sq_fold_opts *opts,
                              const int32_t *const *ref_off, const int32_t *const *ref_pairs, const uint8_t *const *has_ref);
/* The steady-state form: every batch is folded `reps` times back to back by its own host thread, WITHOUT a barrier
 * between the repetitions -- the batches drift apart and overlap each other's host-heavy and GPU-heavy phases (a
 * server that re-uses resident batches for a stream of identical requests; bench.py's timed region is one such call).
 * After the call every batch holds the results of its last fold. */
/* A caller that folds several batches at once from threads of its OWN (a server with a rolling window of requests: each slot
 * creates, folds, reads out and destroys its batches independently, no barrier between them) tells every batch how many are
 * in flight -- what sq_fold_concurrent does for its batches: the host threads then wait for the device with pauses instead of
 * spinning on every CPU, and the worker pools and side streams are sized for a shared chip.  n < 1 counts as 1. */
SQ_API int sq_batch_set_inflight(sq_batch *b, int32_t n);
SQ_API int sq_fold_concurrent_n(sq_batch *const *batches, int32_t nbatch, const sq_fold_opts *opts,
                                const int32_t *const *ref_off, const int32_t *const *ref_pairs, const uint8_t *const *has_ref,
                                int32_t reps);

/* Which driver ran the greedy pool loop of the batch's last fold: 0 the host loop over round kernels, 1 rounds chained on
 * the device (poollim == 1), 2 device pools, 3 device pools that outgrew a capacity and were repeated by the host loop.
 * All give identical results; the number is for tests and tuning (max_structs). */
SQ_API int32_t sq_fold_driver(const sq_batch *b);
/* Which parts of the batch's last fold ran on the device beyond the kernels of a round: bit 0 -- the ranking tail
 * (SQRNdbnseq.py:1201-1286: dedupe, ScoreStruct, RankStructs, bracket rows, consensus, metrics; else the host tail took it:
 * rankbydiff, forced hardrest pairs, conslim > 1, > 4096 final structures of one sequence), bit 1 -- RunAlgo's edge lists and
 * stem filters (SQRNdbnseq.py:548-595; else host-built: reactivity factors / non-dyadic weights on E / H paramsets,
 * sequences above 4096 nt), bit 2 -- the rounds of width-1 pools (driver 1) as ONE launch of the persistent round kernel
 * (SQRNdbnseq.py:1102-1199: a block per structure loops over its own rounds; else one chain of launches per round:
 * jobs with dense matrices, sequences above 8192 nt, SQ_NO_ROUNDS), bit 3 -- a round of the device pools (driver 2) as ONE
 * kernel per structure list + the scan kernel (sequences up to 256 nt with batches in flight or >= 4096 jobs; else state /
 * scan / score / choose / extend kernels), bit 4 -- jobs of wider pools that almost never branch (range factor 1.0, cells from
 * a dense fp64 matrix: the alignment's rows, bpp terms) ran as chains on the persistent round kernel first; the ones that met a
 * tie were folded by the device pools, bit 5 -- the rounds of the device pools were enqueued ahead of the host (a batch alone:
 * every launch covers all structure slots and follows the generation sizes the device publishes; SQ_POOL_AHEAD), bit 6 -- the
 * device pools of sequences of 257-1,024 nt ran the one-wave round kernel over per-job root lists (the runs of the empty
 * structure with their bpscores, checked against every structure's partner array) instead of the launched scan and score
 * kernels (SQ_POOL_ROOT, or bit 7), bit 7 -- ... and every structure read the list its PARENT left (SQ_BATCH_POOL_LISTS: runs,
 * bpscores and the finalscores no strand of the child's stem comes near) in the root list's place, scoring only what the new
 * stem changed, one launch per round.  Identical results either way; for tests and tuning. */
SQ_API int32_t sq_fold_paths(const sq_batch *b);
/* Most structures any round of the batch's last fold evaluated at once (device pools: the largest generation; 0 when the
 * host-driven loop ran).  A host that folds a stream of similar batches sizes max_structs from it. */
SQ_API int64_t sq_fold_peak_structs(const sq_batch *b);

/* Result getters (valid after sq_fold until the next sq_fold / destroy). */
/* k > 0: the getters below (single and bulk) show only the first k structures of every sequence, in rank order -- a
 * caller that prints the top few (RunSQRNdbnseq's outplim, SQRNdbnseq.py:1289-1410) need not fetch a pool of a thousand.
 * k = 0 (default): all of them, as SQRNdbnseq returns them.  Consensus and metrics do not depend on it.  A limit set
 * BEFORE sq_fold also spares the fold the bracket strings of the structures beyond it (most of the ranking tail's time
 * for pools of a thousand); those structures are then not kept, and raising the limit afterwards does not bring them back. */
SQ_API int sq_result_limit(sq_batch *b, int32_t k);
SQ_API int32_t sq_result_nstruct(const sq_batch *b, int32_t seq);
/* levels: per position, 0 = unpaired, +L = opening bracket of level L, -L = closing. */
SQ_API int sq_result_consensus(const sq_batch *b, int32_t seq, int16_t *levels);
SQ_API int sq_result_struct(const sq_batch *b, int32_t seq, int32_t k, int16_t *levels, double scores[3],
                     uint64_t *pset_mask);
SQ_API int sq_result_metrics(const sq_batch *b, int32_t seq, double cons[6], double best[7]);
/* Bulk form of the getters: one buffer per sequence, little-endian, 8-byte aligned sections:
 *   int64  nstruct, n, has_ref, evals
 *   double cons_metrics[6], best_metrics[7], ref_scores[3]   (ref_scores: ScoreStruct of the known structure,
 *                                                              ReferenceScores SQRNdbnseq.py:958-970; NaN without one)
 *   double scores[nstruct][3]
 *   uint64 pset_mask[nstruct]
 *   int16  levels[1 + nstruct][n]      (row 0 = consensus)
 * sq_result_pack_size returns the bytes needed. */
SQ_API int64_t sq_result_pack_size(const sq_batch *b, int32_t seq);
SQ_API int sq_result_pack(const sq_batch *b, int32_t seq, void *buf, int64_t cap);
/* Every sequence of the batch in one call (the payload of the multi-GPU result gather): record s occupies
 * [off[s], off[s+1]) of buf, off has nseq + 1 entries, records start 8-byte aligned. */
SQ_API int64_t sq_result_pack_all_size(const sq_batch *b);
SQ_API int sq_result_pack_all(const sq_batch *b, void *buf, int64_t cap, int64_t *off);
/* The same records WITHOUT a copy, where the device tail wrote them: *buf = the library's pinned host buffer, *off = its
 * nseq + 1 offsets (both owned by the batch, valid until its next sq_fold or sq_batch_destroy; read-only).  Returns 0 and the
 * pointers, or 1 when the last fold's records are not in that form (the host tail ran, or sq_result_limit shows fewer
 * structures than were packed): then sq_result_pack_all forms them.  Replaces the copy a caller of SQRNdbnseq never had to
 * make (the reference returns its tuples by reference, SQRNdbnseq.py:1285-1286). */
SQ_API int sq_result_view(const sq_batch *b, const void **buf, const int64_t **off, int64_t *nbytes);
/* ... and the buffer itself handed over: after sq_result_view returned 0, sq_result_detach makes the records' pinned buffer
 * the CALLER's -- the batch forgets it (and its results: the next fold takes a new buffer), its destruction leaves it alone --
 * until sq_buffer_release returns it to the library's pinned cache.  For a caller that keeps the records beyond the batch
 * (the results of a Python call outlive the batch that made them: 544 MB per thousand 500-nt records under pools of a
 * thousand were copied record by record, a quarter of the call).  Copy the offsets first: they stay the batch's. */
SQ_API int sq_result_detach(sq_batch *b, void **buf, int64_t *nbytes);
SQ_API void sq_buffer_release(void *buf);
/* The same results as pair tables in the CALLER's device memory (no reference counterpart: a caller of SQRNdbnseq parses
 * the bracket strings, DBNToPairs SQRNdbnseq.py:172-207) -- for code that goes on with them on the same GPU.  Field by field
 * what sq_result_pack holds, brackets replaced by partners:
 *   d_partner    int32: record s has 1 + nstruct[s] rows of n[s] entries from d_partner[d_cell_off[s]] on; row 0 is the
 *                consensus (the top structure when the fold's conslim was 1; all -1 when it was 0 or the record has no
 *                structure), rows 1.. the shown structures in rank order; entry i = the 0-based partner of position i, or
 *                -1 (gap-free coordinates, as in the packed records)
 *   d_scores     double[rows][3], d_pset_mask uint64[rows]: the structure rows only, record s from row d_row_off[s] on
 *   d_metrics    double[nseq][16]: cons_metrics[6], best_metrics[7], ref_scores[3] (NaN without a known structure)
 *   d_row_off, d_cell_off   int64[nseq + 1]: written here, the totals last
 * nstruct[s] = d_row_off[s + 1] - d_row_off[s] is what sq_result_nstruct reports (sq_result_limit as for the packed getters).
 * sq_result_pairs_size gives the totals a caller sizes its buffers with: rows = sum of nstruct, cells = sum of (1 + nstruct) n.
 * Both return 0, or 1 when the last fold's results are not in the device tail's form -- the host tail ran (sq_fold_paths
 * bit 0 clear), sq_result_limit shows fewer structures than were packed, or sq_result_detach took the records away: the
 * caller then reads the packed records --, or -1 (bad argument; a capacity below what sq_result_pairs_size reports:
 * nothing is written, sq_last_error names the sizes).  Not -3: that status is about the capacities a BATCH was created with
 * (sq_last_capacity) and makes a caller repeat the fold with a larger batch, which does not help a buffer of the caller's;
 * and not -(needed): two sizes are needed.  sq_result_pairs_size is the way to learn them -- call it first.
 * The rows are formed by a kernel from the scratch the ranking tail left in the batch's workspace; nothing but the next
 * sq_fold of the batch writes that scratch (no other entry point recycles it), so the call is valid, any number of times,
 * from the return of sq_fold until the batch's next sq_fold or its destruction.  The library allocates nothing.
 * Asynchronous: the work is enqueued on hip_stream (NULL: the batch's stream) and the call does not wait for it; it must
 * be complete before the batch folds again. */
SQ_API int sq_result_pairs_size(const sq_batch *b, int64_t *rows, int64_t *cells);
SQ_API int sq_result_pairs_dev(sq_batch *b, int32_t *d_partner, int64_t cells_cap, double *d_scores, uint64_t *d_pset_mask,
                               int64_t rows_cap, double *d_metrics, int64_t *d_row_off, int64_t *d_cell_off, void *hip_stream);
/* Dot-bracket rows of every record as ASCII text: record s occupies [off[s], off[s+1]) of buf with its consensus row
 * and then its nstruct structure rows, n characters each (gap-free coordinates; gap columns and separators are
 * re-inserted by the caller, SQRNdbnseq.py:1239-1246).  Levels 1..30 print as ( [ { < A..Z and ) ] } > a..z (:107-112);
 * deep[s] = 1 when record s uses a deeper level (the reference continues with Cyrillic letters): use the level form
 * (sq_result_pack) for those. */
SQ_API int64_t sq_result_dbn_all_size(const sq_batch *b);
SQ_API int sq_result_dbn_all(const sq_batch *b, char *buf, int64_t cap, int64_t *off, uint8_t *deep);
/* ---- text of the drop-in layer (per-record work of RunSQRNdbnseq, in C++ because a batch has thousands of records) ----
 * sq_dbn_pairs: DBNToPairs (SQRNdbnseq.py:172-207) for nrec dot-bracket lines: line r = text[off[r], off[r+1]); brackets
 * ( ) [ ] { } < > A..Z / a..z, unmatched closers ignored; line r's pairs, sorted, at pairs[2 pair_off[r] .. 2 pair_off[r+1]). */
SQ_API int sq_dbn_pairs(const char *text, const int64_t *off, int32_t nrec, int32_t *pairs, int64_t pair_cap, int64_t *pair_off);
/* sq_write_blocks: the output block of RunSQRNdbnseq (SQRNdbnseq.py:1301-1406: name, sequence, optional reactivities /
 * restraints / reference lines, the consensus line, up to outplim structure lines with scores, paramset names and metrics)
 * for every record of a batch whose last fold left packed results (sq_fold_paths bit 0).  The per-record input lines come
 * '\n'-joined, one line per record in batch order (an empty line: the record has none; a NULL field: no record has one);
 * seqs are the INPUT sequences (gap columns and separators included: they are re-inserted into every bracket row,
 * :1239-1246); reacts the already encoded reactivity lines (EncodedReactivities, :82-101).  Record r's block is
 * buf[off[r], off[r+1]); skipped[r] = 1: the record uses bracket levels beyond the ASCII alphabet, its block is empty and
 * left to the caller.  Returns the bytes written, or -(bytes needed + 16) when cap is too small (nothing written). */
typedef struct sq_block_desc {
    int32_t nrec;
    const char *names, *seqs, *reacts, *restr, *refs;
    const int32_t *nameset;         /* [nrec] which list of paramset names a record prints (NULL: list 0)      */
    const char *const *psnames;     /* [nsets] the names of a configuration's paramsets, '\n'-joined            */
    int32_t nsets, conslim, outplim;
} sq_block_desc;
SQ_API int64_t sq_write_blocks(const sq_batch *b, const sq_block_desc *d, char *buf, int64_t cap, int64_t *off, uint8_t *skipped);

/* sq_parse_default -- the record scan of the reference's default input format (SQUARNA.py:80-203, ParseDefaultInput) over
 * the bytes of a file: a '>' line names a record, the lines behind it are its fields in the order of `inputformat`
 * (nfields letters; q_ind / t_ind / r_ind / f_ind: the positions of q, t, r, f in it, -1 when absent; as in the reference
 * a t / r / f at position 0 is not read).  out[rec][10] = offset, length of: the stripped name line, the sequence token,
 * the stripped reactivities line, the restraints token, the reference token (length -1: None; restraints / reference
 * also for an empty line).  Returns the number of records, or -1 when the file needs the general parser: default lines
 * in front of the first record, a byte outside ASCII, NUL or '\r', a record without a sequence token, more than cap
 * records.  Host code; values are not validated here (lengths, reactivities): the caller's checks stay the reference's. */
/* sq_align_first_fit -- the first structure of MatrixToDBNs (SQRNdbnali.py:121-192, the one its caller keeps, :242): the cells
 * flat[k] = v * N + w, given in decreasing order of value (ties: flat index ascending), are taken one by one; a cell of span
 * >= minspan whose columns are both free joins.  pairs: up to cap (v, w) pairs in the order taken; returns their number. */
SQ_API int64_t sq_align_first_fit(const int64_t *flat, int64_t n, int32_t N, int32_t minspan, int32_t *pairs, int64_t cap);
SQ_API int64_t sq_parse_default(const char *text, int64_t len, int32_t nfields, int32_t q_ind, int32_t t_ind, int32_t r_ind,
                                int32_t f_ind, int64_t *out, int64_t cap);

/* R = number of AnnotateStems evaluations the reference algorithm performs for this sequence. */
SQ_API int64_t sq_result_evals(const sq_batch *b, int32_t seq);

/* ---- alignment step 1 (SQRNdbnali.py:60-108, 211-242) ------------------------------------
 * For each listed job, in order: AnnotateStems with no selected stems, then
 *   matrix[cols[v], cols[w]] += stem score;  matrix[cols[w], cols[v]] += stem score
 * for every base pair (v, w) of every stem -- the parent-side loop of SQRNdbnali (:233-237).
 * cols[col_off[k] + p] is the alignment column of position p of job_ids[k] (ReAlignDict, :20-37).
 * d_matrix: caller-owned DEVICE memory, L x L fp64 row-major, accumulated into: zero it first, then pass
 * the same matrix to as many calls as the alignment needs.  Both additions of a pair are the same number
 * in the same order, so the library accumulates the upper triangle and copies it onto the lower one at the
 * end of every call (the lower triangle of the input is overwritten).
 * A cell receives at most one addition per sequence and sequences are applied in list order, so
 * every cell sees the reference's fp64 summation order (when every sum is exact anyway -- pair weights
 * that are multiples of 2^-10, no reactivities -- the sequences of a chunk are added in one launch).
 * The matrix is complete when the call returns. */
SQ_API int sq_align_accumulate(sq_batch *b, int32_t njob, const int32_t *job_ids, const int32_t *col_off,
                               const int32_t *cols, int32_t L, double *d_matrix);
/* Cells (v, w) of a device L x L fp64 matrix with w - v >= minspan and value >= threshold
 * (MatrixToDBNs' candidates, SQRNdbnali.py:127-148).  All buffers are caller-owned DEVICE memory:
 * d_idx[cap] (flat indices v*L+w), d_val[cap], d_count[1] (zeroed here; may end up > cap, then only
 * the first cap hits were stored).  Unordered.  Asynchronous on hip_stream. */
SQ_API int sq_colmatrix_select(const double *d_matrix, int32_t L, double threshold, int32_t minspan,
                               int64_t *d_idx, double *d_val, int64_t cap, uint64_t *d_count, void *hip_stream);

/* ---- alignment consensus on the device (SQRNdbnali.py:121-192, 271-304) -------------------------------
 * sq_align_pair_count -- Consensus' dict (:281-284) from the pair tables of a fold.  d_partner / d_cell_off: the layout of
 * sq_result_pairs_dev (gap-free coordinates); row 0 of each of the nrec records -- its consensus -- is read.  d_col_off
 * int32[nrec + 1] / d_cols: the records' gap maps in sq_align_accumulate's form, in DEVICE memory: d_cols[d_col_off[r] + p] is
 * the alignment column of position p of record r, and d_col_off[r + 1] - d_col_off[r] the record's length.  Every pair
 * (i, j), i < j, becomes the column pair (v, w); for every distinct one, count = the number of records that hold it and
 * first = the smallest index of such a record.  The distinct pairs with count >= threshold (>= 1) are written, unordered, as
 * d_flat[k] = v * L + w, d_count[k], d_first[k]; d_out[0] = their number (may exceed cap: then only the first cap were
 * stored, as for sq_colmatrix_select), d_out[1] = 0, or 2 when a table entry pointed outside its record or the L columns
 * (such an entry is not counted).  d_scratch: sq_align_pair_count_scratch(L) bytes (two dense int32 L x L tables), set here.
 * sq_first_fit_dev -- the sequential pass of sq_align_first_fit / Consensus (:285-295) over d_flat[n], candidates v * L + w
 * given in rank order: a candidate with v < w and w - v >= minspan is taken iff both of its columns are still free.
 * d_partner int32[L]: the partner of every column, -1 where free.  d_info int32[4]: status (0, or 1: more than L / 2 + 1
 * rounds -- cannot happen, the loop is bounded by it; the result is then incomplete), the rounds used, the pairs taken,
 * candidates left live (0 with status 0).  One launch of one workgroup (rounds: csrc/sq_firstfit.h).  d_scratch:
 * sq_first_fit_scratch(n, L) bytes.
 * Both are asynchronous on hip_stream and allocate nothing; 0, or -1 (bad argument, scratch too small: nothing enqueued). */
SQ_API size_t sq_align_pair_count_scratch(int32_t L);
SQ_API int sq_align_pair_count(const int32_t *d_partner, const int64_t *d_cell_off, const int32_t *d_col_off, const int32_t *d_cols,
                               int32_t nrec, int32_t L, int32_t threshold, void *d_scratch, size_t scratch_bytes, int64_t *d_flat,
                               int32_t *d_count, int32_t *d_first, int64_t cap, uint64_t *d_out, void *hip_stream);
SQ_API size_t sq_first_fit_scratch(int64_t n, int32_t L);
SQ_API int sq_first_fit_dev(const int64_t *d_flat, int64_t n, int32_t L, int32_t minspan, int32_t *d_partner, void *d_scratch,
                            size_t scratch_bytes, int32_t *d_info, void *hip_stream);

/* ---- pair counts over sliding windows (FoldWindows) ---------------------------------------------------
 * The windows of long sequences lie on one axis of Ltot (<= 2^31 - 1) positions on which the records follow one another:
 * window k covers [d_start[k], d_start[k] + d_len[k]), d_start int64[nwin] non-decreasing (so are the ends), and its
 * structure is row 0 of record rec0 + k of the pair tables d_partner / d_cell_off (sq_result_pairs_dev's layout; d_cell_off
 * holds at least rec0 + nwin + 1 offsets), in the window's own coordinates.  For every distinct pair gi < gj of axis positions
 * that any window's row holds, one record is written, unordered: d_flat = gi * Ltot + gj, d_count = the windows that hold
 * the pair, d_cover = the windows that contain both positions, d_first = the smallest k of a holder.  The first holder
 * forms the record from its neighbours' rows (csrc/sq_windows.h): no dense table, no scratch, no atomics on data.
 * d_out[0] = the number of distinct pairs (may exceed cap: then only cap were stored and nothing is written beyond cap),
 * d_out[1] = 0, or 2 when an entry was invalid -- a partner outside [-1, len), the position itself or one that does not
 * point back, a window outside the axis or longer than its table -- (such an entry is not counted).
 * Asynchronous on hip_stream, allocates nothing; 0, or -1 (bad argument: nothing enqueued). */
SQ_API int sq_window_pair_count(const int32_t *d_partner, const int64_t *d_cell_off, int32_t rec0, int32_t nwin, const int64_t *d_start,
                                const int32_t *d_len, int64_t Ltot, int64_t *d_flat, int32_t *d_count, int32_t *d_cover,
                                int32_t *d_first, int64_t cap, uint64_t *d_out, void *hip_stream);

/* ---- structure change of sequence variants (FoldMutants) -----------------------------------------------
 * The pair tables d_partner / d_cell_off / d_lengths (sq_result_pairs_dev's layout; at least rec0 + nvar records) hold wild
 * types among the first rec0 records and their substitution variants behind them: variant m is record rec0 + m, its wild
 * type is record d_wt_rec[m] in [0, rec0), of the same length n, and both are read at row 0 (the consensus row).  The wild
 * types lie on one axis of Ltot (<= 2^31 - 1) positions: record r's positions start at d_pos_off[r] (int64, at least rec0
 * entries; only the entries d_wt_rec names are read).
 * d_diff int32[nvar * 6], per variant: the wild type's pairs it lacks, its pairs the wild type lacks, the pairs of both, the
 * positions whose partner differs, the lowest and the highest of them (-1, -1 without one).  d_pos_changed int32[Ltot]:
 * per wild-type position the variants of its record whose partner there differs (cleared by the call, then added to).
 * d_out[0] = 0, d_out[1] = 0, or 2 when a variant was invalid -- d_wt_rec outside [0, rec0), lengths that differ, a row
 * longer than its table or outside the axis, a partner outside [-1, n), the position itself or one that does not point
 * back --: that variant's six numbers and its additions to d_pos_changed are then unspecified, every other variant's are
 * right, and no read leaves the two rows (csrc/sq_variants.h).
 * One wave per variant.  Asynchronous on hip_stream, allocates nothing; 0, or -1 (bad argument: nothing enqueued; pointers
 * that only variants need may be null when nvar = 0). */
SQ_API int sq_variant_diff(const int32_t *d_partner, const int64_t *d_cell_off, const int64_t *d_lengths, int32_t rec0, int32_t nvar,
                           const int32_t *d_wt_rec, const int64_t *d_pos_off, int64_t Ltot, int32_t *d_diff, int32_t *d_pos_changed,
                           uint64_t *d_out, void *hip_stream);

/* ---- what two chains do to one another (FoldDuplex) --------------------------------------------------------
 * Two sets of pair tables in sq_result_pairs_dev's layout, which may be one allocation: nsolo records folded alone
 * (d_partner_s / d_cell_off_s / d_lengths_s) and ndup duplex records (d_partner_d / d_cell_off_d / d_lengths_d).  Duplex k is
 * the chain of solo record d_a_rec[k] (nA positions), one separator column and the chain of solo record d_b_rec[k] (nB
 * positions), both int32 in [0, nsolo) and possibly the same record: its row has nA + 1 + nB entries, entry nA the
 * separator.  All rows are read at row 0 (the consensus row).  The solo records lie on one axis of Ltot (<= 2^31 - 1)
 * positions: record r's positions start at d_pos_off[r] (int64[nsolo + 1]).
 * d_summary int32[ndup * 9], per duplex, pairs counted at their 5' ends: the pairs between the chains, the pairs inside
 * chain A, inside chain B, the pairs of A alone whose 5' end has another partner or none in the duplex, the same for B (a
 * partner q of B alone corresponds to q + nA + 1), the lowest and the highest position of A with a partner in B, the same
 * for B in B's own coordinates (-1, -1 without one).  d_bound int32[Ltot]: per solo position the duplexes in which it
 * pairs across the separator, in either role (cleared by the call, then added to).
 * d_out[0] = 0, d_out[1] = 0, or 2 when a duplex was invalid -- a chain outside [0, nsolo), a duplex row that is not
 * nA + 1 + nB entries long, a row longer than its table or outside the axis, a paired separator column, a partner outside
 * [-1, its row's length), the position itself or one that does not point back --: that duplex's nine numbers and its
 * additions to d_bound are then unspecified, every other duplex's are right, and no read leaves the three rows
 * (csrc/sq_duplex.h).
 * One wave per duplex.  Asynchronous on hip_stream, allocates nothing; 0, or -1 (bad argument: nothing enqueued; pointers
 * that only duplexes need may be null when ndup = 0, which clears d_out and d_bound). */
SQ_API int sq_duplex_summary(const int32_t *d_partner_s, const int64_t *d_cell_off_s, const int64_t *d_lengths_s, int32_t nsolo,
                             const int32_t *d_partner_d, const int64_t *d_cell_off_d, const int64_t *d_lengths_d, int32_t ndup,
                             const int32_t *d_a_rec, const int32_t *d_b_rec, const int64_t *d_pos_off, int64_t Ltot,
                             int32_t *d_summary, int32_t *d_bound, uint64_t *d_out, void *hip_stream);

/* ---- covariation evidence for alignment columns (Covariation) ----------------------------------------------
 * d_rows uint8[R * L]: the ASCII rows of an alignment of R rows and L columns, row after row.  A byte is upper-cased and T
 * reads as U; it is then A, C, G, U, a gap ('-', '.', '~') or "other".  For columns v < w, over the rows: c[t] = the rows
 * whose two letters are the pair type t of AU UA GC CG GU UG (in this order), both_gap = the rows with a gap in both columns,
 * and cov = the sum over t < t' of c[t] * c[t'] * d(t, t') with d the Hamming distance of the two two-letter strings -- the
 * sum, over the unordered pairs of rows that both hold a canonical pair, of the distance of their pairs.  A record is the
 * seven int32 counts (c[0..5], both_gap) and cov (int64); bp_rows = the sum of c, incompatible = R - bp_rows - both_gap.
 * Both entries first write the rows as five bit planes of 64 rows per word into d_scratch (sq_covariation_scratch(R, L)
 * bytes, 8-byte aligned; csrc/sq_covar.h has the layout).
 * sq_covariation_scan: every cell with w - v >= minspan, as an all-pairs scan in tiles of columns from LDS; a cell with
 * bp_rows >= min_rows and cov >= min_cov leaves one record, unordered: d_flat = v * L + w, d_counts[7], d_cov.
 * d_out[0] = the number of such cells (may exceed cap: then only cap were stored and nothing is written beyond cap),
 * d_out[1] = 0.
 * sq_covariation_pairs: the records of the P column pairs d_pairs int32[P * 2] = (v, w), in their order.  d_out[0] = 0,
 * d_out[1] = 0, or 2 when a pair was not 0 <= v < w < L: that pair's record is all zero, every other record is right.
 * Asynchronous on hip_stream, allocate nothing; 0, or -1 (a null pointer, R < 1, L < 1, scratch too small, a negative
 * minspan, threshold, cap or P: nothing enqueued; the record pointers may be null when cap or P is 0). */
SQ_API size_t sq_covariation_scratch(int32_t R, int32_t L);
SQ_API int sq_covariation_scan(const uint8_t *d_rows, int32_t R, int32_t L, int32_t minspan, int32_t min_rows, int64_t min_cov,
                               void *d_scratch, size_t scratch_bytes, int64_t *d_flat, int32_t *d_counts, int64_t *d_cov, int64_t cap,
                               uint64_t *d_out, void *hip_stream);
SQ_API int sq_covariation_pairs(const uint8_t *d_rows, int32_t R, int32_t L, const int32_t *d_pairs, int64_t P, void *d_scratch,
                                size_t scratch_bytes, int32_t *d_counts, int64_t *d_cov, uint64_t *d_out, void *hip_stream);

/* ---- covariation statistics of alignment columns (CovariationStatistics) ------------------------------------
 * d_rows as above.  For columns v < w the joint table n[a * 4 + b] (int32, a, b in A C G U) = the rows with residue a at v
 * and b at w; rows with a gap or "other" at either column take part in nothing.  N = the sum of n, na / nb its marginals.
 * statistic 0 / 1 / 2 = mi / gt / chi: S = the sum over n > 0 of (n / N) ln(n N / (na nb)); 2 * the sum over n > 0 of
 * n ln(n N / (na nb)); the sum over na nb > 0 of (n - e)^2 / e with e = na nb / N.  S = 0 when N = 0 (csrc/sq_covar_stat.h).
 * correction 0 / 1 / 2 = none / apc / asc, from the means over every pair of distinct columns (no minspan, no threshold):
 * mean[c] = the sum over c' != c of S(c, c') / (L - 1), mean_all = the mean of S over v < w.  apc: C = S - mean[v] mean[w] /
 * mean_all (S when mean_all = 0); asc: C = S - (mean[v] + mean[w] - mean_all); none: C = S.  With a correction d_mean
 * double[L + 1] receives mean[0 .. L - 1] and mean_all at [L], by a first pass over every cell whose sums have a fixed order
 * (no float atomics: two calls give the same bits); with none d_mean may be null and the pass is skipped.
 * A record is n[16], S (d_raw) and C (d_value).  d_scratch: sq_covariation_stat_scratch(R, L) bytes, 8-byte aligned (the bit
 * planes and the first pass's partial column sums, ceil(L / 32) x (L rounded up to 64) doubles).
 * sq_covariation_stat_scan: every cell with w - v >= minspan, N >= min_rows and C >= min_stat (-infinity: every C) leaves one
 * record, unordered, d_flat = v * L + w.  d_out[0] = the number of such cells (may exceed cap: then only cap were stored and
 * nothing is written beyond cap), d_out[1] = 0.
 * sq_covariation_stat_pairs: the records of the P column pairs d_pairs int32[P * 2] = (v, w), in their order.  d_out[0] = 0,
 * d_out[1] = 0, or 2 when a pair was not 0 <= v < w < L: that pair's record is all zero, every other record is right.
 * Asynchronous on hip_stream, allocate nothing; 0, or -1 (a null pointer, R < 1, L < 1, an unknown statistic or correction,
 * scratch too small, a negative minspan, min_rows, cap or P, a NaN min_stat: nothing enqueued; the record pointers may be
 * null when cap or P is 0). */
SQ_API size_t sq_covariation_stat_scratch(int32_t R, int32_t L);
SQ_API int sq_covariation_stat_scan(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction, int32_t minspan,
                                    int32_t min_rows, double min_stat, void *d_scratch, size_t scratch_bytes, double *d_mean,
                                    int64_t *d_flat, int32_t *d_joint, double *d_raw, double *d_value, int64_t cap, uint64_t *d_out,
                                    void *hip_stream);
SQ_API int sq_covariation_stat_pairs(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction,
                                     const int32_t *d_pairs, int64_t P, void *d_scratch, size_t scratch_bytes, double *d_mean,
                                     int32_t *d_joint, double *d_raw, double *d_value, uint64_t *d_out, void *hip_stream);

/* ---- covariation statistics with a weight per row (CovariationStatistics(weights=)) ------------------------------
 * The two entries above with d_weights double[R], one weight per row: finite, 0 <= w <= 2048; R <= 2^22.  A weight is
 * quantised once, q = rint(w * 2^20) (ties to even), and the joint table is Q[a * 4 + b] (int64) = the sum of q over the rows
 * with residue a at v and b at w: integer sums, exact and the same in two calls; the weighted count is Q / 2^20.  The
 * statistics, the means and the corrections are those above on x = Q / 2^20 as doubles (csrc/sq_covar_wstat.h: with integer
 * weights the bits of the unweighted entries on the repeated rows).  A record is Q[16] (d_joint int64[cap * 16]), S and C.
 * d_scratch: sq_covariation_wstat_scratch(R, L) bytes, 8-byte aligned (the scratch above and q).
 * sq_covariation_wstat_scan: every cell with w - v >= minspan, N = (the sum of Q) / 2^20 >= min_rows and C >= min_stat leaves
 * one record; d_out as above, but d_out[1] = 3 when a weight was not such a number (it then counted as 0).
 * sq_covariation_wstat_pairs: the records of the P given pairs; d_out[1] = 0, 2 (a pair was not 0 <= v < w < L) or 3.
 * Asynchronous on hip_stream, allocate nothing; 0, or -1 as above, also for a null d_weights, R > 2^22 and a negative or NaN
 * min_rows: nothing enqueued. */
SQ_API size_t sq_covariation_wstat_scratch(int32_t R, int32_t L);
SQ_API int sq_covariation_wstat_scan(const uint8_t *d_rows, int32_t R, int32_t L, const double *d_weights, int32_t statistic,
                                     int32_t correction, int32_t minspan, double min_rows, double min_stat, void *d_scratch,
                                     size_t scratch_bytes, double *d_mean, int64_t *d_flat, int64_t *d_joint, double *d_raw,
                                     double *d_value, int64_t cap, uint64_t *d_out, void *hip_stream);
SQ_API int sq_covariation_wstat_pairs(const uint8_t *d_rows, int32_t R, int32_t L, const double *d_weights, int32_t statistic,
                                      int32_t correction, const int32_t *d_pairs, int64_t P, void *d_scratch, size_t scratch_bytes,
                                      double *d_mean, int64_t *d_joint, double *d_raw, double *d_value, uint64_t *d_out,
                                      void *hip_stream);

/* ---- the shuffled-column null of cov (CovariationSignificance) ---------------------------------------------------------
 * Sample k of K permutes the rows of every column of the alignment on its own: row r of column c gets the key
 * z = seed + 0x9E3779B97F4A7C15 * (1 + ((k * L + c) * R + r)) mod 2^64, the splitmix64 finaliser, (z & ~0xFFFF) | r, and row j
 * of the shuffled column holds the class of the row with the j-th smallest key (csrc/sq_covar_null.h).  The in-scope cells
 * of a sample are the v < w < L with w - v >= minspan; their covs are the null.
 * sq_covariation_null: d_pairs int32[P * 2] and d_cov int64[P] are the observed pairs and their cov, d_thresholds int64[U]
 * sorted distinct values (for CovariationSignificance those of d_cov).  Outputs: d_hist int64[U + 1], d_hist[b] = the null cells of all K samples with
 * exactly b thresholds <= their cov; d_own_ge int32[P], the samples in which the cell of pair p has cov >= d_cov[p];
 * d_null_max int64[K], the largest cov of a sample's cells (0 without a cell).  d_out[0] = 0, d_out[1] = 0, or 2 when a pair
 * was not 0 <= v < w < L (it counts nothing).  The samples are formed `batch` at a time in d_scratch
 * (sq_covariation_null_scratch(R, L, batch) bytes, 8-byte aligned: the bit planes of `batch` shuffled alignments and the
 * class bytes of the rows); the results do not depend on batch.
 * sq_covariation_null_planes: the planes of the samples k .. k + count - 1 alone, one after the other at the front of d_scratch
 * (sq_covariation_null_scratch(R, L, count) bytes; layout of a sample's planes: csrc/sq_covar.h).
 * Asynchronous on hip_stream, allocate nothing; 0, or -1 (a null pointer, R < 1, L < 1, K < 1, k < 0, batch or count outside 1..65535,
 * a negative minspan, P or U, R above SQ_COVNULL_MAX_ROWS = 4096, L above 2^21, scratch too small: nothing enqueued;
 * the pair pointers may be null when P is 0, d_thresholds when U is 0). */
SQ_API size_t sq_covariation_null_scratch(int32_t R, int32_t L, int32_t batch);
SQ_API int sq_covariation_null(const uint8_t *d_rows, int32_t R, int32_t L, int32_t minspan, const int32_t *d_pairs, const int64_t *d_cov,
                               int64_t P, const int64_t *d_thresholds, int64_t U, int32_t K, uint64_t seed, int32_t batch, void *d_scratch,
                               size_t scratch_bytes, int64_t *d_hist, int32_t *d_own_ge, int64_t *d_null_max, uint64_t *d_out,
                               void *hip_stream);
SQ_API int sq_covariation_null_planes(const uint8_t *d_rows, int32_t R, int32_t L, int64_t k, int32_t count, uint64_t seed,
                                      void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* ---- the shuffled-column null of the covariation statistics (CovariationStatisticsSignificance) ------------------------
 * The shuffle of sq_covariation_null and the statistics of sq_covariation_stat_scan (statistic 0 / 1 / 2 = mi / gt / chi,
 * correction 0 / 1 / 2 = none / apc / asc): the value of a null cell v < w < L, w - v >= minspan, of sample k is C with
 * the column means of that shuffled sample over every pair of its distinct columns -- the bits sq_covariation_stat_scan gives
 * for the shuffled alignment (csrc/sq_covar_stat_null.h).
 * sq_covariation_stat_null: d_pairs int32[P * 2] and d_value double[P] are the observed pairs and their C, d_thresholds
 * double[U] sorted distinct values without a NaN (for CovariationStatisticsSignificance those of d_value).  Outputs: d_hist
 * int64[U + 1], d_hist[b] = the null cells of all K samples with exactly b thresholds <= their C (IEEE comparisons);
 * d_own_ge int32[P], the samples in which the cell of pair p has C >= d_value[p]; d_null_max double[K], the largest C of a
 * sample's cells (-infinity without a cell; folded through an integer key, no float atomics: two calls give the same
 * bits).  d_out[0] = 0, d_out[1] = 0, or 2 when a pair was not 0 <= v < w < L (it counts nothing).  The samples are formed
 * `batch` at a time in d_scratch (sq_covariation_stat_null_scratch(R, L, batch) bytes, 8-byte aligned: per sample of a batch
 * the bit planes, the first pass's partial column sums and L + 1 means, then the class bytes of the rows); the results do
 * not depend on batch.
 * Asynchronous on hip_stream, allocate nothing; 0, or -1 (a null pointer, R < 1, L < 1, K < 1, an unknown statistic or
 * correction, batch outside 1..65535, a negative minspan, P or U, R above SQ_COVNULL_MAX_ROWS = 4096, L above 2^21, scratch
 * too small: nothing enqueued; the pair pointers may be null when P is 0, d_thresholds when U is 0). */
SQ_API size_t sq_covariation_stat_null_scratch(int32_t R, int32_t L, int32_t batch);
SQ_API int sq_covariation_stat_null(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction, int32_t minspan,
                                    const int32_t *d_pairs, const double *d_value, int64_t P, const double *d_thresholds, int64_t U,
                                    int32_t K, uint64_t seed, int32_t batch, void *d_scratch, size_t scratch_bytes, int64_t *d_hist,
                                    int32_t *d_own_ge, double *d_null_max, uint64_t *d_out, void *hip_stream);

/* ---- the shuffled-column null of the weighted covariation statistics (CovariationStatisticsSignificance(weights=)) ------
 * sq_covariation_stat_null with the joint tables of sq_covariation_wstat_scan: d_weights double[R], each finite and in
 * 0 .. 2048, quantised once as there.  The weights belong to the row slots: sample k permutes the rows of every column as
 * sq_covariation_null does and row r keeps its weight, so a null cell's value is the C that sq_covariation_wstat_scan gives
 * for the shuffled rows and the same weights, bit for bit (csrc/sq_covar_wstat_null.h).  A row of weight 0 is shuffled and
 * counts nothing.  Every other argument, output and error is sq_covariation_stat_null's; d_out[1] = 0, 2 (a pair was not
 * 0 <= v < w < L; it counts nothing) or 3 (a weight was not a finite number in 0 .. 2048; it counts as 0).  The scratch
 * (sq_covariation_wstat_null_scratch(R, L, batch) bytes) is that of sq_covariation_stat_null, then the quantised weights. */
SQ_API size_t sq_covariation_wstat_null_scratch(int32_t R, int32_t L, int32_t batch);
SQ_API int sq_covariation_wstat_null(const uint8_t *d_rows, int32_t R, int32_t L, int32_t statistic, int32_t correction, int32_t minspan,
                                     const int32_t *d_pairs, const double *d_value, int64_t P, const double *d_thresholds, int64_t U,
                                     int32_t K, uint64_t seed, int32_t batch, void *d_scratch, size_t scratch_bytes, int64_t *d_hist,
                                     int32_t *d_own_ge, double *d_null_max, uint64_t *d_out, void *hip_stream, const double *d_weights);

/* ---- row identities, neighbour counts and the redundancy filter of an alignment (RowIdentity) ----------------------------
 * d_rows uint8[R * L] as for the covariation entries, the bytes classified in the same way; a residue is any non-gap, a base
 * is A, C, G or U, and "other" matches nothing.  For rows a, b: same[a, b] = the columns where both hold the same base,
 * both[a, b] = the columns where both hold a residue, len[a] = both[a, a], bases[a] = same[a, a].  The denominator den(a, b)
 * is min(len[a], len[b]) (denominator 0, "shorter"), both[a, b] (1, "aligned") or L (2, "columns"); rows a != b are neighbours
 * iff den > 0 and same * 10000 >= threshold_bp * den, in int64.  Outputs: d_len, d_bases, d_neighbours int32[R]
 * (neighbours[a] = 1 + the neighbours of a), d_keep uint8[R] (the greedy filter in row order: row a is kept iff no kept row
 * b < a is its neighbour), and d_same, d_both int32[R * R] (symmetric, the diagonal included), which may both be null: then no
 * matrix is written.  d_out[0] = d_out[1] = 0.  d_scratch (sq_row_identity_scratch(R, L) bytes, 8-byte aligned; 0 for sizes
 * the entry refuses) holds the rows as four bit planes of 64 columns per word and the neighbour bit matrix
 * uint64[R * ceil(R / 64)] (csrc/sq_identity.h has both layouts).  Three kernels, one after the other: the planes, all pairs
 * of rows in tiles of 64 x 64 from LDS, the filter as one wave.
 * Asynchronous on hip_stream, allocates nothing; 0, or -1 (a null pointer other than the two matrices, exactly one of the
 * two matrices, R < 1, L < 1, R above SQ_ID_MAX_ROWS = 65535, L above 2^21, a denominator outside 0..2, threshold_bp outside
 * 0..10000, scratch too small: nothing enqueued, nothing written).
 * sq_row_identity_phases: the same call with only the kernels of `phases` (bit 0: the planes with len and bases, bit 1: all
 * pairs, bit 2: the filter; 1..7, else -1) on buffers that hold what the earlier phases left: for measuring a kernel alone. */
SQ_API size_t sq_row_identity_scratch(int32_t R, int32_t L);
SQ_API int sq_row_identity(const uint8_t *d_rows, int32_t R, int32_t L, int32_t denominator, int32_t threshold_bp, void *d_scratch,
                           size_t scratch_bytes, int32_t *d_len, int32_t *d_bases, int32_t *d_same, int32_t *d_both,
                           int32_t *d_neighbours, uint8_t *d_keep, uint64_t *d_out, void *hip_stream);
SQ_API int sq_row_identity_phases(int32_t phases, const uint8_t *d_rows, int32_t R, int32_t L, int32_t denominator, int32_t threshold_bp,
                                  void *d_scratch, size_t scratch_bytes, int32_t *d_len, int32_t *d_bases, int32_t *d_same,
                                  int32_t *d_both, int32_t *d_neighbours, uint8_t *d_keep, uint64_t *d_out, void *hip_stream);

/* ---- base-pair distances, neighbour counts and the greedy filter of structures (Distances) --------------------------------
 * S structure rows: row q is the row_width[q] partners at d_partner[row_start[q] ..] (int32[partner_len]; p[i] = the partner
 * of column i or -1), Wmax = the widest row.  The pairs of a row are {(i, p[i]) : p[i] > i}; npairs[a] = their number,
 * common[a, b] = the pairs rows a and b share, d(a, b) = npairs[a] + npairs[b] - 2 common[a, b].  A row is invalid (status 1,
 * npairs 0, no cell, nobody's neighbour, neighbours 0, keep 0, leader -1) when its place is not inside d_partner, a partner
 * lies outside [-1, width), p[p[i]] != i or p[i] == i.  Rows are compared within a group only: group g of the G groups has the
 * consecutive rows d_group_off[g] .. d_group_off[g + 1] - 1 (int32[G + 1], from 0 to S), d_row_group[q] = the group of row q,
 * max_group_rows = the rows of the largest.  Rows a != b of one group are neighbours iff d <= threshold (mode 0, a radius >= 0)
 * or d * 10000 <= threshold * (npairs[a] + npairs[b]) (mode 1, basis points 0..10000), in int64.  d_tiles int32[T * 2] = the
 * planned tiles (ta, tb) of 64 x 64 rows: the upper-triangle tiles over the global row index that hold a cell of one group
 * (SqDistances::plan_tiles, csrc/sq_distances.h).
 * Outputs: d_status, d_npairs, d_neighbours (1 + the neighbours of a), d_leader int32[S], d_keep uint8[S] (greedy in row
 * order within the group: row a is kept iff no kept row below it in its group is its neighbour; leader = the row itself
 * when kept, else its lowest kept neighbour, a global row index), and d_common int32[common_cells], which may be null with
 * common_cells 0: the cell (a, b) of group g of n_g rows sits at d_mat_off[g] + (a - first) * n_g + (b - first) (int64[G + 1]).
 * d_out[0] = 0; d_out[1] = a status: bit 0 an entry of d_tiles outside the tile range (skipped), bit 1 a group the filter
 * could not take (offsets not ascending within 0..S, or more rows than max_group_rows says; left alone).
 * d_scratch (sq_structure_distances_scratch(S, Wmax, T) bytes, 8-byte aligned; 0 for sizes the entry refuses) holds the rows
 * as 1 + bits(Wmax - 1) bit planes of 64 columns per word and the neighbour bit matrix uint64[S * ceil(S / 64)].  Three kernels,
 * one after the other: the planes, the planned tiles from LDS, the filter with one wave per group.
 * Asynchronous on hip_stream, allocates nothing; 0, or -1 (a null pointer other than d_common, d_common without cells or
 * cells without it, S < 1, S above 65535, Wmax < 1, Wmax above 32768, partner_len < 1, G < 1, max_group_rows outside 1..S,
 * T < 1 or above the upper triangle's tiles, a mode outside 0..1, a threshold < 0 or above 10000 basis points, scratch too
 * small: nothing enqueued, nothing written).
 * sq_structure_distances_phases: the same call with only the kernels of `phases` (bit 0: the planes with status and npairs,
 * bit 1: the pairs, bit 2: the filter; 1..7, else -1) on buffers that hold what the earlier phases left. */
SQ_API size_t sq_structure_distances_scratch(int32_t S, int32_t Wmax, int32_t T);
SQ_API int sq_structure_distances(const int32_t *d_partner, int64_t partner_len, const int64_t *d_row_start, const int32_t *d_row_width,
                                  const int32_t *d_row_group, int32_t S, int32_t Wmax, const int32_t *d_group_off, const int64_t *d_mat_off,
                                  int32_t G, int32_t max_group_rows, const int32_t *d_tiles, int32_t T, int32_t mode, int32_t threshold,
                                  void *d_scratch, size_t scratch_bytes, int32_t *d_status, int32_t *d_npairs, int32_t *d_common,
                                  int64_t common_cells, int32_t *d_neighbours, int32_t *d_leader, uint8_t *d_keep, uint64_t *d_out,
                                  void *hip_stream);
SQ_API int sq_structure_distances_phases(int32_t phases, const int32_t *d_partner, int64_t partner_len, const int64_t *d_row_start,
                                         const int32_t *d_row_width, const int32_t *d_row_group, int32_t S, int32_t Wmax,
                                         const int32_t *d_group_off, const int64_t *d_mat_off, int32_t G, int32_t max_group_rows,
                                         const int32_t *d_tiles, int32_t T, int32_t mode, int32_t threshold, void *d_scratch,
                                         size_t scratch_bytes, int32_t *d_status, int32_t *d_npairs, int32_t *d_common, int64_t common_cells,
                                         int32_t *d_neighbours, int32_t *d_leader, uint8_t *d_keep, uint64_t *d_out, void *hip_stream);

/* ---- structures between the columns of an alignment and the residues of its rows (Project, Lift) ---------------------------
 * d_rows = uint8[R * L], the rows' ASCII bytes (classes as in sq_covariation_scan: A C G U in either case, T as U, gaps
 * - . ~, anything else "other"; a residue is any non-gap).  For every row: d_length int32[R] = its residues, d_col_of
 * int32[R * Lmax] = the column of residue i (-1 beyond the row's length), d_pos_of int32[R * L] = the residue of column c
 * (-1 at a gap).  Lmax >= the residues of every row is the caller's to know; a row with more gets status 2 on every line,
 * the first Lmax entries of col_of, and no structure.
 * sq_project_rows: K structure lines over the L columns per row, partners int32 (-1 unpaired): line k of row r at
 * d_structs[r * row_stride + k * L ..], row_stride = 0 (the K lines are shared by all rows) or K * L.  Per (row, line):
 * d_partner int32[R * K * Lmax] = the line in the row's residue coordinates (-1 unpaired and beyond the length), d_cls
 * uint8[R * K * L] = at the opening column v of every pair (v, w), v < w, its class in that row (1..6 = AU UA GC CG GU UG as
 * (letter at v, letter at w), 7 = two residues that are no canonical pair, 8 = a gap in exactly one column, 9 = a gap in
 * both; 0 elsewhere), d_counts int32[R * K * 12] = [0] the pairs, [1..9] per class, [10] those of an admitted class that
 * min_loop alone drops, [11] the pairs kept, d_status int32[R * K].  A pair is kept iff its class is 1..6, or 7 unless
 * canonical_only, and at least min_loop residues of the row lie strictly between its ends.  A line with a partner outside
 * [-1, L), p[p[c]] != c or p[c] == c has status 1, partners -1, classes and counts 0.
 * sq_lift_rows: per row up to K structure lines over the row's residues: line k < d_nstruct[r] (int32[R], taken within
 * 0..K) at d_short[d_start[r] + k * d_stride[r] ..] (int32[short_len]; d_start int64[R], d_stride int32[R] >= the row's
 * length), of which the row's length first entries are read.  d_partner int32[R * K * L] = the line over the columns (-1
 * at gaps, unpaired, and on the lines beyond d_nstruct[r], whose status is 0), d_status int32[R * K]: 1 for a line that is
 * invalid against the row's length, 2 for a row whose lines do not lie inside d_short or are narrower than its length.
 * One kernel each, a block per row at a time with the row's gap map in LDS as 64-column ballot words (csrc/sq_project.h);
 * every output cell is written by the kernel.  Asynchronous on hip_stream, allocate nothing, need no scratch; 0, or -1 (a
 * null pointer, R outside 1..2^20, L or Lmax outside 1..32768, K < 1, a row_stride other than 0 and K * L, canonical_only
 * outside 0..1, a negative min_loop, short_len < 1: nothing enqueued, nothing written). */
SQ_API int sq_project_rows(const uint8_t *d_rows, int32_t R, int32_t L, const int32_t *d_structs, int64_t row_stride, int32_t K,
                           int32_t Lmax, int32_t canonical_only, int32_t min_loop, int32_t *d_length, int32_t *d_col_of,
                           int32_t *d_pos_of, int32_t *d_partner, uint8_t *d_cls, int32_t *d_counts, int32_t *d_status,
                           void *hip_stream);
SQ_API int sq_lift_rows(const uint8_t *d_rows, int32_t R, int32_t L, const int32_t *d_short, int64_t short_len, const int64_t *d_start,
                        const int32_t *d_stride, const int32_t *d_nstruct, int32_t K, int32_t Lmax, int32_t *d_length,
                        int32_t *d_col_of, int32_t *d_pos_of, int32_t *d_partner, int32_t *d_status, void *hip_stream);

/* ---- measurement ------------------------------------------------------------
 * Kernel ids: 0 fill, 1 state, 2 stem_scan, 3 stem_score (+ select), 4 Edmonds, 5 Hungarian,
 * 6 Nussinov, 9 the bpp terms formed at sq_batch_create from bpp_matrix_dev (both kernels; recorded whether profiling
 * is enabled or not; alg_bytes = 8 N^2 (2 + bpp jobs) per sequence).  When enabled, every launch is bracketed by
 * hipEvents on the stream it runs on (the matching kernels run on the batch's side streams). */
SQ_API int sq_profile_enable(sq_batch *b, int32_t on);
SQ_API int sq_profile_get(sq_batch *b, int32_t kernel, double *total_ms, int64_t *launches, double *alg_bytes);
SQ_API int sq_profile_reset(sq_batch *b);
/* Work counters of the blossom kernel (kernel 4) since the last reset, always on: out[0] graphs matched, out[1] their
 * scan passes (one pass = one chunk of <= 64 neighbours of a popped S-vertex), and for the graph with the most
 * passes -- the kernel's critical path, one wave per graph -- out[2] its passes, out[3] its lane-0 events, out[4] its
 * vertices, out[5] its edges. */
SQ_API int sq_profile_counters(sq_batch *b, int32_t kernel, int64_t out[6]);

/* ---- scores and metrics of GIVEN structures (SQRNdbnseq.py:958-970, 861-899, 498-517, 1249-1258) -----------------------
 * sq_score_structs_dev -- for every partner row: ReferenceScores of the structure under its record (ScoreStruct of
 * PairsToStems(sorted pairs) in gap-free coordinates, with the host libm's powers), its stems, and TP FP FN FS PR RC against the
 * record's known structure; for every record the three scores of its known structure.  No sq_batch.  All pointers are the
 * caller's DEVICE memory; everything is enqueued on hip_stream, nothing is allocated or waited for.
 * Records (sq_score_desc), arrays over the gap-free positions of all records, record r from d_pos_off[r] on: d_codes (letter
 * codes as for sq_batch_desc, after upper() and T -> U), d_reacts (NULL when max_react_len is 0), d_gfcol (the input column of
 * every position), d_known (the known structure's partner in gap-free coordinates, -1 unpaired).  Per record: d_has_reacts
 * (0: every reactivity is 0.5, d_reacts is not read), d_nsep (its separators), d_known_n (pairs of the known structure, -1: none).
 * d_colmap, record r from d_col_off[r] on: the gap-free position of every input column, -1 for a gap column.  d_col_off /
 * d_colmap / d_gfcol are NULL when no record has a gap column.  d_pow[k] = pow(k / 2, 1.7) of the host's libm, k < pow_len
 * (4 x the longest record + 1 covers every stem).  max_react_len: the longest gap-free length of a record with reactivities
 * (<= 32768; sizes the kernel's LDS bitmap).
 * Rows (sq_score_rows): row q is record d_row_rec[q]'s and starts at d_partner[d_row_start[q]]: one int32 per INPUT column
 * of the record, the partner's column or -1.  Outputs per row: d_status (0; 1 invalid: a partner outside the record, p[p[i]]
 * != i, p[i] == i, a pair on a separator, or a record without a position to score; 2: beyond the exact range of the
 * rounding -- the caller recomputes that row), d_npairs and d_nstems (after the pairs that touch a gap column are dropped),
 * d_scores [nrows][3], d_metrics [nrows][6] (NaN without a known structure; both NaN for an invalid row), d_stems [stem_cap][3]
 * = (i, j, len) in input columns, row q's from d_stem_off[q] on.  Per record: d_ref_scores [nrec][3] (NaN without a known
 * structure), d_ref_status [nrec].
 * pass 0 writes d_status, d_npairs, d_nstems (and d_ref_status); the caller forms d_stem_off int64[nrows + 1], the exclusive
 * scan of d_nstems, and sizes d_stems; pass 1 writes the rest.  d_scratch: sq_score_scratch(nrec) bytes, the same for both
 * passes.  Returns 0, or -1 (bad argument, scratch too small: nothing enqueued). */
typedef struct sq_score_desc {
    int32_t nrec, max_react_len;
    const int64_t *d_pos_off;       /* [nrec + 1] */
    const uint8_t *d_codes;
    const double *d_reacts;
    const uint8_t *d_has_reacts;    /* [nrec] */
    const int32_t *d_nsep;          /* [nrec] */
    const int64_t *d_col_off;       /* [nrec + 1] or NULL */
    const int32_t *d_colmap, *d_gfcol;
    const int32_t *d_known, *d_known_n;
    const double *d_pow;
    int32_t pow_len;
} sq_score_desc;
typedef struct sq_score_rows {
    int64_t nrows;
    const int32_t *d_partner;
    const int64_t *d_row_start;     /* [nrows] */
    const int32_t *d_row_rec;       /* [nrows] */
    int32_t *d_status, *d_npairs, *d_nstems;
    const int64_t *d_stem_off;      /* [nrows + 1], pass 1 */
    int32_t *d_stems;
    int64_t stem_cap;
    double *d_scores, *d_metrics;
    double *d_ref_scores;
    int32_t *d_ref_status;
} sq_score_rows;
SQ_API size_t sq_score_scratch(int32_t nrec);
SQ_API int sq_score_structs_dev(const sq_score_desc *d, const sq_score_rows *o, int32_t pass, void *d_scratch, size_t scratch_bytes,
                                void *hip_stream);

/* ---- loop and pseudoknot annotation of GIVEN structures (SQRNdbnseq.py:104-150 for the levels) ------------------------------
 * sq_elements_rows -- for every partner row: the pseudoknot level of every pair (PairsToDBN's rule: pairs ordered by (crossing
 * count, start), first-fitted into groups, the groups ranked by size, the largest is level 1), what every column is, and the
 * loops that the pairs of level 1 close, with their sizes.  No sq_batch.  All pointers are the caller's DEVICE memory;
 * everything is enqueued on hip_stream, nothing is allocated or waited for.
 * Records (sq_elements_desc): d_pos_off, d_codes, d_col_off, d_colmap, d_gfcol as in sq_score_desc (the maps are NULL when no
 * record has a gap column); max_len: the longest gap-free length of a record (<= 32768; sizes the LDS of the levels).
 * Rows (sq_elements_rowset): row q is record d_row_rec[q]'s and starts at d_partner[d_row_start[q]], one int32 per INPUT column
 * as for sq_score_rows; its per-column outputs start at d_cell_off[q] (int64[nrows + 1], the exclusive scan of the rows'
 * widths; cells = its last entry): d_element int8 (0 exterior, 1 stem, 2 hairpin, 3 bulge, 4 internal, 5 multiloop, 6 a pair
 * of level >= 2, 7 a separator, 8 a gap column; an unpaired column carries its loop's type), d_level int16 (+L opens, -L
 * closes a pair of level L, else 0), d_loop_of int32 (the column's loop in the row's list; -1 for columns of kinds 1, 7, 8).
 * Per row: d_status (0; 1 invalid: a partner outside the record, p[p[i]] != i, p[i] == i or a pair on a separator -- its
 * columns hold -1, 0, -1 and it has no loop; 2: more stems than the LDS holds or more than 64 levels -- the caller annotates
 * that row), d_npairs (after the pairs that touch a gap column are dropped), d_nlevels, d_nloops (0 unless the status is 0).
 * d_loops [loop_cap][6] = (type, i, j, branches, unpaired, side5), i and j in input columns, row q's from d_loop_off[q] on:
 * the exterior loop (-1, the row's width) first, then the loops by i ascending; stacks are not listed.
 * pass 0 writes d_level, the kinds 1, 6, 7, 8 of d_element, d_status, d_npairs, d_nlevels, d_nloops; the caller forms d_loop_off
 * int64[nrows + 1], the exclusive scan of d_nloops, and sizes d_loops; pass 1 writes the rest.  d_scratch:
 * sq_elements_scratch(cells) bytes, the same memory for both passes (pass 0 leaves the loops' openers there).
 * Returns 0, or -1 (bad argument, scratch too small: nothing enqueued). */
typedef struct sq_elements_desc {
    int32_t nrec, max_len;
    const int64_t *d_pos_off;       /* [nrec + 1] */
    const uint8_t *d_codes;
    const int64_t *d_col_off;       /* [nrec + 1] or NULL */
    const int32_t *d_colmap, *d_gfcol;
} sq_elements_desc;
typedef struct sq_elements_rowset {
    int64_t nrows, cells;
    const int32_t *d_partner;
    const int64_t *d_row_start;     /* [nrows] */
    const int32_t *d_row_rec;       /* [nrows] */
    const int64_t *d_cell_off;      /* [nrows + 1] */
    int8_t *d_element;              /* [cells] */
    int16_t *d_level;               /* [cells] */
    int32_t *d_loop_of;             /* [cells] */
    int32_t *d_status, *d_npairs, *d_nlevels, *d_nloops;
    const int64_t *d_loop_off;      /* [nrows + 1], pass 1 */
    int32_t *d_loops;
    int64_t loop_cap;
} sq_elements_rowset;
SQ_API size_t sq_elements_scratch(int64_t cells);
SQ_API int sq_elements_rows(const sq_elements_desc *d, const sq_elements_rowset *o, int32_t pass, void *d_scratch, size_t scratch_bytes,
                            void *hip_stream);

/* ---- entropy mode as data (SQRNdbnseq.py:520-545, 1087-1089) ---------------------------------------------------------------
 * sq_entropy_rows -- for each listed job: AnnotateStems with no selected stem; its stems (len >= minlen, bpscore >= minbpscore)
 * form the symmetric N x N stem matrix, every cell (v, w) of a stem and its mirror holding the stem's total score; row i with
 * S = sum_j m[i][j] != 0 has H_i = -sum_{j: m != 0} p log2 p, p = m[i][j] / S, in bits, else H_i = 0.  fp64 throughout.
 * All d_ pointers are the caller's DEVICE memory: d_pos_off int64[njob + 1] -- list entry k's N values H_i are written to
 * d_position[d_pos_off[k] ..] (d_pos_off[k + 1] - d_pos_off[k] must be N: rows beyond it are not written); d_mean[k] = sum_i
 * H_i / N (NaN for N = 0); d_nstems[k] = the stems that formed the matrix.  d_scratch: sq_entropy_scratch(njob, cells) bytes,
 * cells = the sum of N^2 over the list (one dense tile per entry); its content is undefined afterwards.
 * Deterministic: a cell is stored by exactly one stem and every sum has one fixed order, so a job gives the same bits whatever
 * else the call or the batch holds.  Sequences of more than 32,768 nt are refused (-1).
 * Runs on the batch's stream like sq_align_accumulate; the outputs are complete when the call returns.  Returns 0, -1 (bad
 * argument, scratch too small), -3 (a capacity of the batch: sq_last_capacity). */
SQ_API size_t sq_entropy_scratch(int32_t njob, int64_t cells);
SQ_API int sq_entropy_rows(sq_batch *b, int32_t njob, const int32_t *job_ids, const int64_t *d_pos_off, double *d_position,
                           double *d_mean, int32_t *d_nstems, void *d_scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SQUARNA_HIP_H */
