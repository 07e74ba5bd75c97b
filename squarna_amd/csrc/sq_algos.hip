// sq_algos.hip -- host driver of RunAlgo (SQRNdbnseq.py:548-595) for the E / H / N algorithms:
// one AnnotateStems pass on the GPU (scan + exact rescoring), the matching / DP on the GPU
// (sq_match.hip), then the reference's stem filters on the host.
#include <algorithm>
#include <functional>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>
#include "sq_host.h"
#include "sq_match.h"
#include "sq_blossom.h"
#include "sq_algo_plan.h"
#include "sq_algos_dev.h"
#include "sq_cells.h"

#define HIPCK(x) do { int _r = sq_check((x), #x); if (_r) return _r; } while (0)

typedef std::pair<int, int> BP;

#include <chrono>
static inline double sq_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// exact scoremat cell on the host: the same fp64 expression as sq_cell_score (sq_kernels.hip)
static double cell_score_host(const sq_batch *b, const SqJob &J, int i, int j, const double *dense = nullptr)
{
    if (dense) return dense[(size_t)sq_m64_index(J, i, j)];   // jobs with a bpp term / multiplier: the device's exact matrix
    const uint8_t *codes = b->codes.data() + J.pos_off;
    const sq_paramset &ps = b->psets[J.pset];
    const double w = ps.bpweight[codes[i] * 32 + codes[j]];
    double rf = 1.0;
    if (!J.default_reacts) {
        if (J.rf_idx >= 0) {                               // the host-libm table the device reads (sq_reactfactor)
            const uint8_t *lv = b->ridx.data() + J.pos_off;
            rf = b->rftab[(size_t)J.rf_idx * 256 + lv[i] * 16 + lv[j]];
        } else {
            const double *r = sq_host_reacts(b) + J.pos_off;
            rf = sqrt((1.0 - (r[i] + r[j]) / 2.0) * 2.0);
        }
    }
    if (w <= 0) rf = 1.0 / (rf > 0.01 ? rf : 0.01);
    return w * rf;
}

// PairsToStems (SQRNdbnseq.py:498-517) on sorted pairs
static void pairs_to_stems(const std::vector<BP> &sp, std::vector<HStem> &out)
{
    out.clear();
    for (size_t k = 0; k < sp.size(); k++) {
        if (k && sp[k - 1].first + 1 == sp[k].first && sp[k - 1].second == sp[k].second + 1) out.back().len++;
        else out.push_back(HStem{sp[k].first, sp[k].second, 1, 0, 0});
    }
}

// the two filter passes of RunAlgo (:570-595)
// The pairs of a matching form stems (maximal stacks).  All base pairs of a stem cross the same pairs, so PairsToDBN's
// level rule (:104-150: crossing counts, order by (count, start), first fit, groups ranked by size) gives every stem
// one level and can be evaluated per STEM with the stem lengths as weights (sq_stem_levels; DESIGN.md section 5 has the
// argument) -- a dozen stems instead of a hundred pairs, and the rule is quadratic.  Dropping whole stems (score filter,
// level limit) never changes how the remaining pairs stack, so the stems stay the stems.
static void filter_stemset(const sq_batch *b, const SqJob &J, std::vector<BP> pairs, int levellimit,
                           std::vector<HStem> &stemset, const double *dense = nullptr)
{
    const sq_paramset &ps = b->psets[J.pset];
    for (BP &p : pairs) if (p.first > p.second) std::swap(p.first, p.second);
    std::sort(pairs.begin(), pairs.end());
    static thread_local std::vector<HStem> stems, kept, lim;
    static thread_local std::vector<int> lv;
    pairs_to_stems(pairs, stems);
    auto score_of = [&](const HStem &st) {
        double s = 0;                                                    // sum(...) from int 0, left to right
        for (int k = 0; k < st.len; k++) s = s + cell_score_host(b, J, st.i + k, st.j - k, dense);
        return s;
    };
    kept.clear();
    for (HStem &st : stems) {
        st.bps = score_of(st);
        if (st.bps >= ps.minbpscore && (double)st.len >= ps.minlen) kept.push_back(st);
    }
    // DBNToPairs(PairsToDBN(pairs, N, levellimit)) : drop pseudoknot levels above the limit (:581)
    sq_stem_levels(kept, lv);
    lim.clear();
    for (size_t k = 0; k < kept.size(); k++)
        if ((levellimit < 0 || lv[k] <= levellimit) && lv[k] <= 49) lim.push_back(kept[k]);   // 49 bracket types exist
    sq_stem_levels(lim, lv);                                             // :582 levels of what is left
    stemset.clear();
    for (size_t k = 0; k < lim.size(); k++) {
        const HStem &st = lim[k];
        if (lv[k] > 1 && st.len < 4) continue;                           // :589 short pseudoknotted stems
        const double sc = st.bps;                                        // (the same sum as in the first pass)
        if (sc >= ps.minbpscore && (double)st.len >= ps.minlen) stemset.push_back(HStem{st.i, st.j, st.len, sc, sc});
    }
}

// ---- one chunk of matching work: planned (sq_algo_plan.h), staged (kernel launch, asynchronous) and collected later ------
struct SqAlgoChunk : SqAlgoPlan {
    int algo = 0;
    size_t k0 = 0, k1 = 0;                       // jobs[k0, k1) of the caller's list
    std::vector<std::vector<int>> vid2pos;       // Edmonds: graph vertex -> position
    std::vector<uint64_t> seen_hash;             // (SQ_MWM_POSTHOC) hash of every job's result as the collector read it
    // pointers into the pinned staging buffer (SqAlgoStage), set by chunk_stage
    SqMatchJob *p_mj = nullptr; SqAlgoJob *p_aj = nullptr; SqAlgoStat *h_stats = nullptr;   // device-side RunAlgo: the job table
                                                 // in list order, the per-job records, the finish kernel's statistics
    SqMatchJob *p_jobs = nullptr;                // the sorted job table and the edge list (read by the kernels in place)
    SqMatchEdge *p_edges = nullptr;
    int32_t *d_out = nullptr, *d_cnt = nullptr;  // results, written by the kernels in place
    uint32_t *flag = nullptr; uint32_t flag_val = 0;   // completion word published by sq_flag_kernel
    int32_t *bin_head = nullptr;                 // Edmonds only: first job (row of the sorted table) of every block
    uint32_t *job_flags = nullptr;               // Edmonds only: per job "mates are in host memory" (== flag_val),
                                                 // indexed by the job's position in the SORTED table (sorted_pos)
    hipStream_t st = nullptr;
    // Streams of the size classes (SqAlgoPlan::classes): class 0 of Edmonds (the largest graphs, the critical path) runs on
    // the Edmonds side stream, its other classes go -- largest first -- in front of the Hungarian / Nussinov kernels on THEIR
    // stream: no extra streams (see side_of), and the whole sequence still ends before class 0 does.
};

namespace {
// pow(x, 1.7) through the host libm (SQRNalgos.py:101,122), memoised: the stem scores of one sequence take few
// distinct values (sums of a handful of pair weights), and pow dominates the edge build otherwise
struct PowCache {
    uint64_t key[64]; double val[64]; bool used[64];
    PowCache() { for (bool &u : used) u = false; }
    double operator()(double x)
    {
        uint64_t k; memcpy(&k, &x, 8);
        unsigned h = (unsigned)((k * 0x9E3779B97F4A7C15ull) >> 58);
        for (int t = 0; t < 8; t++, h = (h + 1) & 63) {
            if (used[h] && key[h] == k) return val[h];
            if (!used[h]) { used[h] = true; key[h] = k; return val[h] = pow(x, 1.7); }
        }
        return pow(x, 1.7);
    }
};
}

// Side stream of staging slot `slot` (0 Edmonds, 1 Hungarian, 2 Nussinov).  The two short kernels share a stream: the
// runtime multiplexes all streams of the process onto a few hardware queues (GPU_MAX_HW_QUEUES), streams that share a
// queue serialise, and with several batches in flight every stream less keeps a 6 ms blossom kernel out of some other
// batch's round queue.  Hungarian + Nussinov back to back (1.4 + 1.5 ms) still end long before Edmonds does.
// One batch folded alone keeps Nussinov on a stream of its own (it then ends before the greedy loop does, and the
// collection of the short kernels does not wait behind Edmonds' second size class + Hungarian); sq_fold_concurrent
// with three or more batches in flight asks for the two-stream form.
// (slot 3: the stream of the blossom kernel's smaller size classes -- a stream of its own when the batch is folded alone,
// else in front of the short kernels on theirs.  Until the critical class took 2.2 ms they could sit in front of the
// Hungarian kernel: 1.0 + 1.5 ms then ended after the critical class did)
static inline int side_of(const sq_batch *b, int slot)
{
    const int forced = sq_tuning().side_streams;
    const int nside = forced ? forced : b->side_streams;
    if (slot == 3) return nside >= 3 ? 3 : (nside == 2 ? 1 : 0);
    return nside >= 3 ? slot : (nside == 2 ? (slot == 0 ? 0 : 1) : 0);
}

// pinned staging buffer `slot` of the batch, at least `bytes` large (grow-only)
static char *stage_buffer(sq_batch *b, int slot, size_t bytes)
{
    if (b->stage_cap[slot] < bytes) {
        if (b->stage_buf[slot]) { hipStreamSynchronize(slot < 3 && b->side[side_of(b, slot)] ? b->side[side_of(b, slot)] : b->stream); sq_pinned_put(b->stage_buf[slot]); }
        b->stage_buf[slot] = nullptr; b->stage_cap[slot] = 0;
        const size_t cap = bytes + bytes / 2 + 4096;
        if (sq_pinned_get((void **)&b->stage_buf[slot], cap)) return nullptr;
        memset(b->stage_buf[slot], 0, cap);               // (a cached buffer may hold completion flags of an earlier batch)
        b->stage_cap[slot] = cap;
    }
    return b->stage_buf[slot];
}

// step 1 of algo_build: the sizes of jobs[k0..) -- cells (= edges) and, for Edmonds, graph vertices (distinct positions) --
// from the stems (worker pool) or, when the stems stayed on the device, from sq_algo_sizes_kernel's records
static void chunk_sizes(sq_batch *b, const std::vector<int> &jobs, const std::vector<std::vector<HStem>> &stems, size_t k0,
                        int algo, const SqAlgoSize *dev_sizes, std::vector<SqAlgoJobSize> &jb)
{
    auto size_one = [&](int q) {
        const SqJob &J = b->jobs[jobs[k0 + q]];
        size_t ncell = 0;
        if (dev_sizes) ncell = (size_t)dev_sizes[k0 + q].nedges;
        else for (const HStem &s : stems[k0 + q]) ncell += (size_t)s.len;
        int n = J.n;
        if (algo == SQ_ALGO_E) {
            n = 0;
            if (dev_sizes) n = dev_sizes[k0 + q].nv;
            else {
                static thread_local std::vector<char> seen;
                seen.assign((size_t)J.n, 0);
                for (const HStem &s : stems[k0 + q])
                    for (int t = 0; t < s.len; t++) {
                        if (!seen[s.i + t]) { seen[s.i + t] = 1; n++; }
                        if (!seen[s.j - t]) { seen[s.j - t] = 1; n++; }
                    }
            }
        }
        jb[q] = sq_algo_job_size(algo, n, ncell);
    };
    // (with the sizes from the device a job costs a few instructions: waking the pool costs more than the loop)
    if (dev_sizes) for (int q = 0; q < (int)jb.size(); q++) size_one(q);
    else sq_pool(b)->parallel_for((int)jb.size(), size_one);
}

// step 3 of algo_build: the pinned staging buffer `slot` of the planned chunk, its pointers, the sorted job table
static int chunk_stage(sq_batch *b, int slot, SqAlgoChunk &ck, bool dev)
{
    const SqAlgoStage &s = ck.stage;
    const size_t nq = ck.mj.size();
    char *pin = stage_buffer(b, slot, s.bytes);
    if (!pin) return 2;
    if (dev) {
        ck.p_mj = (SqMatchJob *)(pin + s.p_mj); ck.p_aj = (SqAlgoJob *)(pin + s.p_aj); ck.h_stats = (SqAlgoStat *)(pin + s.h_stats);
        memcpy(ck.p_mj, ck.mj.data(), nq * sizeof(SqMatchJob));
        memset(ck.h_stats, 0, sizeof(SqAlgoStat));
    }
    ck.p_jobs = (SqMatchJob *)(pin + s.jobs); ck.p_edges = (SqMatchEdge *)(pin + s.edges);
    ck.d_out = (int32_t *)(pin + s.out); ck.d_cnt = (int32_t *)(pin + s.cnt);
    ck.flag = (uint32_t *)(pin + s.flag);
    ck.flag_val = ++b->algo_seq;
    *ck.flag = 0;
    if (s.job_flags != SQ_PLAN_NONE) {
        ck.job_flags = (uint32_t *)(pin + s.job_flags); memset(ck.job_flags, 0, nq * 4);
        ck.bin_head = (int32_t *)(pin + s.bin_head);
    }
    memcpy(ck.p_jobs, ck.sorted.data(), nq * sizeof(SqMatchJob));
    return 0;
}

// step 4 of algo_build (host-driven form): the edges, written by the worker pool straight into the pinned buffer
static void chunk_edges(sq_batch *b, const std::vector<int> &jobs, const std::vector<std::vector<HStem>> &stems, SqAlgoChunk &ck)
{
    const std::vector<SqMatchJob> &mj = ck.mj;
    const int algo = ck.algo;
    const size_t k0 = ck.k0;
    ck.vid2pos.resize(mj.size());
    if (b->sw.mwm_posthoc) ck.seen_hash.assign(mj.size(), 0);
    sq_pool(b)->parallel_for((int)mj.size(), [&](int q) {
        CpuScope cpu_(2);
        const SqJob &J = b->jobs[jobs[k0 + q]];
        const std::vector<HStem> &st_ = stems[k0 + q];
        SqMatchEdge *e = ck.p_edges + mj[q].edge_off;
        PowCache pow17;
        if (algo == SQ_ALGO_E) {
            static thread_local std::vector<int> pos2id;
            pos2id.assign((size_t)J.n, -1);
            std::vector<int> &ids = ck.vid2pos[q];
            ids.reserve((size_t)mj[q].n);
            for (const HStem &s : st_) {
                const double wt = pow17(s.bps);                      // SQRNalgos.py:101
                for (int t = 0; t < s.len; t++) {
                    const int v = s.i + t, w = s.j - t;
                    if (pos2id[v] < 0) { pos2id[v] = (int)ids.size(); ids.push_back(v); }   // node order = first appearance
                    if (pos2id[w] < 0) { pos2id[w] = (int)ids.size(); ids.push_back(w); }
                    *e++ = SqMatchEdge{pos2id[v], pos2id[w], wt};
                }
            }
        } else {
            for (const HStem &s : st_) {
                const double wt = algo == SQ_ALGO_H ? pow17(s.bps) : s.bps;      // SQRNalgos.py:122 / :49
                for (int t = 0; t < s.len; t++) *e++ = SqMatchEdge{s.i + t, s.j - t, wt};
            }
        }
    });
}

// Host part of a chunk: jobs[k0..) of `algo`, as many as fit into region_bytes (ck.k1, ck.carve.bytes) -- their sizes, the
// plan (sq_algo_plan.h), pinned staging buffer `slot` and, in the host-driven form, the edge lists.  dev_sizes: the device
// form (the stems stayed on the device, sq_algo_edges_kernel writes the edges).
static int algo_build(sq_batch *b, const std::vector<int> &jobs, const std::vector<std::vector<HStem>> &stems, size_t k0,
                      int algo, size_t region_bytes, int slot, SqAlgoChunk &ck, const SqAlgoSize *dev_sizes = nullptr)
{
    ck = SqAlgoChunk();
    ck.algo = algo; ck.k0 = k0;
    const double tb0 = sq_now();
    std::vector<SqAlgoJobSize> jb(jobs.size() - k0);
    chunk_sizes(b, jobs, stems, k0, algo, dev_sizes, jb);
    const double tb1 = sq_now();
    sq_algo_plan_chunk(algo, jb.data(), jb.size(), region_bytes, dev_sizes != nullptr, b->inflight, sq_algo_knobs(b->sw.lsap_classes), ck);
    const size_t nq = ck.mj.size();
    ck.k1 = k0 + nq;
    if (!nq) return 0;
    for (size_t q = 0; q < nq; q++) ck.mj[q].pos_off = ck.sorted[ck.sorted_pos[q]].pos_off = b->jobs[jobs[k0 + q]].pos_off;
    const int rs = chunk_stage(b, slot, ck, dev_sizes != nullptr);
    if (rs) return rs;
    if (b->sw.mwm_dump && algo == SQ_ALGO_E) {
        fprintf(stderr, "[mwm] %zu graphs, classes:", nq);
        for (auto &c : ck.classes) fprintf(stderr, " [%d +%d: %zu B]", c.start, c.count, ck.need[ck.sorted[c.start].pad]);
        fprintf(stderr, "\n[mwm] (n m bytes):");
        for (size_t r = 0; r < nq; r++) fprintf(stderr, " %d %d %zu;", ck.sorted[r].n, ck.sorted[r].nedges, ck.need[ck.sorted[r].pad]);
        fprintf(stderr, "\n");
    }
    const double tb2 = sq_now();
    if (dev_sizes) {                                      // (the edges are written on the device: sq_algo_edges_kernel)
        if (b->sw.timing) fprintf(stderr, "[sq_algos] layout algo %d: sizes %.3f ms, tables + classes %.3f ms\n", algo, (tb1 - tb0) * 1e3, (tb2 - tb1) * 1e3);
        return 0;
    }
    chunk_edges(b, jobs, stems, ck);
    if (b->sw.timing) fprintf(stderr, "[sq_algos] build algo %d: sizes %.3f ms, layout+pinned alloc %.3f ms, edges %.3f ms\n", algo,
                                     (tb1 - tb0) * 1e3, (tb2 - tb1) * 1e3, (sq_now() - tb2) * 1e3);
    return 0;
}

// The launches of a planned chunk, one per size class of its sorted table.  edges / out / cnt / job_flags: what the kernels
// read and write (the pinned staging buffer, or the region in the device form); scratch and the device copy of the edges lie
// in the region.  `other` (Edmonds in a fold): the stream of the short kernels takes the classes after the first; st then
// waits for it, so "st is idle" still means "the chunk is done".  Without it the classes follow each other on st.
static int launch_classes(sq_batch *b, SqAlgoChunk &ck, char *region, const SqMatchEdge *edges, int32_t *out, int32_t *cnt,
                          uint32_t *job_flags, hipStream_t st, hipStream_t other)
{
    const SqAlgoKnobs kn = sq_algo_knobs(b->sw.lsap_classes);
    for (size_t cidx = 0; cidx < ck.classes.size(); cidx++) {
        const SqAlgoClass &c = ck.classes[cidx];
        const int rl = sq_launch_matching(ck.algo, ck.sorted.data() + c.start, c.count, ck.p_jobs + c.start, edges, ck.nedges,
                                          (SqMatchEdge *)(region + ck.carve.o_edges), region + ck.carve.o_scr, out, cnt, b->ctx.codes,
                                          job_flags ? job_flags + c.start : nullptr, ck.flag_val, (cidx > 0 && other) ? other : st,
                                          ck.p_jobs + c.start, ck.bin_head ? ck.bin_head + c.start : nullptr, b->inflight, kn, b->sw.mwm_dump);
        if (rl) return sq_check((hipError_t)rl, "matching kernel launch");
    }
    if (other && ck.classes.size() > 1) {
        if (!b->class_ev) HIPCK(sq_event_get(b->device, &b->class_ev));
        HIPCK(hipEventRecord(b->class_ev, other));
        HIPCK(hipStreamWaitEvent(st, b->class_ev, 0));
    }
    return 0;
}

// Device part: kernel of a built chunk into [region, region + ck.carve.bytes) on stream st.  The job table and the edges
// are read by the kernels straight from the pinned staging buffer (each kernel reads them once, at its start), the results
// go there too.  Nothing is waited for.
static int algo_launch(sq_batch *b, SqAlgoChunk &ck, char *region, hipStream_t st, hipStream_t st2 = nullptr)
{
    ck.st = st;
    if (ck.mj.empty()) return 0;
    hipEvent_t pe0;
    const int pslot = ck.algo == SQ_ALGO_E ? 4 : ck.algo == SQ_ALGO_H ? 5 : 6;
    sq_prof_begin(b, pslot, st, &pe0);
    const int rl = launch_classes(b, ck, region, ck.p_edges, ck.d_out, ck.d_cnt, ck.job_flags, st, ck.algo == SQ_ALGO_E ? st2 : nullptr);
    if (rl) return rl;
    sq_prof_end(b, pslot, st, pe0);
    hipLaunchKernelGGL(sq_flag_kernel, dim3(1), dim3(1), 0, st, ck.flag, ck.flag_val);   // "results are in host memory"
    HIPCK(hipGetLastError());
    return 0;
}

// jobs whose score matrix carries a bpp term / multiplier: RunAlgo's stem filters re-sum cells of THAT matrix, read back here
static int chunk_dense(sq_batch *b, const std::vector<int> &jobs, const SqAlgoChunk &ck, std::vector<std::vector<double>> &dense)
{
    dense.assign(ck.mj.size(), {});
    for (size_t q = 0; q < ck.mj.size(); q++) {
        const SqJob &J = b->jobs[jobs[ck.k0 + q]];
        if (J.mat64_off < 0 && !J.mulsh) continue;
        dense[q].resize((size_t)J.n * J.n);
        if (J.mulsh) {
            // an alignment's row (weights read through the gap map from the shared matrix, no slice of its own): its slice for
            // the host's filters, gathered into a buffer of this call
            double *tmp = nullptr; int32_t *d_j = nullptr;
            const int32_t jid = jobs[ck.k0 + q];
            HIPCK(hipMalloc((void **)&tmp, dense[q].size() * 8 + 256));
            d_j = (int32_t *)((char *)tmp + dense[q].size() * 8);
            HIPCK(hipMemcpy(d_j, &jid, 4, hipMemcpyHostToDevice));
            sq_launch_gather_mul(b->ctx, d_j, 1, J.n, b->stream, tmp);
            const hipError_t ge = hipStreamSynchronize(b->stream);
            if (ge == hipSuccess) hipMemcpy(dense[q].data(), tmp, dense[q].size() * 8, hipMemcpyDeviceToHost);
            hipFree(tmp);
            HIPCK(ge);
            continue;
        }
        HIPCK(hipMemcpy(dense[q].data(), b->ctx.mat64 + J.mat64_off, dense[q].size() * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

static uint64_t mates_hash(const int32_t *mate, int n)     // (SQ_MWM_POSTHOC) FNV-1a over a job's result
{
    uint64_t h = 1469598103934665603ull;
    for (int v = 0; v < 2 * n + 2; v++) { h ^= (uint32_t)mate[v]; h *= 1099511628211ull; }
    return h;
}

// the pairs of Edmonds job q from its mates; false: the kernel reported an exceeded capacity
static bool edmonds_pairs(sq_batch *b, SqAlgoChunk &ck, size_t q, const int32_t *mate, std::vector<BP> &pairs)
{
    const SqMatchJob &m = ck.mj[q];
    if (m.n > 0 && mate[0] == -2) return false;
    {   // measurement: the job with the most scan passes is the kernel's critical path
        const int64_t np = mate[2 * m.n], ne = mate[2 * m.n + 1];
        std::lock_guard<std::mutex> lk(b->mwm_mu);
        b->mwm_stats[0]++; b->mwm_stats[1] += np;
        if (np > b->mwm_stats[2]) { b->mwm_stats[2] = np; b->mwm_stats[3] = ne; b->mwm_stats[4] = m.n; b->mwm_stats[5] = m.nedges; }
    }
    if (b->sw.mwm_posthoc && ck.seen_hash.size() == ck.mj.size()) ck.seen_hash[q] = mates_hash(mate, m.n);   // debug: what this read saw
    if (sq_tuning().mwm_verify && m.n > 0) {
        // debug: the same algorithm object run on the host over the job's edges must give the kernel's mates
        std::vector<char> scr(SqBlossom::scratch_bytes(m.n, m.nedges) + 64);
        SqBlossom hb;
        hb.init(m.n, m.nedges, ck.p_edges + m.edge_off, scr.data());
        hb.run();
        int diff = 0;
        for (int v = 0; v < m.n; v++) diff += hb.mate[v] != mate[v];
        if (diff || hb.error) {
            const int sp = ck.sorted.empty() ? (int)q : ck.sorted_pos[q];
            int cls = 0;
            for (size_t ci = 0; ci < ck.classes.size(); ci++) if (sp >= ck.classes[ci].start) cls = (int)ci;
            fprintf(stderr, "[mwm verify] job %zu (row %d, class %d of %zu): n %d m %d: %d of the kernel's mates differ from the host run "
                    "(host error %d; kernel passes %d events %d, host passes %d events %d)\n", q, sp, cls, ck.classes.size(), m.n,
                    m.nedges, diff, hb.error, mate[2 * m.n], mate[2 * m.n + 1], hb.stat_pass, hb.stat_event);
        }
    }
    for (int v = 0; v < m.n; v++)
        if (mate[v] > v) pairs.push_back(BP(ck.vid2pos[q][v], ck.vid2pos[q][mate[v]]));
    return true;
}

// the pairs of a Hungarian job from its assignment `sol` (SQRNalgos.py:119-133)
static void hungarian_pairs(const sq_batch *b, const SqJob &J, const std::vector<HStem> &stems, const int32_t *sol, std::vector<BP> &pairs)
{
    const uint8_t *codes = b->codes.data() + J.pos_off;
    // cells with mat[v,w] != 0 (SQRNalgos.py:119-123) as a bit matrix (set, queried, cleared cell by cell: no sort,
    // no O(N^2) clearing); sequences too long for that keep a sorted list
    static thread_local std::vector<int64_t> cells;
    static thread_local std::vector<uint64_t> cellbits;
    const size_t nn = (size_t)J.n * J.n;
    const bool use_bits = nn <= ((size_t)1 << 24);
    if (use_bits && cellbits.size() < (nn + 63) / 64) cellbits.resize((nn + 63) / 64, 0);
    cells.clear();
    PowCache pow17;
    for (const HStem &s : stems) {
        if (-pow17(s.bps) == 0) continue;
        for (int t = 0; t < s.len; t++) cells.push_back((int64_t)(s.i + t) * J.n + (s.j - t));
    }
    if (use_bits) for (int64_t cidx : cells) cellbits[(size_t)cidx >> 6] |= 1ull << (cidx & 63);
    else std::sort(cells.begin(), cells.end());
    for (int kk = 0; kk < J.n; kk++) {                        // SQRNalgos.py:130-133
        const int sk = sol[kk];
        if (sk < 0 || !(kk < sk)) continue;
        bool far = kk < sk - 3;
        if (!far) for (int x = kk + 1; x < sk; x++) if (codes[x] == SQ_CODE_SEP1 || codes[x] == SQ_CODE_SEP2) { far = true; break; }
        if (!far) continue;
        if (sol[sk] != kk) continue;
        const int64_t cidx = (int64_t)kk * J.n + sk;
        if (use_bits ? !((cellbits[(size_t)cidx >> 6] >> (cidx & 63)) & 1ull) : !std::binary_search(cells.begin(), cells.end(), cidx)) continue;
        pairs.push_back(BP(kk, sk));
    }
    if (use_bits) for (int64_t cidx : cells) cellbits[(size_t)cidx >> 6] = 0;
}

// Edmonds job by job.  ONE poller (this thread) sweeps the per-job completion words and hands every group of newly finished
// jobs to the worker pool -- workers never spin: with several batches in flight, 32 spinning workers per batch would take
// every host core for the whole length of the blossom kernel.  Returns 0, 2 (a job was never published) or 3 (stream_err).
static int collect_streamed(sq_batch *b, SqAlgoChunk &ck, std::vector<int> pending, const std::function<void(size_t)> &finish_job,
                            const std::atomic<int> &bad, int &stream_err)
{
    std::vector<int> ready;
    uint64_t idle = 0;
    while (!pending.empty() && !bad) {
        ready.clear();
        size_t w = 0;
        for (int q : pending) {
            if (*(volatile uint32_t *)(ck.job_flags + ck.sorted_pos[q]) == ck.flag_val) ready.push_back(q);
            else pending[w++] = q;
        }
        pending.resize(w);
        if (!ready.empty()) {
            std::atomic_thread_fence(std::memory_order_acquire);
            idle = 0;
            if (ready.size() <= 2) for (int q : ready) finish_job((size_t)q);
            else sq_pool(b)->parallel_for((int)ready.size(), [&](int t) { finish_job((size_t)ready[t]); }, ready.size() >= 128 ? 1 : 0);
            continue;
        }
        if ((++idle & 0x3FFF) == 0) {
            // a faulted kernel / aborted queue never writes its flags: poll the stream now and then
            const hipError_t qe = hipStreamQuery(ck.st);
            if (qe != hipErrorNotReady && qe != hipSuccess) { stream_err = (int)qe; return 3; }
            if (qe == hipSuccess || *(volatile uint32_t *)ck.flag == ck.flag_val) {
                bool missing = false;                    // kernel over: every flag must be there now
                for (int q : pending) missing |= *(volatile uint32_t *)(ck.job_flags + ck.sorted_pos[q]) != ck.flag_val;
                if (missing) return 2;
            }
        }
        if (sq_relaxed_waits(b)) sq_wait_step(1 << 20, true);    // (sleeps ~10 us)
        else for (int t = 0; t < 32; t++) sq_wait_step(0, false);
    }
    return 0;
}

// Wait for a staged chunk, read its result and apply the reference's stem filters (:570-595).
// on_job (optional, Edmonds with per-job flags): jobs are collected one by one as the kernel finishes them, smallest
// graphs first, and on_job(k) is called (from a pool worker) as soon as out[k] is final.
static int algo_collect(sq_batch *b, const std::vector<int> &jobs, const std::vector<std::vector<HStem>> &stems,
                        SqAlgoChunk &ck, int levellimit_opt, std::vector<std::vector<HStem>> &out,
                        const std::function<void(size_t)> *on_job = nullptr)
{
    if (ck.mj.empty()) return 0;
    const std::vector<SqMatchJob> &mj = ck.mj;
    const int algo = ck.algo;
    const double tw0 = sq_now();
    const bool streaming = on_job && ck.job_flags;
    if (!streaming) {   // spin on the completion word in pinned memory (no driver round trip, no staged copy)
        const int wr = sq_wait_word(b, ck.flag, ck.flag_val, ck.st, "matching kernel");
        if (wr) return wr;
    }
    const int32_t *h_out_p = ck.d_out, *h_cnt_p = ck.d_cnt;
    const double tw1 = sq_now();
    struct Rep { int algo; double t0, t1; bool on; ~Rep() { if (on) fprintf(stderr, "[sq_algos] algo %d: wait %.3f ms, host filters %.3f ms\n", algo, (t1 - t0) * 1e3, (sq_now() - t1) * 1e3); } } rep{algo, tw0, tw1, b->sw.timing};
    std::vector<std::vector<double>> dense;
    { const int rd = chunk_dense(b, jobs, ck, dense); if (rd) return rd; }
    std::atomic<int> bad{0};
    int stream_err = 0;
    std::vector<int> order(mj.size());
    for (size_t q = 0; q < mj.size(); q++) order[q] = (int)q;
    if (streaming) std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return mj[x].nedges < mj[y].nedges; });
    // body of one job: read its result from pinned memory, RunAlgo's filters, optional hook
    const std::function<void(size_t)> finish_job = [&](size_t q) {
        CpuScope cpu_(1);
        const size_t k = ck.k0 + q;
        const SqJob &J = b->jobs[jobs[k]];
        const int levellimit = levellimit_opt >= 0 ? levellimit_opt : 3 - (J.n > 500 ? 1 : 0);   // :1043-1044
        std::vector<BP> pairs;
        if (algo == SQ_ALGO_E) {
            if (!edmonds_pairs(b, ck, q, h_out_p + mj[q].out_off, pairs)) { bad = 1; return; }
        } else if (algo == SQ_ALGO_N) {
            const int32_t *pp = h_out_p + 2 * mj[q].out_off;
            for (int t = 0; t < h_cnt_p[q]; t++) pairs.push_back(BP(pp[2 * t], pp[2 * t + 1]));
        } else hungarian_pairs(b, J, stems[k], h_out_p + mj[q].out_off, pairs);
        { CpuScope cpu_f(3); filter_stemset(b, J, pairs, levellimit, out[k], dense[q].empty() ? nullptr : dense[q].data()); }
        if (streaming) { CpuScope cpu_h(5); (*on_job)(k); }
    };
    if (!streaming) sq_pool(b)->parallel_for((int)mj.size(), [&](int qi) { finish_job((size_t)order[qi]); });
    else { const int rs = collect_streamed(b, ck, order, finish_job, bad, stream_err); if (rs) bad = rs; }
    if (b->sw.mwm_posthoc && algo == SQ_ALGO_E && ck.seen_hash.size() == mj.size()) {
        hipStreamSynchronize(ck.st);
        for (size_t q = 0; q < mj.size(); q++)
            if (mates_hash(h_out_p + mj[q].out_off, mj[q].n) != ck.seen_hash[q])
                fprintf(stderr, "[mwm posthoc] job %zu (n %d m %d): the result read when its flag appeared differs from the result after the kernel\n",
                        q, mj[q].n, mj[q].nedges);
    }
    if (bad == 3) return sq_check((hipError_t)stream_err, "matching kernel");
    if (bad == 2) { sq_set_error("matching kernel did not publish a job"); return 2; }
    if (bad) { sq_set_capacity_error(SQ_CAP_FIXED, "blossom capacity exceeded"); return -3; }
    if (!streaming && on_job) for (size_t q = 0; q < mj.size(); q++) (*on_job)(ck.k0 + q);
    return 0;
}

static int algo_annotate(sq_batch *b, const std::vector<int> &jobs, std::vector<std::vector<HStem>> &stems)
{
    // (jobs with caller matrices, has_ext == 1: the stem filters of RunAlgo re-sum the cells of the caller's score
    // matrix, which algo_collect reads back from the dense arena like a weighted matrix)
    // AnnotateStems(bool, score, rbps, [], minlen, minbpscore)  (:553)
    std::vector<HStruct> hs(jobs.size());
    std::vector<SView> views(jobs.size());
    for (size_t k = 0; k < jobs.size(); k++) { hs[k].job = jobs[k]; views[k] = SView{jobs[k], 1.0, &hs[k]}; }
    return sq_run_round(b, views, 1, stems);
}

// RunAlgo's matching for `jobs` in chunks that fit `arena` bytes of the (idle) candidate arena: built, launched and collected
// one after the other
static int run_chunks(sq_batch *b, const std::vector<int> &jobs, const std::vector<std::vector<HStem>> &stems, int algo, size_t arena,
                      int levellimit_opt, std::vector<std::vector<HStem>> &out)
{
    for (size_t k0 = 0; k0 < jobs.size();) {
        SqAlgoChunk ck;
        int r = algo_build(b, jobs, stems, k0, algo, arena, 3, ck);
        if (r) return r;
        if (ck.k1 == k0) { sq_set_error("sequence too long for the matching scratch"); return -3; }
        r = algo_launch(b, ck, (char *)b->scan.cands, b->stream);
        if (r) return r;
        r = algo_collect(b, jobs, stems, ck, levellimit_opt, out);
        if (r) return r;
        k0 = ck.k1;
    }
    return 0;
}

int sq_run_algo(sq_batch *b, const std::vector<int> &jobs, int algo, int levellimit_opt,
                std::vector<std::vector<HStem>> &out)
{
    out.assign(jobs.size(), {});
    if (jobs.empty()) return 0;
    std::vector<std::vector<HStem>> stems;
    const int r = algo_annotate(b, jobs, stems);
    if (r) return r;
    return run_chunks(b, jobs, stems, algo, (size_t)(b->cand_records - b->cand_reserved) * sizeof(SqCand), levellimit_opt, out);
}

// ---- asynchronous form used by sq_fold: E, H and N run on side streams, in scratch reserved at the end of
// the candidate arena, while the greedy rounds proceed on the batch stream ------------------------------
struct SqAlgoAsync {
    struct Item { int algo; std::vector<int> jobs; std::vector<std::vector<HStem>> stems; SqAlgoChunk ck; bool staged = false; };
    std::vector<Item> items;
    bool dev = false;                             // the whole of RunAlgo runs on the device (sq_algos_dev.hip)
    SqAlgoSize *h_sizes = nullptr;                // pinned: per job of all items, in item order
};
bool sq_algos_on_device(const SqAlgoAsync *pa) { return pa && pa->dev; }

// Region of an item that runs as ONE chunk with staging slot `sidx`: Hungarian / Nussinov in the batch's own scratch when the
// chunk fits it (planned from the lengths), else carved downwards from the end of the candidate arena, of which free_rec
// records may be lent.  *region stays null (and it.ck empty) when the item does not fit as one chunk.
static int place_item(sq_batch *b, SqAlgoAsync::Item &it, int sidx, int64_t free_rec, const SqAlgoSize *dev_sizes, char **region)
{
    *region = nullptr;
    if (it.algo != SQ_ALGO_E && b->algo_bytes > b->algo_used + 65536) {
        const size_t room = b->algo_bytes - b->algo_used;
        const int r = algo_build(b, it.jobs, it.stems, 0, it.algo, room, sidx, it.ck, dev_sizes);
        if (r) return r;
        if (it.ck.k1 == it.jobs.size() && it.ck.carve.bytes + 256 <= room) {
            *region = b->algo_scratch + b->algo_used;
            b->algo_used += sq_up256(it.ck.carve.bytes + 256);
            return 0;
        }
        it.ck = SqAlgoChunk();
    }
    if (free_rec <= 0) return 0;
    const int r = algo_build(b, it.jobs, it.stems, 0, it.algo, (size_t)free_rec * sizeof(SqCand), sidx, it.ck, dev_sizes);
    if (r) return r;
    if (it.ck.k1 != it.jobs.size()) { it.ck = SqAlgoChunk(); return 0; }
    b->cand_reserved += (int64_t)((it.ck.carve.bytes + 256 + sizeof(SqCand) - 1) / sizeof(SqCand));
    char *at = (char *)(b->scan.cands + (b->cand_records - b->cand_reserved));
    *region = (char *)(((uintptr_t)at + 255) & ~(uintptr_t)255);
    return 0;
}

// ---- RunAlgo on the device (sq_algos_dev.hip): one AnnotateStems round for the jobs of all three algorithms with the
// stems left in the arena, the sizes to the host (the plan of every item's chunk), the edge lists written by a kernel, the
// matching kernels on the side streams as before, and behind each of them the kernel that applies RunAlgo's filters and
// appends the job's stemset to the device log of final structures.  The host neither sees stems nor matchings.
// algos_begin_dev runs the stages below in order; what one stage leaves for the next is in SqAlgoDevRun.
struct SqAlgoDevRun {
    std::vector<int> all;                         // the jobs of all items, in item order: the structures of the round
    std::vector<uint8_t> need_raw;                // per job: its edge weights go through the host libm
    size_t raw_cap = 0;
    int maxn = 0, tmax = 1;
    size_t fin_lds = 0;
    char *pin = nullptr;                          // staging slot 3: [sizes][round records][need_raw][raw list]
    size_t o_aj = 0;
    SqAlgoRaw raw{nullptr, nullptr, nullptr, 0};
    int64_t cands_used = 0;
    double t_sizes = 0;                           // (SQ_TIMING) when the sizes had arrived
    std::vector<char *> regions;                  // per item
    int S() const { return (int)all.size(); }
};

// stage 1: does the batch qualify?  0: yes; 1: no (nothing happened that the host-driven form cannot repeat)
static int dev_qualify(sq_batch *b, SqAlgoAsync *pa, SqAlgoDevRun &D)
{
    const bool off = b->sw.no_device_algos;                             // (per fold: tests compare both forms in one process)
    if (off || pa->items.empty()) return 1;
    for (auto &it : pa->items) {
        for (int j : it.jobs) {
            const SqJob &J = b->jobs[j];
            D.maxn = std::max(D.maxn, J.n);
            uint8_t nr = 0;
            if (it.algo != SQ_ALGO_N) {
                // Edmonds / Hungarian weigh an edge with stemscore ** 1.7 from the host libm: on the device that is a table
                // lookup when the score is k 2^-q exactly (dyadic weights, no reactivity factors); the other jobs -- decided
                // per JOB -- leave their stem scores in pinned memory and the host raises them in bulk (SqAlgoRaw)
                if (J.mat64_off >= 0 || J.mulsh) return 1;
                if (!J.default_reacts || b->psets_dev[J.pset].pow_len <= 0) { nr = 1; D.raw_cap += (size_t)4 * J.n + 64; }
            }
            D.all.push_back(j);
            D.need_raw.push_back(nr);
        }
    }
    if (D.raw_cap && sq_tuning().no_algo_raw) return 1;      // (measurement: such batches take the host-driven form)
    if (D.maxn > SQ_ALGO_MAXN || D.maxn < 1) return 1;
    D.tmax = std::max(b->chain_tmax, 1);
    D.fin_lds = sq_algo_finish_lds(D.maxn, D.tmax);
    return D.fin_lds > 150 * 1024 ? 1 : 0;
}

// stage 2: the AnnotateStems round with the sizes of all jobs into pinned memory, then the raw stem scores raised on the host
static int dev_annotate(sq_batch *b, SqAlgoAsync *pa, SqAlgoDevRun &D)
{
    const int S = D.S();
    // pinned: the sizes of all jobs (slot 3 of the staging buffers is free while a fold runs)
    // (and, behind them, the per-job records the edges kernel reads: one allocation, the buffer must not move in between)
    D.o_aj = sq_up256(sizeof(SqAlgoSize) * (size_t)S);
    const size_t o_need = sq_up256(D.o_aj + sizeof(SqAlgoJob) * (size_t)S);
    const size_t o_raw = sq_up256(o_need + (size_t)S);
    D.pin = stage_buffer(b, 3, o_raw + 8 * D.raw_cap + 256);
    if (!D.pin) return 2;
    pa->h_sizes = (SqAlgoSize *)D.pin;
    if (D.raw_cap) {
        memcpy(D.pin + o_need, D.need_raw.data(), (size_t)S);
        D.raw.need = (const uint8_t *)(D.pin + o_need); D.raw.vals = (double *)(D.pin + o_raw);
        D.raw.ctr = b->d_fin_ctr + 8;                       // (a word of the fold's counter block: zero since sq_fold_begin_kernel)
        D.raw.cap = (uint32_t)std::min<size_t>(D.raw_cap, 0x7FFFFFF0u);
    }
    const int r = sq_round_annotate_dev(b, D.all, pa->h_sizes, &D.cands_used, D.raw);
    if (r) return r;                                       // (1: does not fit one round)
    D.t_sizes = sq_now();
    if (!D.raw_cap) return 0;
    // stemscore ** 1.7 with the host's libm, in place (the reference: Python's float ** on every stem, SQRNalgos.py:101,122)
    CpuScope cpu_(2);
    std::vector<std::pair<int, int>> spans;
    size_t total = 0;
    for (int s2 = 0; s2 < S; s2++)
        if (D.need_raw[s2]) {
            const SqAlgoSize &z = pa->h_sizes[s2];
            if (z.raw_base < 0) return 1;               // the list had no room: the host-driven form takes the batch
            spans.push_back({z.raw_base, z.nok}); total += (size_t)z.nok;
        }
    auto one = [&](int k) { double *v = D.raw.vals + spans[k].first; for (int q = 0; q < spans[k].second; q++) v[q] = pow(v[q], 1.7); };
    if (total >= 32768) sq_pool(b)->parallel_for((int)spans.size(), one);
    else for (int k = 0; k < (int)spans.size(); k++) one(k);
    return 0;
}

// stage 3: the plan of every item (algo_build without stems) and its region (place_item); an item that does not fit as one chunk
// sends the batch to the host-driven form
static int dev_place(sq_batch *b, SqAlgoAsync *pa, SqAlgoDevRun &D)
{
    const int64_t half = b->cand_records / 2;
    size_t base = 0;
    D.regions.assign(pa->items.size(), nullptr);
    b->algo_used = 0;
    for (size_t q = 0; q < pa->items.size(); q++) {
        auto &it = pa->items[q];
        const int64_t free_rec = std::min<int64_t>(half - b->cand_reserved, b->cand_records - b->cand_reserved - D.cands_used);
        // (algo_build indexes dev_sizes by k0 + q of the item's own list)
        const int r = place_item(b, it, (int)q, free_rec, pa->h_sizes + base, &D.regions[q]);
        if (r) return r;
        if (!D.regions[q]) { b->cand_reserved = 0; return 1; }
        base += it.jobs.size();
    }
    return 0;
}

// stage 4: the per-job records of the edges / finish kernels.  The edges kernel takes one record per structure of the round:
// all items' records, contiguous, in round order (behind the sizes in slot 3); the finish kernel of an item takes the item's
static void dev_fill_jobs(SqAlgoAsync *pa, SqAlgoDevRun &D)
{
    SqAlgoJob *round_aj = (SqAlgoJob *)(D.pin + D.o_aj);
    size_t base = 0;
    for (size_t q = 0; q < pa->items.size(); q++) {
        auto &it = pa->items[q];
        const std::vector<SqMatchJob> &mj = it.ck.mj;
        const SqAlgoCarve &cv = it.ck.carve;
        size_t vid = 0;
        for (size_t k = 0; k < mj.size(); k++) {
            SqAlgoJob aj;
            aj.job = it.jobs[k]; aj.algo = it.algo;
            aj.edges = (SqMatchEdge *)(D.regions[q] + cv.o_edges) + mj[k].edge_off;
            aj.vid2pos = (int32_t *)(D.regions[q] + cv.o_vid) + vid;
            aj.raw = D.need_raw[base + k] ? D.raw.vals + pa->h_sizes[base + k].raw_base : nullptr;
            if (it.algo == SQ_ALGO_E) vid += (size_t)mj[k].n;
            it.ck.p_aj[k] = aj;
            round_aj[base + k] = aj;
        }
        base += mj.size();
    }
}

// stage 5: the edges kernel on the batch stream (it owns the arena); edges_ev marks its end
static int dev_launch_edges(sq_batch *b, SqAlgoAsync *pa, SqAlgoDevRun &D)
{
    hipStream_t st = b->stream;
    const int S = D.S();
    const SqAlgoJob *round_aj = (const SqAlgoJob *)(D.pin + D.o_aj);
    const int maxn_lds = (std::min(b->maxn, SQ_ALGO_MAXN) + 7) & ~7;   // (the device RunAlgo only takes batches up to SQ_ALGO_MAXN nt)
    SqAlgoStatPtrs zs{{nullptr, nullptr, nullptr}};
    for (size_t q = 0; q < pa->items.size() && q < 3; q++) zs.p[q] = (SqAlgoStat *)(D.regions[q] + pa->items[q].ck.carve.o_stat);
    // the stem lists in LDS when the longest of the launch fits
    int nokcap = 0;
    for (int s2 = 0; s2 < S; s2++) nokcap = std::max(nokcap, (int)pa->h_sizes[s2].nok);
    nokcap = (nokcap + 63) & ~63;
    // (up to 6,144 stems -- 130 KB, a block per CU: the other form ranks every stem against ALL the keys in global memory,
    // O(stems^2): 15-25 ms for the 1,500 jobs of 500 records of 500 nt, in front of the greedy loop on the batch's stream)
    if (nokcap > 6144 || sq_algo_edges_lds(maxn_lds, nokcap) > 150 * 1024 || b->sw.no_edges_lds) nokcap = 0;
    if (sq_algo_edges_lds(maxn_lds, nokcap) > 48 * 1024) sq_max_dynamic_lds((const void *)sq_algo_edges_kernel, 160 * 1024);
    // (one wave per job on a crowded chip: the work of a job is a few hundred stems behind a handful of trips to L2, and
    // three waves that mostly wait held three wave slots -- sizes + edges were 7 % of a crowded step's wave cycles)
    const bool crowded_k = sq_algo_crowded(b->inflight, (size_t)b->njobs);
    // (the jobs' records to the device first when the scratch has room behind the items' regions: from the pinned table
    // every block of the kernel began with a read over PCIe)
    const SqAlgoJob *edges_aj = round_aj;
    const size_t at = sq_up256(b->algo_used), need = (size_t)S * sizeof(SqAlgoJob);
    if (b->algo_scratch && at + need <= b->algo_bytes && !sq_tuning().no_state_copy) {
        HIPCK(hipMemcpyAsync(b->algo_scratch + at, round_aj, need, hipMemcpyHostToDevice, st));
        edges_aj = (const SqAlgoJob *)(b->algo_scratch + at);
    }
    hipLaunchKernelGGL(sq_algo_edges_kernel, dim3(S), dim3(crowded_k ? 64 : 256), sq_algo_edges_lds(maxn_lds, nokcap), st, b->ctx, b->lane_full.d_structs,
                       [&] { SqScanArgs a = b->scan; a.ctr = b->lane_full.d_ctr; return a; }(), edges_aj, maxn_lds, zs, nokcap);
    HIPCK(hipGetLastError());
    if (!b->class_ev) HIPCK(sq_event_get(b->device, &b->class_ev));
    if (!b->edges_ev) HIPCK(sq_event_get(b->device, &b->edges_ev));
    HIPCK(hipEventRecord(b->edges_ev, st));
    return 0;
}

// stage 6, per item, on side stream `sidx`: its tables to the region, the matching kernels in size classes, the finish kernel
// (RunAlgo's filters, the stemsets to the device log) and the kernel that publishes statistics and completion word
static int dev_launch_item(sq_batch *b, SqAlgoAsync::Item &it, int sidx, char *region, const SqAlgoDevRun &D, int levellimit_opt)
{
    SqAlgoChunk &ck = it.ck;
    const SqAlgoCarve &cv = ck.carve;
    const int ss = side_of(b, sidx);
    if (!b->side[ss]) { if (sq_check(sq_stream_get(b->device, &b->side[ss]), "hipStreamCreate")) return 2; }
    hipStream_t cs = b->side[ss];
    HIPCK(hipStreamWaitEvent(cs, b->edges_ev, 0));
    ck.st = cs;
    int32_t *d_out = (int32_t *)(region + cv.o_out), *d_cnt = (int32_t *)(region + cv.o_cnt);
    SqAlgoStat *d_stat = (SqAlgoStat *)(region + cv.o_stat);
    if (sidx >= 3) HIPCK(hipMemsetAsync(d_stat, 0, sizeof(SqAlgoStat), cs));   // (the first three: zeroed by the edges kernel)
    const int nj = (int)ck.mj.size();
    // The finish kernel's two records per job go to the device first: from the pinned table every one of its waves began
    // with two reads over PCIe (and the publish kernel's wave walks the table): microseconds in a wave that works for a few.
    SqMatchJob *const dev_mj = (SqMatchJob *)(region + cv.o_jobs);
    SqAlgoJob *const dev_aj = (SqAlgoJob *)(region + cv.o_aj);
    HIPCK(hipMemcpyAsync(dev_mj, ck.p_mj, (size_t)nj * sizeof(SqMatchJob), hipMemcpyHostToDevice, cs));
    HIPCK(hipMemcpyAsync(dev_aj, ck.p_aj, (size_t)nj * sizeof(SqAlgoJob), hipMemcpyHostToDevice, cs));
    hipEvent_t pe0;
    const int pslot = it.algo == SQ_ALGO_E ? 4 : it.algo == SQ_ALGO_H ? 5 : 6;
    sq_prof_begin(b, pslot, cs, &pe0);
    // Edmonds folded alone: its first class (the largest graphs, the critical path) on this stream, the others in front of the
    // short kernels on their stream, joined before the finish kernel
    hipStream_t other = nullptr;
    if (it.algo == SQ_ALGO_E && ck.classes.size() > 1 && side_of(b, 3) != ss) {
        const int s2 = side_of(b, 3);
        if (!b->side[s2]) { if (sq_check(sq_stream_get(b->device, &b->side[s2]), "hipStreamCreate")) return 2; }
        other = b->side[s2];
        HIPCK(hipStreamWaitEvent(other, b->edges_ev, 0));
    }
    const int rl = launch_classes(b, ck, region, (const SqMatchEdge *)(region + cv.o_edges), d_out, d_cnt, nullptr, cs, other);
    if (rl) return rl;
    sq_prof_end(b, pslot, cs, pe0);
    hipLaunchKernelGGL(sq_algo_finish_kernel, dim3(nj), dim3(64), D.fin_lds, cs, b->ctx, dev_aj, dev_mj, d_out, d_cnt, levellimit_opt,
                       b->d_fin, b->d_fin_stems, b->d_fin_ctr, b->fin_cap, b->fin_stem_cap, d_stat, D.tmax);
    hipLaunchKernelGGL(sq_algo_publish_kernel, dim3(1), dim3(64), 0, cs, d_stat, ck.h_stats, dev_mj, d_out, it.algo == SQ_ALGO_E ? 1 : 0,
                       ck.flag, ck.flag_val, nj);
    HIPCK(hipGetLastError());
    it.staged = true;
    return 0;
}

// Returns 0: staged, 1: the batch does not qualify (nothing happened that the host-driven form cannot repeat).
static int algos_begin_dev(sq_batch *b, SqAlgoAsync *pa, int levellimit_opt)
{
    SqAlgoDevRun D;
    int r = dev_qualify(b, pa, D);
    if (r) return r;
    const double tt0 = sq_now();
    r = dev_annotate(b, pa, D);
    if (r) return r;
    r = dev_place(b, pa, D);
    if (r) return r;
    dev_fill_jobs(pa, D);
    const double tt2 = sq_now();
    struct Rep { double t0, t1, t2; bool on; ~Rep() { if (on) fprintf(stderr, "[sq_algos] device RunAlgo: annotate round + wait for the sizes %.3f ms, layout %.3f ms, launches %.3f ms\n", (t1 - t0) * 1e3, (t2 - t1) * 1e3, (sq_now() - t2) * 1e3); } } rep_dev{tt0, D.t_sizes, tt2, b->sw.timing};
    r = dev_launch_edges(b, pa, D);
    if (r) return r;
    if (D.fin_lds > 64 * 1024) sq_max_dynamic_lds((const void *)sq_algo_finish_kernel, 160 * 1024);
    for (size_t q = 0; q < pa->items.size(); q++) {
        r = dev_launch_item(b, pa->items[q], (int)q, D.regions[q], D, levellimit_opt);
        if (r) return r;
    }
    pa->dev = true;
    return 0;
}

// waits for the device-side RunAlgo of a fold (the stemsets are in the device log by then)
static int algos_end_dev(sq_batch *b, SqAlgoAsync *pa)
{
    int r = 0;
    for (size_t q = pa->items.size(); q-- > 0 && !r;) {
        SqAlgoChunk &ck = pa->items[q].ck;
        r = sq_wait_word(b, ck.flag, ck.flag_val, ck.st, "matching kernel");
        if (r) break;
        const SqAlgoStat hs = *ck.h_stats;
        if (hs.bad == 1) { sq_set_capacity_error(SQ_CAP_FIXED, "blossom capacity exceeded"); r = -3; }
        else if (hs.bad) { sq_set_capacity_error(SQ_CAP_FIXED, "stem capacity of RunAlgo's filters exceeded"); r = -3; }
        else if (hs.level_ovf) { sq_set_error("more than 64 pseudoknot levels"); r = -3; }
        if (pa->items[q].algo == SQ_ALGO_E && hs.graphs) {
            std::lock_guard<std::mutex> lk(b->mwm_mu);
            b->mwm_stats[0] += (int64_t)hs.graphs; b->mwm_stats[1] += (int64_t)hs.passes;
            const int64_t np = (int64_t)(hs.max_pass_job >> 32);
            if (np > b->mwm_stats[2]) { b->mwm_stats[2] = np; b->mwm_stats[3] = hs.max_events; b->mwm_stats[4] = hs.max_n; b->mwm_stats[5] = hs.max_m; }
        }
    }
    for (int k = 0; k < 4; k++) if (b->side[k]) hipStreamSynchronize(b->side[k]);
    b->cand_reserved = 0;
    return r;
}

int sq_algos_begin(sq_batch *b, const std::vector<uint32_t> &algos, SqAlgoAsync *&pa, int levellimit_opt, bool want_dev)
{
    pa = new SqAlgoAsync();
    b->algo_used = 0;
    for (int algo : {SQ_ALGO_E, SQ_ALGO_H, SQ_ALGO_N}) {
        SqAlgoAsync::Item it;
        it.algo = algo;
        for (int j = 0; j < b->njobs; j++) if (algos[j] & (uint32_t)algo) it.jobs.push_back(j);
        if (it.jobs.empty()) continue;
        pa->items.push_back(std::move(it));
    }
    if (pa->items.empty()) return 0;
    if (want_dev) {
        const int rd = algos_begin_dev(b, pa, levellimit_opt);
        if (rd == 0) return 0;
        if (rd != 1) return rd;
        for (auto &it : pa->items) { it.ck = SqAlgoChunk(); it.staged = false; }   // the host-driven form, from scratch
        b->algo_used = 0; b->cand_reserved = 0;
    }
    const bool async = !b->sw.algo_sync;
    const int64_t half = b->cand_records / 2;          // at most half of the arena is lent to the matching kernels
    int sidx = 0;
    // Edmonds is the long pole: its AnnotateStems pass and launch go first, alone; the other algorithms share
    // one more pass.  Everything that is staged runs on side streams while the caller proceeds.
    auto stage = [&](SqAlgoAsync::Item &it) -> int {
        const double ts0 = sq_now();
        struct Rep { int algo; double t0; bool on; ~Rep() { if (on) fprintf(stderr, "[sq_algos] stage algo %d: %.3f ms\n", algo, (sq_now() - t0) * 1e3); } } rep{it.algo, ts0, b->sw.timing};
        if (!async || sidx >= 3) return 0;
        char *region = nullptr;
        const int rb = place_item(b, it, sidx, half - b->cand_reserved, nullptr, &region);
        if (rb || !region) return rb;                       // (does not fit as one chunk: synchronous later)
        const int ss = side_of(b, sidx);
        if (!b->side[ss]) { if (sq_check(sq_stream_get(b->device, &b->side[ss]), "hipStreamCreate")) return 2; }
        const double tl0 = sq_now();
        hipStream_t st2 = nullptr;
        if (it.algo == SQ_ALGO_E && side_of(b, 3) != ss) {               // the stream of the smaller classes (created here if need be)
            const int s2 = side_of(b, 3);
            if (!b->side[s2]) { if (sq_check(sq_stream_get(b->device, &b->side[s2]), "hipStreamCreate")) return 2; }
            st2 = b->side[s2];
        }
        const int r = algo_launch(b, it.ck, region, b->side[ss], st2);
        if (b->sw.timing) fprintf(stderr, "[sq_algos] launch algo %d: %.3f ms\n", it.algo, (sq_now() - tl0) * 1e3);
        if (r) return r;
        it.staged = true;
        sidx++;
        return 0;
    };
    size_t first_rest = 0;
    const double ta0 = sq_now();
    if (pa->items[0].algo == SQ_ALGO_E) {
        int r = algo_annotate(b, pa->items[0].jobs, pa->items[0].stems);
        if (r) return r;
        if (b->sw.timing) fprintf(stderr, "[sq_algos] annotate E %.3f ms\n", (sq_now() - ta0) * 1e3);
        r = stage(pa->items[0]);
        if (r) return r;
        first_rest = 1;
    }
    std::vector<int> all;
    for (size_t q = first_rest; q < pa->items.size(); q++) all.insert(all.end(), pa->items[q].jobs.begin(), pa->items[q].jobs.end());
    if (!all.empty()) {
        std::vector<std::vector<HStem>> stems;
        int r = algo_annotate(b, all, stems);
        if (r) return r;
        size_t pos = 0;
        for (size_t q = first_rest; q < pa->items.size(); q++) {
            auto &it = pa->items[q];
            it.stems.assign(std::make_move_iterator(stems.begin() + pos), std::make_move_iterator(stems.begin() + pos + it.jobs.size()));
            pos += it.jobs.size();
            r = stage(it);
            if (r) return r;
        }
    }
    if (b->sw.timing) fprintf(stderr, "[sq_algos] annotate + stage %.3f ms\n", (sq_now() - ta0) * 1e3);
    return 0;
}

void sq_algos_abandon(sq_batch *b, SqAlgoAsync *pa)
{
    for (int k = 0; k < 4; k++) if (b->side[k]) hipStreamSynchronize(b->side[k]);
    b->cand_reserved = 0;
    delete pa;
}

int sq_algos_end(sq_batch *b, SqAlgoAsync *pa, int levellimit_opt, std::vector<JobSets> &sets, const SqAlgoEndHooks *hooks)
{
    int r = 0;
    if (pa->dev) { r = algos_end_dev(b, pa); delete pa; return r; }
    // collect staged work first, release the reservation, then run what was not staged
    for (auto &it : pa->items) {
        JobSets js; js.algo = it.algo; js.jobs = it.jobs; js.sets.assign(it.jobs.size(), {});
        sets.push_back(std::move(js));
    }
    bool all_staged = true;
    for (auto &it : pa->items) all_staged &= it.staged;
    const bool stream_e = hooks && all_staged && !pa->items.empty() && pa->items[0].algo == SQ_ALGO_E && pa->items[0].ck.job_flags;
    // last staged first: the short kernels (N, H) are done long before Edmonds, so their host filters run
    // while the blossom kernel is still busy
    for (size_t q = pa->items.size(); q-- > (stream_e ? 1 : 0);) {
        auto &it = pa->items[q];
        if (it.staged && !r) r = algo_collect(b, it.jobs, it.stems, it.ck, levellimit_opt, sets[q].sets);
    }
    if (stream_e && !r) {
        // Edmonds job by job: the caller first takes the H / N stemsets, then every sequence is finished (filters +
        // its ranking tail, in the hook) as soon as its graph is matched -- only the largest graph is waited for
        hooks->after_short(sets);
        auto &it = pa->items[0];
        sets[0].streamed = true;
        const std::function<void(size_t)> cb = [&](size_t k) { hooks->on_e_job(it.jobs[k], sets[0].sets[k]); };
        r = algo_collect(b, it.jobs, it.stems, it.ck, levellimit_opt, sets[0].sets, &cb);
    }
    for (int k = 0; k < 4; k++) if (b->side[k]) hipStreamSynchronize(b->side[k]);
    b->cand_reserved = 0;
    size_t q = 0;
    for (auto &it : pa->items) {
        JobSets &js = sets[q++];
        if (it.staged || r) continue;
        if (it.stems.size() != it.jobs.size()) {          // (sq_algos_begin stopped before this item's AnnotateStems pass)
            r = algo_annotate(b, it.jobs, it.stems);
            if (r) break;
        }
        r = run_chunks(b, it.jobs, it.stems, it.algo, (size_t)b->cand_records * sizeof(SqCand), levellimit_opt, js.sets);
    }
    delete pa;
    return r;
}
extern "C" int sq_run_algos(sq_batch *b, int32_t njob, const int32_t *job_ids, int32_t algo, int32_t levellimit,
                            sq_stem *out, int32_t out_cap, int32_t *out_off)
{
    if (!b || njob < 0 || (algo != SQ_ALGO_E && algo != SQ_ALGO_H && algo != SQ_ALGO_N)) { sq_set_error("bad argument"); return -1; }
    SqSlackGuard slack_guard;
    std::vector<int> jobs(job_ids, job_ids + njob);
    for (int j : jobs) if (j < 0 || j >= b->njobs) { sq_set_error("bad job index"); return -1; }
    std::vector<std::vector<HStem>> res;
    int r = sq_run_algo(b, jobs, algo, levellimit, res);
    if (r) return r;
    int32_t o = 0;
    for (int k = 0; k < njob; k++) {
        out_off[k] = o;
        for (const HStem &t : res[k]) {
            if (o >= out_cap) { sq_set_error("out_cap too small"); return -3; }
            out[o++] = sq_stem{t.i, t.j, t.len, 0, t.bps, t.fin};
        }
    }
    out_off[njob] = o;
    return 0;
}
