// Test-only host harness of the plan of a matching chunk (squarna_amd/csrc/sq_algo_plan.h), compiled without HIP.
//   no argument: stdin holds cases, one per line; stdout gets one JSON object per case with the keys of tests/golden/algo_plan.json.gz
//     C algo inflight region_bytes dev lsap_classes mwm_classes nj  n ncell  n ncell ...      (a chunk)
//     M inflight bin_waves bin_bytes all_cap nolds nj  n m  n m ...                          (the LDS bins of one blossom launch,
//                                                                                             "hdr" and the kernel's "forms" besides)
//     N inflight nuss_threads nj  n m  n m ...                                               (the block size of one Nussinov launch)
//     S n m                                                                                   (the sizes of one graph's blossom state)
//   "props": the layout and ordering properties on synthetic job lists; prints the number of plans checked, exit 1 on a failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../squarna_amd/csrc/sq_algo_plan.h"

static long long sz(size_t x) { return x == SQ_PLAN_NONE ? -1 : (long long)x; }

static void print_chunk(const SqAlgoPlan &P)
{
    const SqAlgoCarve &c = P.carve;
    const SqAlgoStage &s = P.stage;
    printf("{\"k1\":%zu,\"bytes\":%zu,\"scratch\":%zu,\"outints\":%zu,\"nedges\":%zu,\"vids\":%zu,", P.mj.size(), c.bytes, P.scratch, P.outints, P.nedges, P.vids);
    printf("\"carve\":{\"o_edges\":%zu,\"o_out\":%zu,\"o_cnt\":%zu,\"o_vid\":%zu,\"o_stat\":%zu,\"o_aj\":%zu,\"o_scr\":%zu},", c.o_edges, c.o_out, c.o_cnt,
           c.o_vid, c.o_stat, c.o_aj, c.o_scr);
    printf("\"stage\":{\"jobs\":%lld,\"edges\":%lld,\"out\":%lld,\"cnt\":%lld,\"flag\":%lld,\"job_flags\":%lld,\"bin_head\":%lld,\"p_mj\":%lld,\"p_aj\":%lld,"
           "\"h_stats\":%lld,\"total\":%lld},", sz(s.jobs), sz(s.edges), sz(s.out), sz(s.cnt), sz(s.flag), sz(s.job_flags), sz(s.bin_head), sz(s.p_mj),
           sz(s.p_aj), sz(s.h_stats), sz(s.bytes));
    printf("\"need\":[");
    for (size_t q = 0; q < P.need.size(); q++) printf("%s%zu", q ? "," : "", P.need[q]);
    printf("],\"sorted_pos\":[");
    for (size_t q = 0; q < P.sorted_pos.size(); q++) printf("%s%d", q ? "," : "", P.sorted_pos[q]);
    printf("],\"classes\":[");
    for (size_t k = 0; k < P.classes.size(); k++) printf("%s[%d,%d]", k ? "," : "", P.classes[k].start, P.classes[k].count);
    printf("]}\n");
}

static int replay()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'C') {
            int algo, inflight, dev, nj;
            size_t region;
            SqAlgoKnobs kn;
            if (scanf("%d %d %zu %d %d %d %d", &algo, &inflight, &region, &dev, &kn.lsap_classes, &kn.mwm_classes, &nj) != 7) return 1;
            std::vector<SqAlgoJobSize> jb((size_t)nj);
            for (auto &B : jb) {
                int n; size_t ncell;
                if (scanf("%d %zu", &n, &ncell) != 2) return 1;
                B = sq_algo_job_size(algo, n, ncell);
            }
            SqAlgoPlan P;
            sq_algo_plan_chunk(algo, jb.data(), jb.size(), region, dev != 0, inflight, kn, P);
            print_chunk(P);
        } else if (kind == 'M') {
            int inflight, nolds, nj;
            SqAlgoKnobs kn;
            if (scanf("%d %d %ld %ld %d %d", &inflight, &kn.mwm_bin_waves, &kn.mwm_bin_bytes, &kn.mwm_all_cap, &nolds, &nj) != 6) return 1;
            kn.mwm_nolds = nolds != 0;
            std::vector<SqMatchJob> jobs((size_t)nj);
            for (auto &J : jobs) { J = SqMatchJob(); if (scanf("%d %d", &J.n, &J.nedges) != 2) return 1; }
            std::vector<SqMatchJob> rw(jobs);
            std::vector<int32_t> head((size_t)nj + 1, -7);
            const SqMwmPlan M = sq_mwm_plan(jobs.data(), rw.data(), nj, head.data(), inflight, kn, false);
            printf("{\"nbins\":%d,\"waves\":%d,\"lds\":%zu,\"all_in_lds\":%d,\"slices\":[", M.nbins, M.waves, M.lds, M.all_in_lds ? 1 : 0);
            for (int q = 0; q < nj; q++) printf("%s[%d,%d,%d]", q ? "," : "", rw[q].lds_off, rw[q].lds_bytes, rw[q].next);
            printf("],\"bin_head\":[");
            for (int k = 0; k < M.nbins; k++) printf("%s%d", k ? "," : "", head[k]);
            // the storage form the KERNEL takes for every graph (the two tests at the top of sq_mwm_one; -1: no vertex): a
            // one-graph block sees the launch-wide LDS less the algorithm object, a wave of a bin its own slice less the object
            const size_t hdr = sq_blossom_hdr();
            printf("],\"hdr\":%zu,\"forms\":[", hdr);
            for (int q = 0; q < nj; q++) {
                const int n = jobs[q].n, m = jobs[q].nedges;
                const size_t have = M.waves == 1 ? M.lds : (size_t)rw[q].lds_bytes;
                const size_t lds_bytes = have > hdr ? have - hdr : 0;
                const size_t ebytes = ((size_t)m * sizeof(SqMatchEdge) + 15) & ~(size_t)15;
                int form = 0;
                if (n <= 0) form = -1;
                else if (SqBlossom::scratch_bytes(n, m, 1) + ebytes + 16 <= lds_bytes) form = 1;
                else if (SqBlossom::hot_bytes(n, m, 2) + 16 <= lds_bytes) form = 2;
                printf("%s%d", q ? "," : "", form);
            }
            printf("]}\n");
        } else if (kind == 'N') {
            int inflight, nj, maxn = 0;
            SqAlgoKnobs kn;
            if (scanf("%d %d %d", &inflight, &kn.nuss_threads, &nj) != 3) return 1;
            std::vector<SqMatchJob> jobs((size_t)nj);
            for (auto &J : jobs) { J = SqMatchJob(); if (scanf("%d %d", &J.n, &J.nedges) != 2) return 1; maxn = std::max(maxn, (int)J.n); }
            printf("{\"threads\":%d}\n", sq_nussinov_threads(jobs.data(), nj, maxn, inflight, kn));
        } else if (kind == 'S') {
            int n, m;
            if (scanf("%d %d", &n, &m) != 2) return 1;
            printf("{\"hdr\":%zu,\"edge\":%zu", sq_blossom_hdr(), SqBlossom::edge_bytes(m));
            for (int t = 0; t < 3; t++)
                printf(",\"t%d\":[%zu,%zu,%zu,%d,%d,%d]", t, SqBlossom::hot_bytes(n, m, t), SqBlossom::cold_bytes(n, m, t), SqBlossom::scratch_bytes(n, m, t),
                       t == 2 ? SqBlossom::queue_hot_cap(n) : SqBlossom::queue_cap(n, m, t), SqBlossom::pool_capacity(n, m, t ? 1 : 0), SqBlossom::frame_ints(n, t ? 1 : 0));
            printf("}\n");
        } else return 1;
    }
    return 0;
}

// ---- properties ----
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// want_k1 < 0: at least -want_k1 jobs
static void check_plan(int algo, const std::vector<SqAlgoJobSize> &jb, size_t region, bool dev, int inflight, long want_k1, const char *tag)
{
    SqAlgoKnobs kn;
    SqAlgoPlan P;
    sq_algo_plan_chunk(algo, jb.data(), jb.size(), region, dev, inflight, kn, P);
    const size_t nq = P.mj.size();
    CHECK(want_k1 >= 0 ? (long)nq == want_k1 : (long)nq >= -want_k1, "%s: algo %d dev %d: %zu jobs admitted, %ld expected", tag, algo, (int)dev, nq, want_k1);
    const SqAlgoCarve &c = P.carve;
    const SqAlgoStage &s = P.stage;
    // every offset on a 256-byte boundary
    for (size_t o : {c.o_jobs, c.o_edges, c.o_out, c.o_cnt, c.o_vid, c.o_stat, c.o_aj, c.o_scr, s.jobs, s.edges, s.out, s.cnt, s.flag, s.bytes})
        CHECK(o % 256 == 0, "%s: offset %zu", tag, o);
    for (size_t o : {s.job_flags, s.bin_head, s.p_mj, s.p_aj, s.h_stats}) CHECK(o == SQ_PLAN_NONE || o % 256 == 0, "%s: offset %zu", tag, o);
    CHECK((s.job_flags != SQ_PLAN_NONE) == (algo == SQ_ALGO_E) && (s.bin_head != SQ_PLAN_NONE) == (algo == SQ_ALGO_E), "%s: flags of algo %d", tag, algo);
    CHECK((s.p_mj != SQ_PLAN_NONE) == dev && (s.p_aj != SQ_PLAN_NONE) == dev && (s.h_stats != SQ_PLAN_NONE) == dev, "%s: device tail", tag);
    // the parts of the region follow each other without overlap and end at carve.bytes
    struct Part { size_t at, bytes; };
    std::vector<Part> parts = {{c.o_jobs, nq * sizeof(SqMatchJob)}, {c.o_edges, P.nedges * sizeof(SqMatchEdge)}, {c.o_out, P.outints * 4}, {c.o_cnt, nq * 4}};
    if (dev) { parts.push_back({c.o_vid, P.vids * 4}); parts.push_back({c.o_stat, sizeof(SqAlgoStat)}); parts.push_back({c.o_aj, nq * sizeof(SqAlgoJob)}); }
    parts.push_back({c.o_scr, P.scratch});
    for (size_t k = 0; k + 1 < parts.size(); k++) CHECK(parts[k].at + parts[k].bytes <= parts[k + 1].at, "%s: region part %zu overlaps the next", tag, k);
    CHECK(c.o_jobs == 0 && c.o_scr + P.scratch == c.bytes, "%s: region ends", tag);
    if (nq) CHECK(c.bytes <= region, "%s: carve %zu beyond the region %zu the cut admitted the jobs into", tag, c.bytes, region);
    // ... and so do the parts of the staging buffer
    std::vector<Part> sp = {{s.jobs, nq * sizeof(SqMatchJob)}, {s.edges, dev ? 0 : P.nedges * sizeof(SqMatchEdge)}, {s.out, P.outints * 4}, {s.cnt, nq * 4}, {s.flag, 4}};
    if (algo == SQ_ALGO_E) { sp.push_back({s.job_flags, nq * 4}); sp.push_back({s.bin_head, nq * 4}); }
    if (dev) { sp.push_back({s.p_mj, nq * sizeof(SqMatchJob)}); sp.push_back({s.p_aj, nq * sizeof(SqAlgoJob)}); sp.push_back({s.h_stats, sizeof(SqAlgoStat)}); }
    sp.push_back({s.bytes, 0});
    for (size_t k = 0; k + 1 < sp.size(); k++) CHECK(sp[k].at + sp[k].bytes <= sp[k + 1].at, "%s: staging part %zu overlaps the next", tag, k);
    // the jobs' slices of scratch, results and edges
    size_t scr = 0, out = 0, edges = 0;
    for (size_t q = 0; q < nq; q++) {
        const SqMatchJob &m = P.mj[q];
        CHECK(m.n == jb[q].n && (size_t)m.nedges == jb[q].ncell, "%s: job %zu", tag, q);
        CHECK((size_t)m.scratch_off == scr && (size_t)m.edge_off == edges && (size_t)m.out_off * (algo == SQ_ALGO_N ? 2 : 1) == out, "%s: slices of job %zu", tag, q);
        CHECK(m.scratch_off % 256 == 0, "%s: scratch of job %zu", tag, q);
        scr += jb[q].need; out += jb[q].nout; edges += jb[q].ncell;
    }
    CHECK(scr == P.scratch && out == P.outints && edges == P.nedges, "%s: totals", tag);
    // the sorted table
    std::vector<int> seen(nq, 0);
    for (size_t q = 0; q < nq; q++) {
        const int r = P.sorted_pos[q];
        CHECK(r >= 0 && (size_t)r < nq, "%s: sorted_pos[%zu] = %d", tag, q, r);
        if (r < 0 || (size_t)r >= nq) continue;
        seen[r]++;
        const SqMatchJob &t = P.sorted[r], &m = P.mj[q];
        CHECK(t.pad == (int)q && t.n == m.n && t.nedges == m.nedges && t.edge_off == m.edge_off && t.scratch_off == m.scratch_off && t.out_off == m.out_off,
              "%s: row %d is not job %zu", tag, r, q);
    }
    for (size_t r = 0; r < nq; r++) CHECK(seen[r] == 1, "%s: row %zu taken %d times", tag, r, seen[r]);
    for (size_t r = 0; r + 1 < nq; r++) CHECK(P.need[P.sorted[r].pad] >= P.need[P.sorted[r + 1].pad], "%s: order at row %zu", tag, r);
    // the classes tile [0, nq)
    int at = 0;
    for (const SqAlgoClass &k : P.classes) { CHECK(k.start == at && k.count >= 1, "%s: class [%d +%d) at %d", tag, k.start, k.count, at); at += k.count; }
    CHECK((size_t)at == nq && (int)P.classes.size() <= std::max(1, sq_algo_max_classes(algo, inflight, nq, kn)) && (nq == 0) == P.classes.empty(), "%s: classes end at %d of %zu", tag, at, nq);
    if (algo != SQ_ALGO_E) return;
    // the LDS bins of every class's launch
    for (const SqAlgoClass &k : P.classes) {
        std::vector<SqMatchJob> rw(P.sorted.begin() + k.start, P.sorted.begin() + k.start + k.count);
        std::vector<int32_t> head((size_t)k.count, -7);
        const SqMwmPlan M = sq_mwm_plan(P.sorted.data() + k.start, rw.data(), k.count, head.data(), inflight, kn, false);
        std::vector<int> on(k.count, 0);
        CHECK(M.waves >= 1 && M.waves <= 8 && M.cap <= 150 * 1024 && M.lds % 256 == 0, "%s: bins of %d waves, %zu bytes", tag, M.waves, M.cap);
        for (int bin = 0; bin < M.nbins; bin++) {
            int cnt = 0; size_t bytes = 0;
            for (int row = head[bin]; row >= 0 && cnt <= k.count; row = rw[row].next) {
                CHECK(row < k.count, "%s: row %d", tag, row);
                if (row >= k.count) break;
                CHECK((size_t)rw[row].lds_off == bytes && rw[row].lds_bytes >= (int)sq_blossom_hdr(), "%s: slice of row %d", tag, row);
                on[row]++; cnt++; bytes += (size_t)rw[row].lds_bytes;
            }
            CHECK(cnt >= 1 && cnt <= M.waves && bytes <= M.cap && bytes <= M.lds, "%s: bin %d holds %d graphs in %zu bytes", tag, bin, cnt, bytes);
        }
        for (int row = 0; row < k.count; row++) CHECK(on[row] == 1, "%s: row %d is on %d chains", tag, row, on[row]);
    }
}

static int props()
{
    const int ns[6] = {1, 63, 64, 65, 150, 500};
    long plans = 0;
    for (int algo : {SQ_ALGO_E, SQ_ALGO_H, SQ_ALGO_N})
        for (int nj : {1, 2, 4, 5, 4096})
            for (int shift = 0; shift < 6; shift++)
                for (int dense = 0; dense < 2; dense++)
                    for (int dev = 0; dev < 2; dev++)
                        for (int inflight : {1, 3}) {
                            std::vector<SqAlgoJobSize> jb;
                            for (int q = 0; q < nj; q++) {
                                const int n = ns[(q + shift) % 6];
                                jb.push_back(sq_algo_job_size(algo, n, dense ? (size_t)n * n / 20 : 0));
                            }
                            char tag[96];
                            snprintf(tag, sizeof tag, "%d jobs from %d nt, %s, inflight %d", nj, ns[shift], dense ? "n^2/20 edges" : "no edges", inflight);
                            // regions that end the chunk after no job, after the first, and after all of them
                            const size_t one = sq_algo_cut_estimate(1, jb[0].ncell, jb[0].nout, (size_t)jb[0].n, dev != 0) + jb[0].need;
                            check_plan(algo, jb, one - 1, dev != 0, inflight, 0, tag);
                            // (the device form's estimate counts the CANDIDATE's n as vertices under Hungarian / Nussinov too, so a
                            // short second job can still get in where a long first one just fitted)
                            check_plan(algo, jb, one, dev != 0, inflight, dev && algo != SQ_ALGO_E ? -1 : 1, tag);
                            check_plan(algo, jb, (size_t)1 << 40, dev != 0, inflight, nj, tag);
                            plans += 3;
                        }
    printf("%ld plans checked, %d failures\n", plans, failures);
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "props")) return props();
    return replay();
}
