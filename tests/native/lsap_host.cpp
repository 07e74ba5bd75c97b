// Test-only host harness: runs the product's Hungarian restatement (squarna_amd/csrc/sq_lsap.h) on the CPU, one lane, so tests
// can compare it with scipy.optimize.linear_sum_assignment in every storage form without a GPU, and prints the layout and the
// launch decisions (sq_algo_plan.h) the kernel and sq_launch_matching take.
//   (no argument)  stdin: T, then per case "n m lds_bytes" and m lines "v w weight" (distinct cells, v < w).  lds_bytes plays
//                  the launch's dynamic LDS: the case runs in the form sq_lsap_form gives it.
//                  stdout: per case one line: the form (a, b, c), then col4row[0..n-1].
//   layout         stdin: lines "n m".  stdout: per line a JSON object: every array's [offset, element size, elements] -- the
//                  vectors from where they start (form a: LDS; "c_u": form c, global scratch), the sparse matrix from the
//                  start of LDS -- and the byte counts.
//   launch         stdin: lines "nj n m n m ...".  stdout: per line "need lds form form ...": sq_lsap_launch_lds, then the form of
//                  every job under it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../squarna_amd/csrc/sq_algo_plan.h"

static const char FORM[] = "abc";

static int run_cases()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        int n, m;
        long long lds_bytes;
        if (scanf("%d %d %lld", &n, &m, &lds_bytes) != 3) return 1;
        std::vector<SqMatchEdge> e(m);
        for (int k = 0; k < m; k++)
            if (scanf("%d %d %lf", &e[k].v, &e[k].w, &e[k].weight) != 3) return 1;
        const SqLsapForm form = sq_lsap_form(n, m, (size_t)lds_bytes);
        // as in the kernel: every job finds the launch's LDS, whatever its form; 0xA5: nothing may rely on zeroed memory
        std::vector<char> scratch(sq_lsap_scratch_bytes(n), (char)0xA5), lds((size_t)lds_bytes + 16, (char)0xA5);
        const SqLsapLayout L = sq_lsap_carve(scratch.data(), lds.data(), form, n, m);
        if (n > 0) sq_lsap_run<1>(L, form, n, m, e.data(), 0, SqLsapSyncNone(), SqCoopSingle());
        printf("%c", FORM[form]);
        for (int q = 0; q < n; q++) printf(" %d", L.col4row[q]);
        printf("\n");
    }
    return 0;
}

#define ARR(name, ptr, base, count) printf("\"%s\": [%zu, %zu, %zu], ", name, (size_t)((char *)(ptr) - (char *)(base)), sizeof(*(ptr)), (size_t)(count))

static int print_layouts()
{
    int n, m;
    while (scanf("%d %d", &n, &m) == 2) {
        const SqLsapLayout A = sq_lsap_carve(nullptr, nullptr, SQ_LSAP_A, n, m), C = sq_lsap_carve(nullptr, nullptr, SQ_LSAP_C, n, m);
        const size_t N = (size_t)n, cells = N * A.nw;
        printf("{");
        ARR("u", A.u, 0, N); ARR("v", A.v, 0, N); ARR("spc", A.spc, 0, N);
        ARR("path", A.path, 0, N); ARR("col4row", A.col4row, 0, N); ARR("row4col", A.row4col, 0, N); ARR("remaining", A.remaining, 0, N);
        ARR("SR", A.SR, 0, N); ARR("SC", A.SC, 0, N);
        ARR("wts", A.wts, 0, m); ARR("mask", A.mask, 0, cells); ARR("rowstart", A.rowstart, 0, N + 1); ARR("pre", A.pre, 0, cells);
        ARR("cids", A.cids, 0, 2 * (size_t)m);
        ARR("c_cost", C.cost, 0, N * N); ARR("c_u", C.u, 0, N); ARR("c_SC", C.SC, 0, N);
        printf("\"vec_bytes\": %zu, \"sparse_bytes\": %zu, \"lds_bytes\": %zu, \"scratch_bytes\": %zu}\n", sq_lsap_vec_bytes(n),
               sq_lsap_sparse_bytes(n, m), sq_lsap_lds_bytes(n, m), sq_lsap_scratch_bytes(n));
    }
    return 0;
}

static int print_launches()
{
    int nj;
    while (scanf("%d", &nj) == 1) {
        std::vector<SqMatchJob> jobs(nj);
        for (int q = 0; q < nj; q++) {
            jobs[q] = SqMatchJob();
            if (scanf("%d %d", &jobs[q].n, &jobs[q].nedges) != 2) return 1;
        }
        const SqLsapLds P = sq_lsap_launch_lds(jobs.data(), nj);
        printf("%zu %zu", P.need, P.lds);
        for (int q = 0; q < nj; q++) printf(" %c", FORM[sq_lsap_form(jobs[q].n, jobs[q].nedges, P.lds)]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "layout")) return print_layouts();
    if (argc > 1 && !strcmp(argv[1], "launch")) return print_launches();
    return run_cases();
}
