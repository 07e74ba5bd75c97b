// Test-only host harness: runs the product's Nussinov restatement (squarna_amd/csrc/sq_nussinov.h) on the CPU, one thread, so
// tests can compare it with the oracle's Nussinov without a GPU.
// stdin: T, then per case "n m", n letter codes (squarna_amd.dbn.encode_seq) and m lines "v w score" (distinct cells, v < w).
// stdout: per case one line: the bytes the column lists take and the bytes of the region they live in, the number of pairs,
// then the pairs "k j" in the order BackTrack emits them.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../squarna_amd/csrc/sq_blossom.h"

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        int n, m;
        if (scanf("%d %d", &n, &m) != 2) return 1;
        std::vector<uint8_t> codes(n + 1);
        for (int q = 0; q < n; q++) {
            int c;
            if (scanf("%d", &c) != 1) return 1;
            codes[q] = (uint8_t)c;
        }
        std::vector<SqMatchEdge> e(m);
        for (int k = 0; k < m; k++)
            if (scanf("%d %d %lf", &e[k].v, &e[k].w, &e[k].weight) != 3) return 1;
        // 0xA5: the algorithm may rely on no zeroed scratch
        std::vector<char> scratch(sq_nussinov_scratch_bytes(n), (char)0xA5);
        std::vector<int32_t> out(2 * ((size_t)n + 4));
        const SqNussLayout L = sq_nuss_carve(scratch.data(), n, m);
        int32_t count = 0;
        if (n >= 2) sq_nussinov_run(L, n, m, e.data(), codes.data(), out.data(), &count, 0, 1, [] {}, SqCoopSingle());   // (n < 2: as the kernel)
        printf("%zu %zu %d", L.lists_end, L.lists_room, count);
        for (int k = 0; k < 2 * count; k++) printf(" %d", out[k]);
        printf("\n");
    }
    return 0;
}
