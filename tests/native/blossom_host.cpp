// Test-only host harness: runs the product's blossom restatement (squarna_amd/csrc/sq_blossom.h)
// on the CPU so tests can compare it with networkx.max_weight_matching on many graphs quickly.
// optional argument: 0, 1 or 2, the capacities of the run (SqBlossom::init's `tight`; the kernel's forms 1 and 2 run with 1 and 2).
// stdin: T, then per graph: n m, then m lines "v w weight" (vertex ids in graph order).
// stdout: per graph one line with mate[0..n-1], then the rank of every vertex's first mate assignment (mord[0..n-1]).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../squarna_amd/csrc/sq_blossom.h"

int main(int argc, char **argv)
{
    // optional argument: the capacities of the run (SqBlossom::init's `tight`: 0 generous, 1 tight, 2 tight with the short queue)
    const int tight = argc > 1 ? atoi(argv[1]) : 0;
    if (tight < 0 || tight > 2) return 2;
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        int n, m;
        if (scanf("%d %d", &n, &m) != 2) return 1;
        std::vector<SqMatchEdge> e(m);
        for (int k = 0; k < m; k++) {
            if (scanf("%d %d %lf", &e[k].v, &e[k].w, &e[k].weight) != 3) return 1;
        }
        std::vector<char> scratch(SqBlossom::scratch_bytes(n, m) + 64);        // (tight = 0: the largest layout)
        SqBlossom bl;
        bl.init(n, m, e.data(), scratch.data(), tight);
        bl.run();
        if (bl.error) { printf("ERROR %d\n", bl.error); continue; }
        for (int v = 0; v < n; v++) printf("%d ", bl.mate[v]);
        for (int v = 0; v < n; v++) printf("%d ", bl.mord[v]);
        printf("\n");
    }
    return 0;
}
