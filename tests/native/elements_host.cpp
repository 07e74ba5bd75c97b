// Test-only host harness: runs the product's loop annotation (squarna_amd/csrc/sq_elements.h, the logic of the kernels of
// sq_elements_dev.hip) on the CPU as one thread, so tests can compare it with a naive reference without a GPU: the exterior
// loop, then for every position the per-column test of a listed opener and that opener's loop, walked twice as the loops
// kernel walks it (the counts and the type, then the columns).  The levels come from the caller, as the loops kernel reads
// them back from what the levels kernel wrote.
// stdin: T, then per case: n (gap-free positions) and lin (input columns), then four lines of n integers each: the partner
// position (-1 none), the signed level, the separator flag and the input column of every position.
// stdout: first one line with the codes EXTERIOR STEM HAIRPIN BULGE INTERNAL MULTI PK BREAK GAP, then CODES, STACK and WAVES;
// then per case three lines: the number of loops and per loop type i j branches unpaired side5 (i, j input columns); loop_of
// per position (-1 where no loop wrote); the type per position that a loop's walk wrote (-1 elsewhere).
#include <cstdio>
#include <vector>
#include "../../squarna_amd/csrc/sq_elements.h"

struct Row {
    std::vector<int> part, lev, sp, gfcol;
    int n() const { return (int)part.size(); }
    int partner(int g) const { return part[(size_t)g]; }
    int level(int g) const { return lev[(size_t)g]; }
    bool sep(int g) const { return sp[(size_t)g] != 0; }
    int col(int g) const { return gfcol[(size_t)g]; }
};

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", SQ_ELEM_EXTERIOR, SQ_ELEM_STEM, SQ_ELEM_HAIRPIN, SQ_ELEM_BULGE, SQ_ELEM_INTERNAL,
           SQ_ELEM_MULTI, SQ_ELEM_PK, SQ_ELEM_BREAK, SQ_ELEM_GAP, SQ_ELEM_CODES, SQ_ELEM_STACK, SQ_ELEM_WAVES);
    while (T--) {
        int n, lin;
        if (scanf("%d %d", &n, &lin) != 2 || n < 0 || lin < n) return 1;
        Row R;
        for (std::vector<int> *v : {&R.part, &R.lev, &R.sp, &R.gfcol}) {
            v->resize((size_t)n);
            for (int g = 0; g < n; g++) if (scanf("%d", &(*v)[(size_t)g]) != 1) return 1;
        }
        std::vector<int> loop_of((size_t)n, -1), what((size_t)n, -1), loops;
        int nloops = 0;
        auto one = [&](int g, int w) {
            const bool ext = g < 0;
            const SqElemLoop lp = sq_elem_walk(R, g, w, [](int) {});
            const int type = sq_elem_type(ext, lp);
            if (type == SQ_ELEM_STACK) return 1;                     // (no listed opener closes a stack)
            const int k = nloops++;
            for (int x : {type, ext ? -1 : R.col(g), ext ? lin : R.col(w), lp.branches, lp.unpaired, lp.side5}) loops.push_back(x);
            sq_elem_walk(R, g, w, [&](int p) {
                if (loop_of[(size_t)p] != -1) loops[0] = -99;        // a position in two loops: reported as a broken first record
                loop_of[(size_t)p] = k;
                if (R.level(p) == 0) what[(size_t)p] = type;
            });
            return 0;
        };
        if (one(-1, n)) return 2;
        for (int g = 0; g < n; g++) if (sq_elem_listed(R, g) && one(g, R.partner(g))) return 2;
        printf("%d", nloops);
        for (int x : loops) printf(" %d", x);
        printf("\n");
        for (int g = 0; g < n; g++) printf("%d ", loop_of[(size_t)g]);
        printf("\n");
        for (int g = 0; g < n; g++) printf("%d ", what[(size_t)g]);
        printf("\n");
    }
    return 0;
}
