// Test-only host harness: runs the product's first fit in rounds (squarna_amd/csrc/sq_firstfit.h) on the CPU as one thread,
// so tests can compare it with the sequential pass (sq_align_first_fit) without a GPU.
// stdin: T, then per case: L minspan n, then n flat indices v * L + w in rank order.
// stdout: per case one line: status rounds pairs live, then partner[0..L-1].
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../squarna_amd/csrc/sq_firstfit.h"

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        int L, minspan;
        long long n;
        if (scanf("%d %d %lld", &L, &minspan, &n) != 3) return 1;
        std::vector<int64_t> flat((size_t)n + 1);
        for (long long k = 0; k < n; k++) {
            long long f;
            if (scanf("%lld", &f) != 1) return 1;
            flat[(size_t)k] = f;
        }
        std::vector<int32_t> partner((size_t)L, 12345), scratch(SqFirstFit::scratch_ints(n, L), 777);   // (nothing may rely on zeroed memory)
        SqFirstFit f;
        f.flat = flat.data(); f.n = n; f.L = L; f.minspan = minspan; f.partner = partner.data();
        f.bind(scratch.data());
        SqFitSerial x;
        f.run(x);
        printf("%d %d %d %d", f.ctl[4 + SQ_FF_STATUS], f.ctl[4 + SQ_FF_ROUNDS], f.ctl[4 + SQ_FF_PAIRS], f.ctl[4 + SQ_FF_LIVE]);
        for (int c = 0; c < L; c++) printf(" %d", partner[(size_t)c]);
        printf("\n");
    }
    return 0;
}
