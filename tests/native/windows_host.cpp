// Test-only host harness: runs the product's window pair count (squarna_amd/csrc/sq_windows.h, the logic of
// sq_window_pair_count) on the CPU as one thread, so tests can compare it with a dict count without a GPU.
// stdin: T, then per case: Ltot rec0 nwin cap ncell, then rec0 + nwin + 1 cell offsets, ncell partner entries, nwin starts,
// nwin lengths.
// stdout: per case one line: status n, then for each of the first min(n, cap) records: flat count cover first.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../squarna_amd/csrc/sq_windows.h"

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        long long Ltot, cap, ncell;
        int rec0, nwin;
        if (scanf("%lld %d %d %lld %lld", &Ltot, &rec0, &nwin, &cap, &ncell) != 5) return 1;
        std::vector<int64_t> cell_off((size_t)(rec0 + nwin + 1)), start((size_t)nwin);
        std::vector<int32_t> partner((size_t)ncell), len((size_t)nwin);
        long long x;
        for (auto &c : cell_off) { if (scanf("%lld", &x) != 1) return 1; c = x; }
        for (long long k = 0; k < ncell; k++) { if (scanf("%lld", &x) != 1) return 1; partner[(size_t)k] = (int32_t)x; }
        for (int k = 0; k < nwin; k++) { if (scanf("%lld", &x) != 1) return 1; start[(size_t)k] = x; }
        for (int k = 0; k < nwin; k++) { if (scanf("%lld", &x) != 1) return 1; len[(size_t)k] = (int32_t)x; }
        SqWindows w;
        w.partner = partner.data(); w.cell_off = cell_off.data(); w.start = start.data(); w.len = len.data();
        w.rec0 = rec0; w.nwin = nwin; w.Ltot = Ltot;
        std::vector<long long> out;
        long long n = 0;
        int status = 0;
        for (int k = 0; k < nwin; k++)
            for (int32_t t = 0; t < len[(size_t)k]; t++) {
                int64_t flat = 0;
                int32_t count = 0, cover = 0, first = 0;
                const int what = w.entry(k, t, flat, count, cover, first);
                if (what == SQ_W_INVALID) status = 2;
                if (what != SQ_W_EMIT) continue;
                if (n < cap) { out.push_back(flat); out.push_back(count); out.push_back(cover); out.push_back(first); }
                n++;
            }
        printf("%d %lld", status, n);
        for (long long v : out) printf(" %lld", v);
        printf("\n");
    }
    return 0;
}
