// Test-only host harness: runs the definition of the shuffled-column null (squarna_amd/csrc/sq_covar_null.h, the logic of
// sq_covariation_null) on the CPU as one thread, so tests can compare it with a plain-Python restatement without a GPU.
// stdin: T, then T commands:
//   keys  R L k c seed     -> the R sort keys of column c of sample k, row after row
//   order R L k c seed     -> the source row of every row of the shuffled column (the padded bitonic network, as the kernel runs it)
//   bins  U t[0..U-1] Q cov[0..Q-1]  -> bin() of every cov against the sorted distinct thresholds
//   cells L minspan        -> scope_cells
// stdout: first one line "MAX_ROWS KEY_ROWS LDS_BINS", then one line per command.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../squarna_amd/csrc/sq_covar_null.h"

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    printf("%d %d %d\n", SQ_COVNULL_MAX_ROWS, SQ_COVNULL_KEY_ROWS, SQ_COVNULL_LDS_BINS);
    while (T--) {
        char cmd[16];
        if (scanf("%15s", cmd) != 1) return 1;
        if (!strcmp(cmd, "keys") || !strcmp(cmd, "order")) {
            int R, L;
            unsigned long long k, c, seed;
            if (scanf("%d %d %llu %llu %llu", &R, &L, &k, &c, &seed) != 5 || R < 1 || R > SQ_COVNULL_KEY_ROWS || L < 1) return 1;
            if (cmd[0] == 'k') {
                for (int r = 0; r < R; r++)
                    printf("%llu ", (unsigned long long)SqCovarNull::sortkey(seed, k, c, (uint64_t)r, (uint64_t)R, (uint64_t)L));
            } else {
                std::vector<uint64_t> key(SqCovarNull::padded(R));
                SqCovarNull::sort_keys(key.data(), seed, k, c, R, L);
                for (int r = 0; r < R; r++) {
                    if (key[(size_t)r] == SqCovarNull::sentinel() || (r && key[(size_t)r - 1] >= key[(size_t)r])) return 2;
                    printf("%d ", SqCovarNull::source_row(key[(size_t)r]));
                }
                for (size_t r = (size_t)R; r < key.size(); r++)
                    if (key[r] != SqCovarNull::sentinel()) return 2;
            }
        } else if (!strcmp(cmd, "bins")) {
            long long U, Q, x;
            if (scanf("%lld", &U) != 1 || U < 0) return 1;
            std::vector<int64_t> thr((size_t)U);
            for (auto &t : thr) {
                if (scanf("%lld", &x) != 1) return 1;
                t = x;
            }
            if (scanf("%lld", &Q) != 1 || Q < 0) return 1;
            while (Q--) {
                if (scanf("%lld", &x) != 1) return 1;
                printf("%lld ", (long long)SqCovarNull::bin(thr.data(), U, x));
            }
        } else if (!strcmp(cmd, "cells")) {
            int L, minspan;
            if (scanf("%d %d", &L, &minspan) != 2) return 1;
            printf("%lld", (long long)SqCovarNull::scope_cells(L, minspan));
        } else
            return 1;
        printf("\n");
    }
    return 0;
}
