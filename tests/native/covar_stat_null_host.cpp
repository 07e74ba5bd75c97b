// Test-only host harness: runs the shared logic of the statistics' shuffled-column null (squarna_amd/csrc/sq_covar_stat_null.h,
// the bin search on doubles and the ordered integer key of sq_covariation_stat_null) on the CPU as one thread, so tests can
// compare it with bisect and max in Python without a GPU.  Doubles travel as their 64 bits in decimal.
// stdin: T, then T commands:
//   bins  U t[0..U-1] Q c[0..Q-1]   -> bin() of every c against the sorted distinct thresholds
//   keys  Q c[0..Q-1]               -> key() of every c
//   max   Q c[0..Q-1]               -> the bits of unkey(the largest key, from key 0 on): the largest c, -infinity when Q == 0
//   back  Q c[0..Q-1]               -> the bits of unkey(key(c)) of every c
//   words R L batch                 -> scratch_words
// stdout: first one line "LDS_BINS", then one line per command.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../squarna_amd/csrc/sq_covar_stat_null.h"

static double as_double(unsigned long long u)
{
    double x;
    memcpy(&x, &u, sizeof x);
    return x;
}

static bool read_doubles(std::vector<double> &out)
{
    long long n;
    unsigned long long u;
    if (scanf("%lld", &n) != 1 || n < 0) return false;
    out.resize((size_t)n);
    for (auto &x : out) {
        if (scanf("%llu", &u) != 1) return false;
        x = as_double(u);
    }
    return true;
}

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    printf("%d\n", SQ_COVSTATNULL_LDS_BINS);
    while (T--) {
        char cmd[16];
        std::vector<double> thr, val;
        if (scanf("%15s", cmd) != 1) return 1;
        if (!strcmp(cmd, "bins")) {
            if (!read_doubles(thr) || !read_doubles(val)) return 1;
            for (double c : val) printf("%lld ", (long long)SqCovarStatNull::bin(thr.data(), (int64_t)thr.size(), c));
        } else if (!strcmp(cmd, "keys")) {
            if (!read_doubles(val)) return 1;
            for (double c : val) printf("%llu ", (unsigned long long)SqCovarStatNull::key(c));
        } else if (!strcmp(cmd, "max")) {
            if (!read_doubles(val)) return 1;
            uint64_t most = 0;
            for (double c : val) most = SqCovarStatNull::key(c) > most ? SqCovarStatNull::key(c) : most;
            printf("%llu", (unsigned long long)SqCovarStatNull::bits(SqCovarStatNull::unkey(most)));
        } else if (!strcmp(cmd, "back")) {
            if (!read_doubles(val)) return 1;
            for (double c : val) printf("%llu ", (unsigned long long)SqCovarStatNull::bits(SqCovarStatNull::unkey(SqCovarStatNull::key(c))));
        } else if (!strcmp(cmd, "words")) {
            int R, L, batch;
            if (scanf("%d %d %d", &R, &L, &batch) != 3) return 1;
            printf("%lld", (long long)SqCovarStatNull::scratch_words(R, L, batch));
        } else
            return 1;
        printf("\n");
    }
    return 0;
}
