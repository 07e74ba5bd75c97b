// Test-only host harness: runs the product's variant comparison (squarna_amd/csrc/sq_variants.h, the logic of sq_variant_diff)
// on the CPU as one thread, so tests can compare it with set differences without a GPU.
// stdin: T, then per case: Ltot rec0 nvar ncell, then rec0 + nvar + 1 cell offsets, rec0 + nvar lengths, ncell partner entries,
// nvar wild-type records, rec0 + 1 position offsets.
// stdout: per case one line: status, then per variant: valid lost gained kept changed first last, then Ltot counts per position.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../squarna_amd/csrc/sq_variants.h"

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        long long Ltot, ncell, x;
        int rec0, nvar;
        if (scanf("%lld %d %d %lld", &Ltot, &rec0, &nvar, &ncell) != 4) return 1;
        std::vector<int64_t> cell_off((size_t)(rec0 + nvar + 1)), lengths((size_t)(rec0 + nvar)), pos_off((size_t)(rec0 + 1));
        std::vector<int32_t> partner((size_t)ncell), wt_rec((size_t)nvar);
        for (auto &c : cell_off) { if (scanf("%lld", &x) != 1) return 1; c = x; }
        for (auto &c : lengths) { if (scanf("%lld", &x) != 1) return 1; c = x; }
        for (auto &c : partner) { if (scanf("%lld", &x) != 1) return 1; c = (int32_t)x; }
        for (auto &c : wt_rec) { if (scanf("%lld", &x) != 1) return 1; c = (int32_t)x; }
        for (auto &c : pos_off) { if (scanf("%lld", &x) != 1) return 1; c = x; }
        SqVariants s;
        s.partner = partner.data(); s.cell_off = cell_off.data(); s.lengths = lengths.data(); s.wt_rec = wt_rec.data();
        s.pos_off = pos_off.data(); s.rec0 = rec0; s.nvar = nvar; s.Ltot = Ltot;
        std::vector<int32_t> pos_changed((size_t)Ltot, 0);
        std::vector<long long> out;
        int status = 0;
        for (int32_t m = 0; m < nvar; m++) {
            const int32_t n = s.length(m);
            long long lost = 0, gained = 0, kept = 0, changed = 0, first = -1, last = -1;
            bool valid = n >= 0;
            if (valid) {
                const int64_t wt = wt_rec[(size_t)m];
                const int32_t *w = s.row(wt), *v = s.row((int64_t)rec0 + m);
                for (int32_t t = 0; t < n; t++) {
                    const int f = SqVariants::entry(w, v, n, t);
                    if (f & SQ_V_INVALID) { valid = false; continue; }
                    lost += !!(f & SQ_V_LOST); gained += !!(f & SQ_V_GAINED); kept += !!(f & SQ_V_KEPT);
                    if (f & SQ_V_CHANGED) {
                        changed++;
                        if (first < 0) first = t;
                        last = t;
                        pos_changed[(size_t)(pos_off[(size_t)wt] + t)]++;
                    }
                }
            }
            if (!valid) status = 2;
            for (long long q : {(long long)valid, lost, gained, kept, changed, first, last}) out.push_back(q);
        }
        printf("%d", status);
        for (long long q : out) printf(" %lld", q);
        for (int32_t c : pos_changed) printf(" %d", c);
        printf("\n");
    }
    return 0;
}
