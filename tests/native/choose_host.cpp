// Test-only host harness: runs the product's ChooseStems (squarna_amd/csrc/sq_choose.h) on the CPU, one lane, so tests can
// compare it with the oracle's _choose_stems without a GPU.
//   argv[1]  "32" (default) or "16": the index type of the choice's arrays (the choose kernel's, the round kernel's)
//   stdin:   T, then per case "range cap cmax n" and n lines "key len bps fin" (any order; fin may be -inf).
//   stdout:  per case two lines: "pick <key>" -- the stopper's pick at the best finalscore of the list -- or "pick none"; then
//            "ovf range", "ovf picks", or "<taken> <in range>" followed by "key len bps fin" of every stem handed out, in order.
// The choice's arrays hold exactly what the call is told they hold and start out as 0xA5 bytes: nothing may rely on zeroed
// memory, and a sanitizer build sees every access beyond them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../squarna_amd/csrc/sq_choose.h"

struct Stem { uint32_t key, len; double bps, fin; };

template <class T> static T *fresh(std::vector<char> &store, size_t count)
{
    store.assign(count * sizeof(T), (char)0xA5);
    return reinterpret_cast<T *>(store.data());
}

template <class Idx> static int run_cases()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        double range; int cap, cmax, n;
        if (scanf("%lf %d %d %d", &range, &cap, &cmax, &n) != 4) return 1;
        std::vector<Stem> stems(n);
        for (Stem &s : stems) if (scanf("%u %u %lf %lf", &s.key, &s.len, &s.bps, &s.fin) != 4) return 1;
        const SqChooseRecs<Stem> src{stems.data(), (uint32_t)n};
        double best = stems.empty() ? 0.0 : stems[0].fin;
        for (const Stem &s : stems) if (s.fin > best) best = s.fin;
        const uint32_t pick = sq_choose_first(src, best, 0, 1, SqCoopSingle());
        if (pick == SQ_CHOOSE_NONE) printf("pick none\n"); else printf("pick %u\n", stems[pick].key);
        std::vector<char> b_fin, b_key, b_idx, b_ord, b_ri, b_rj, b_rl;
        double *fin = fresh<double>(b_fin, cap); uint32_t *key = fresh<uint32_t>(b_key, cap);
        Idx *idx = fresh<Idx>(b_idx, cap); uint16_t *ord = fresh<uint16_t>(b_ord, cap);
        int *ri = fresh<int>(b_ri, SQ_POOL_CMAX), *rj = fresh<int>(b_rj, SQ_POOL_CMAX), *rl = fresh<int>(b_rl, SQ_POOL_CMAX);
        std::vector<Stem> out;
        const SqChoice ch = sq_choose_stems(src, range, cap, cmax, fin, key, idx, ord, ri, rj, rl, 0, 1, [] {}, SqCoopSingle(),
                                            [&](int k, uint32_t kk, int len, double bps, double f) {
                                                if (k != (int)out.size()) exit(3);          // handed out in order, once each
                                                out.push_back(Stem{kk, (uint32_t)len, bps, f});
                                            });
        if (ch.taken == SQ_CHOOSE_OVF_RANGE) printf("ovf range\n");
        else if (ch.taken == SQ_CHOOSE_OVF_PICKS) printf("ovf picks\n");
        else {
            if (ch.taken != (int)out.size()) return 3;
            printf("%d %d", ch.taken, ch.in_range);
            for (const Stem &s : out) printf(" %u %u %.17g %.17g", s.key, s.len, s.bps, s.fin);
            printf("\n");
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "16")) return run_cases<uint16_t>();
    return run_cases<uint32_t>();
}
