// Test-only host harness: runs the product's logic of the weighted statistics' shuffled-column null
// (squarna_amd/csrc/sq_covar_wstat_null.h and what it joins: the shuffle of sq_covar_null.h, accumulate() and raw_w() of
// sq_covar_wstat.h, bin() and key() of sq_covar_stat_null.h) on the CPU as one thread, so tests can compare it with a
// plain-Python restatement without a GPU.  Sample k of the null is formed as the device forms it -- per column the sorted keys,
// row j of the shuffled column takes the class of its source row, row j keeps q[j] --, its planes are walked chunk by chunk of
// words with the chunk's weights as tile_bins() walks them, and S of every in-scope cell is binned against the thresholds and
// folded into the sample's maximum through its key.
// stdin: T, then T commands:
//   words R L batch    -> the scratch offsets planes partial mean cls q words
//   null  R L statistic minspan K seed U t[0..U-1] (the bits of sorted distinct doubles, in decimal), R weights, R rows of L
//                         characters (none of them white space)
//                      -> the status (0, or 3 for a bad weight), then per sample: the in-scope cells, then per cell "v w Q[0..15]
//                         S" (S as a hexadecimal float), then the U + 1 counts of the sample's histogram and the bits of its
//                         maximum (-infinity without a cell)
// stdout: first one line "LDS_BINS TILE WORD_CHUNK MAX_ROWS", then per kind of sq_covar_wstat_lds() (sums, scan, pairs, null)
// one line "total offset size offset size ..." for planes q bins S row col flat raw em thresholds hist top (the sizes stated
// here, from the arrays' shapes); then one line per command.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../squarna_amd/csrc/sq_covar_wstat_null.h"

int main()
{
    int cases;
    if (scanf("%d", &cases) != 1) return 1;
    constexpr int T = SQ_COVSTAT_TILE, CH = SQ_COVSTAT_WORD_CHUNK, NB = SQ_COVWSTATNULL_LDS_BINS;
    printf("%d %d %d %d\n", NB, T, CH, SQ_COVNULL_MAX_ROWS);
    for (int kernel = 0; kernel < 4; kernel++) {
        const SqCovarWstatLds l = sq_covar_wstat_lds(kernel);
        const bool tiles = kernel != SQ_COVWSTAT_LDS_PAIRS, sums = kernel == SQ_COVWSTAT_LDS_SUMS, scan = kernel == SQ_COVWSTAT_LDS_SCAN;
        const bool null = kernel == SQ_COVWSTAT_LDS_NULL;
        const size_t size[12] = {tiles ? sizeof(uint64_t) * 2 * 4 * CH * T : 0, tiles ? sizeof(uint32_t) * 64 * CH : 0, sizeof(int64_t) * 16 * 256,
                                 sums ? sizeof(double) * T * (T + 1) : 0, sums ? sizeof(double) * T : 0, sums ? sizeof(double) * T : 0,
                                 scan ? sizeof(int64_t) * SQ_COVWSTAT_STAGE : 0, scan ? sizeof(double) * SQ_COVWSTAT_STAGE : 0,
                                 scan ? (size_t)SQ_COVWSTAT_EMIT_BYTES : 0, null ? sizeof(double) * NB : 0, null ? sizeof(uint32_t) * NB : 0,
                                 null ? sizeof(uint64_t) : 0};
        const uint32_t at[12] = {l.planes, l.q, l.bins, l.S, l.row, l.col, l.flat, l.raw, l.em, l.thresholds, l.hist, l.top};
        printf("%zu", l.total);
        for (int k = 0; k < 12; k++) printf(" %u %zu", at[k], size[k]);
        printf("\n");
    }
    std::vector<char> buf;
    while (cases--) {
        char cmd[16];
        if (scanf("%15s", cmd) != 1) return 1;
        if (!strcmp(cmd, "words")) {
            int R, L, batch;
            if (scanf("%d %d %d", &R, &L, &batch) != 3) return 1;
            const SqCovarWstatNullScratch s = SqCovarWstatNull::scratch(R, L, batch);
            printf("%lld %lld %lld %lld %lld %lld\n", (long long)s.planes, (long long)s.partial, (long long)s.mean, (long long)s.cls,
                   (long long)s.q, (long long)s.words);
            continue;
        }
        if (strcmp(cmd, "null")) return 1;
        int R, L, stat, minspan, K;
        unsigned long long seed;
        long long U;
        if (scanf("%d %d %d %d %d %llu %lld", &R, &L, &stat, &minspan, &K, &seed, &U) != 7) return 1;
        if (R < 1 || R > SQ_COVNULL_MAX_ROWS || L < 1 || stat < 0 || stat >= SQ_COVSTAT_STATS || minspan < 0 || K < 1 || U < 0) return 1;
        std::vector<double> thr((size_t)U);
        for (auto &t : thr) {
            unsigned long long u;
            if (scanf("%llu", &u) != 1) return 1;
            memcpy(&t, &u, sizeof t);
        }
        const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L), Rpad = SqCovarWstat::rpad(R);
        std::vector<uint32_t> q((size_t)Rpad, 0u);
        int status = 0;
        for (int r = 0; r < R; r++) {
            double w;
            if (scanf("%lf", &w) != 1) return 1;
            if (!SqCovarWstat::quantise(w, q[(size_t)r])) status = 3;
        }
        std::vector<uint8_t> cls((size_t)R * L);                         // column after column, as null_classes() leaves them
        buf.assign((size_t)L + 2, 0);
        const std::string fmt = "%" + std::to_string(L + 1) + "s";
        for (int r = 0; r < R; r++) {
            if (scanf(fmt.c_str(), buf.data()) != 1 || (int)std::string(buf.data()).size() != L) return 1;
            for (int c = 0; c < L; c++) cls[(size_t)c * R + r] = (uint8_t)SqCovar::cls((uint8_t)buf[(size_t)c]);
        }
        printf("%d", status);
        std::vector<uint64_t> key(SqCovarNull::padded(R));
        for (int k = 0; k < K; k++) {
            std::vector<uint64_t> plane((size_t)SqCovar::plane_words(R, L), 0);
            for (int c = 0; c < L; c++) {
                SqCovarNull::sort_keys(key.data(), seed, (uint64_t)k, (uint64_t)c, R, L);
                for (int j = 0; j < R; j++) {
                    const int p = cls[(size_t)c * R + SqCovarNull::source_row(key[(size_t)j])];
                    if (p < SQ_COV_PLANES) plane[(size_t)SqCovar::at(p, j / 64, c, W, Lpad)] |= 1ull << (j % 64);
                }
            }
            std::vector<long long> hist((size_t)U + 1, 0);
            uint64_t most = 0;
            long long cells = 0;
            std::string out;
            char text[64];
            for (int64_t v = 0; v < L; v++)
                for (int64_t w = v + 1; w < L; w++) {
                    if (!SqCovar::in_scope(v, w, L, minspan)) continue;
                    int64_t Q[16] = {};
                    for (int64_t wb = 0; wb < W; wb += CH) {             // the chunk's 256 weights lie inside q[rpad(R)]
                        if (wb * 64 + 64 * CH > Rpad) return 2;
                        for (int wd = 0; wd < CH; wd++) {
                            uint64_t a[4], b[4];
                            for (int p = 0; p < 4; p++) {
                                a[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, v, W, Lpad)] : 0ull;
                                b[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, w, W, Lpad)] : 0ull;
                            }
                            SqCovarWstat::accumulate(a, b, q.data() + wb * 64 + wd * 64, Q, 1);
                        }
                    }
                    const double S = SqCovarWstat::raw_w(stat, Q);
                    const uint64_t mine = SqCovarStatNull::key(S);
                    most = mine > most ? mine : most;
                    const int64_t b = SqCovarStatNull::bin(thr.data(), U, S);
                    if (b < 0 || b > U) return 2;
                    hist[(size_t)b]++;
                    cells++;
                    out += " " + std::to_string((long long)v) + " " + std::to_string((long long)w);
                    for (int j = 0; j < 16; j++) out += " " + std::to_string((long long)Q[j]);
                    snprintf(text, sizeof text, " %a", S);
                    out += text;
                }
            printf(" %lld%s", cells, out.c_str());
            for (long long h : hist) printf(" %lld", h);
            printf(" %llu", (unsigned long long)SqCovarStatNull::bits(SqCovarStatNull::unkey(most)));
        }
        printf("\n");
    }
    return 0;
}
