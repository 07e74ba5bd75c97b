// Test-only host harness: runs the product's covariation-statistics logic (squarna_amd/csrc/sq_covar_stat.h, the logic of
// sq_covariation_stat_scan) on the CPU as one thread, so tests can compare it with plain counts without a GPU: the planes from
// the rows; pass 1 tile by tile in the order of tile_of(), the tile's S reduced along both axes into the partial column sums,
// the partials reduced in ascending tile order and the means in 256 strided runs, as the kernels walk them; then pass 2.
// stdin: T, then per case: R L statistic correction minspan min_rows min_stat (a double, "-inf" for none) and R rows of L
// characters (none of them white space).
// stdout: first one line "TILE WORD_CHUNK MAX_BLOCKS"; then per case two lines: the L + 1 means (zeros without a correction),
// and the number of emitted cells, then per cell flat n[0..15] S C.  Doubles are printed as hexadecimal floats: every bit.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../squarna_amd/csrc/sq_covar_stat.h"

int main()
{
    int cases;
    if (scanf("%d", &cases) != 1) return 1;
    printf("%d %d %d\n", SQ_COVSTAT_TILE, SQ_COVSTAT_WORD_CHUNK, SQ_COVSTAT_MAX_BLOCKS);
    constexpr int T = SQ_COVSTAT_TILE;
    std::vector<char> buf;
    while (cases--) {
        int R, L, stat, corr, minspan, min_rows;
        double min_stat;
        if (scanf("%d %d %d %d %d %d %lf", &R, &L, &stat, &corr, &minspan, &min_rows, &min_stat) != 7 || R < 1 || L < 1) return 1;
        if (stat < 0 || stat >= SQ_COVSTAT_STATS || corr < 0 || corr >= SQ_COVSTAT_CORRECTIONS) return 1;
        const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L);
        std::vector<uint64_t> plane((size_t)SqCovar::plane_words(R, L), 0);
        buf.assign((size_t)L + 2, 0);
        const std::string fmt = "%" + std::to_string(L + 1) + "s";
        for (int r = 0; r < R; r++) {
            if (scanf(fmt.c_str(), buf.data()) != 1 || (int)std::string(buf.data()).size() != L) return 1;
            for (int c = 0; c < L; c++) {
                const int p = SqCovar::cls((uint8_t)buf[(size_t)c]);
                if (p < SQ_COV_PLANES) plane[(size_t)SqCovar::at(p, r / 64, c, W, Lpad)] |= 1ull << (r % 64);
            }
        }
        // the 16 counters of cell (v, w), word chunk by word chunk with the words beyond W as zero
        auto counters = [&](int64_t v, int64_t w, int32_t n[16]) {
            for (int k = 0; k < 16; k++) n[k] = 0;
            for (int64_t wb = 0; wb < W; wb += SQ_COVSTAT_WORD_CHUNK)
                for (int wd = 0; wd < SQ_COVSTAT_WORD_CHUNK; wd++) {
                    uint64_t a[4], b[4];
                    for (int p = 0; p < 4; p++) {
                        a[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, v, W, Lpad)] : 0ull;
                        b[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, w, W, Lpad)] : 0ull;
                    }
                    SqCovarStat::accumulate(a, b, n);
                }
        };
        const int64_t nT = SqCovarStat::tiles(L), ntiles = SqCovar::tile_count(nT);
        if ((int64_t)nT * T > Lpad) return 2;
        std::vector<double> mean((size_t)L + 1, 0.0);
        if (corr != SQ_COVSTAT_NONE) {
            const double never = -1.0;                                   // every slot of a column < nT * T is written exactly once
            std::vector<double> partial((size_t)SqCovarStat::partial_words(L), never);
            std::vector<int> writes(partial.size(), 0);
            for (int64_t k = 0; k < ntiles; k++) {
                int32_t ti, tj;
                SqCovar::tile_of(k, nT, ti, tj);
                const int64_t v0 = (int64_t)ti * T, w0 = (int64_t)tj * T;
                double S[T][T], row[T], col[T];
                for (int vl = 0; vl < T; vl++)
                    for (int wl = 0; wl < T; wl++) {
                        const int64_t v = v0 + vl, w = w0 + wl;
                        int32_t n[16];
                        counters(v, w, n);
                        S[vl][wl] = v < w && w < L ? SqCovarStat::raw(stat, n) : 0.0;
                    }
                for (int t = 0; t < T; t++) {
                    row[t] = col[t] = 0.0;
                    for (int j = 0; j < T; j++) row[t] += S[t][j];
                    for (int j = 0; j < T; j++) col[t] += S[j][t];
                }
                for (int t = 0; t < T; t++) {
                    if (ti == tj) { partial[(size_t)(ti * Lpad + v0 + t)] = row[t] + col[t]; writes[(size_t)(ti * Lpad + v0 + t)]++; }
                    else {
                        partial[(size_t)(tj * Lpad + v0 + t)] = row[t]; writes[(size_t)(tj * Lpad + v0 + t)]++;
                        partial[(size_t)(ti * Lpad + w0 + t)] = col[t]; writes[(size_t)(ti * Lpad + w0 + t)]++;
                    }
                }
            }
            for (int64_t t = 0; t < nT; t++)
                for (int64_t c = 0; c < Lpad; c++)
                    if (writes[(size_t)(t * Lpad + c)] != (c < nT * T ? 1 : 0)) { fprintf(stderr, "slot (%lld, %lld)\n", (long long)t, (long long)c); return 2; }
            for (int64_t c = 0; c < L; c++) {
                double sum = 0.0;
                for (int64_t t = 0; t < nT; t++) sum += partial[(size_t)(t * Lpad + c)];
                mean[(size_t)c] = L > 1 ? sum / (double)(L - 1) : 0.0;
            }
            double run[256], all = 0.0;
            for (int t = 0; t < 256; t++) {
                run[t] = 0.0;
                for (int64_t c = t; c < L; c += 256) run[t] += mean[(size_t)c];
            }
            for (int t = 0; t < 256; t++) all += run[t];
            mean[(size_t)L] = all / (double)L;
        }
        for (int64_t c = 0; c <= L; c++) printf("%s%a", c ? " " : "", mean[(size_t)c]);
        printf("\n");
        long long emitted = 0;
        std::string out;
        char text[64];
        for (int64_t k = 0; k < ntiles; k++) {
            int32_t ti, tj;
            SqCovar::tile_of(k, nT, ti, tj);
            for (int vl = 0; vl < T; vl++)
                for (int wl = 0; wl < T; wl++) {
                    const int64_t v = (int64_t)ti * T + vl, w = (int64_t)tj * T + wl;   // (< Lpad)
                    int32_t n[16];
                    counters(v, w, n);
                    if (!SqCovar::in_scope(v, w, L, minspan)) continue;
                    const double S = SqCovarStat::raw(stat, n);
                    const double C = SqCovarStat::corrected(corr, S, mean[(size_t)v], mean[(size_t)w], mean[(size_t)L]);
                    if (!SqCovarStat::emits(SqCovarStat::rows(n), C, min_rows, min_stat)) continue;
                    emitted++;
                    out += " " + std::to_string((long long)(v * L + w));
                    for (int j = 0; j < 16; j++) out += " " + std::to_string(n[j]);
                    snprintf(text, sizeof text, " %a %a", S, C);
                    out += text;
                }
        }
        printf("%lld%s\n", emitted, out.c_str());
    }
    return 0;
}
