// Test-only host harness: runs the product's weighted covariation-statistics logic (squarna_amd/csrc/sq_covar_wstat.h, the
// logic of sq_covariation_wstat_scan / _pairs) on the CPU as one thread, so tests can compare it with plain sums without a GPU:
// the weights quantised; the planes from the rows; the counters of a cell chunk by chunk of words with the chunk's weights, as
// the tile kernels walk them, and again word by word, as the pairs kernel and the scan's flush do (both must agree); pass 1
// tile by tile in the order of tile_of(), reduced as the kernels reduce it; then pass 2.
// stdin: T, then per case: R L statistic correction minspan min_rows min_stat (doubles; "-inf" for no min_stat), R weights and
// R rows of L characters (none of them white space).
// stdout: first one line "TILE WORD_CHUNK MAX_BLOCKS ONE MAX_ROWS", then per kernel of sq_covar_wstat_lds() one line "total
// offset size offset size ..." for planes q bins S row col flat raw em (the sizes stated here, from the arrays' shapes); then per
// case three lines: the status (0, or 3 for a bad weight) and the R values of q; the L + 1 means (zeros without a
// correction); and the number of emitted cells, then per cell flat Q[0..15] S C.  Doubles are printed as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../squarna_amd/csrc/sq_covar_wstat.h"

int main()
{
    int cases;
    if (scanf("%d", &cases) != 1) return 1;
    printf("%d %d %d %d %d\n", SQ_COVSTAT_TILE, SQ_COVSTAT_WORD_CHUNK, SQ_COVSTAT_MAX_BLOCKS, SQ_COVWSTAT_ONE, SQ_COVWSTAT_MAX_ROWS);
    constexpr int T = SQ_COVSTAT_TILE, CH = SQ_COVSTAT_WORD_CHUNK;
    for (int kernel = 0; kernel < 3; kernel++) {
        const SqCovarWstatLds l = sq_covar_wstat_lds(kernel);
        const bool tiles = kernel != SQ_COVWSTAT_LDS_PAIRS, sums = kernel == SQ_COVWSTAT_LDS_SUMS, scan = kernel == SQ_COVWSTAT_LDS_SCAN;
        const size_t size[9] = {tiles ? sizeof(uint64_t) * 2 * 4 * CH * T : 0, tiles ? sizeof(uint32_t) * 64 * CH : 0, sizeof(int64_t) * 16 * 256,
                                sums ? sizeof(double) * T * (T + 1) : 0, sums ? sizeof(double) * T : 0, sums ? sizeof(double) * T : 0,
                                scan ? sizeof(int64_t) * SQ_COVWSTAT_STAGE : 0, scan ? sizeof(double) * SQ_COVWSTAT_STAGE : 0,
                                scan ? (size_t)SQ_COVWSTAT_EMIT_BYTES : 0};
        const uint32_t at[9] = {l.planes, l.q, l.bins, l.S, l.row, l.col, l.flat, l.raw, l.em};
        printf("%zu", l.total);
        for (int k = 0; k < 9; k++) printf(" %u %zu", at[k], size[k]);
        printf("\n");
    }
    std::vector<char> buf;
    while (cases--) {
        int R, L, stat, corr, minspan;
        double min_rows, min_stat;
        if (scanf("%d %d %d %d %d %lf %lf", &R, &L, &stat, &corr, &minspan, &min_rows, &min_stat) != 7 || R < 1 || L < 1) return 1;
        if (stat < 0 || stat >= SQ_COVSTAT_STATS || corr < 0 || corr >= SQ_COVSTAT_CORRECTIONS || R > SQ_COVWSTAT_MAX_ROWS) return 1;
        const int64_t W = SqCovar::words(R), Lpad = SqCovar::lpad(L), Rpad = SqCovarWstat::rpad(R);
        if (Rpad < R || Rpad % (64 * CH) || Rpad - R >= 64 * CH || SqCovarWstat::scratch_words(R, L) != SqCovarStat::scratch_words(R, L) + Rpad / 2)
            return 2;
        std::vector<uint32_t> q((size_t)Rpad, 0u);
        int status = 0;
        for (int r = 0; r < R; r++) {
            double w;
            if (scanf("%lf", &w) != 1) return 1;
            if (!SqCovarWstat::quantise(w, q[(size_t)r])) status = 3;
        }
        printf("%d", status);
        for (int r = 0; r < R; r++) printf(" %u", q[(size_t)r]);
        printf("\n");
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
        // the 16 counters of cell (v, w), word chunk by word chunk with the words beyond W as zero and the chunk's 256 weights
        auto counters = [&](int64_t v, int64_t w, int64_t Q[16]) {
            for (int k = 0; k < 16; k++) Q[k] = 0;
            for (int64_t wb = 0; wb < W; wb += CH) {
                if (wb * 64 + 64 * CH > Rpad) exit(2);
                const uint32_t *chunk = q.data() + wb * 64;
                for (int wd = 0; wd < CH; wd++) {
                    uint64_t a[4], b[4];
                    for (int p = 0; p < 4; p++) {
                        a[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, v, W, Lpad)] : 0ull;
                        b[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, w, W, Lpad)] : 0ull;
                    }
                    SqCovarWstat::accumulate(a, b, chunk + wd * 64, Q, 1);
                }
            }
        };
        // the same from "global memory", word by word, into bins a stride apart (the pairs kernel, the scan's flush)
        auto lookup = [&](int64_t v, int64_t w, int64_t Q[16]) {
            int64_t bins[16 * 3];
            for (int k = 0; k < 16 * 3; k++) bins[k] = k % 3 == 1 ? 0 : -1;
            for (int64_t wd = 0; wd < W; wd++) {
                uint64_t a[4], b[4];
                for (int p = 0; p < 4; p++) {
                    a[p] = plane[(size_t)SqCovar::at(p, wd, v, W, Lpad)];
                    b[p] = plane[(size_t)SqCovar::at(p, wd, w, W, Lpad)];
                }
                SqCovarWstat::accumulate(a, b, q.data() + wd * 64, bins + 1, 3);
            }
            for (int k = 0; k < 16 * 3; k++)
                if (k % 3 == 1) Q[k / 3] = bins[k];
                else if (bins[k] != -1) exit(2);
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
                        int64_t Q[16];
                        counters(v, w, Q);
                        S[vl][wl] = v < w && w < L ? SqCovarWstat::raw_w(stat, Q) : 0.0;
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
                    int64_t Q[16], again[16];
                    counters(v, w, Q);
                    if (!SqCovar::in_scope(v, w, L, minspan)) continue;
                    lookup(v, w, again);
                    for (int j = 0; j < 16; j++)
                        if (Q[j] != again[j]) return 2;
                    const double S = SqCovarWstat::raw_w(stat, Q);
                    const double C = SqCovarStat::corrected(corr, S, mean[(size_t)v], mean[(size_t)w], mean[(size_t)L]);
                    if (!SqCovarWstat::emits_w(SqCovarWstat::rows(SqCovarWstat::total(Q)), C, min_rows, min_stat)) continue;
                    emitted++;
                    out += " " + std::to_string((long long)(v * L + w));
                    for (int j = 0; j < 16; j++) out += " " + std::to_string((long long)Q[j]);
                    snprintf(text, sizeof text, " %a %a", S, C);
                    out += text;
                }
        }
        printf("%lld%s\n", emitted, out.c_str());
    }
    return 0;
}
