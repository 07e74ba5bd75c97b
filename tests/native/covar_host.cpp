// Test-only host harness: runs the product's covariation logic (squarna_amd/csrc/sq_covar.h, the logic of sq_covariation_scan)
// on the CPU as one thread, so tests can compare it with plain counts without a GPU: the planes from the rows, then every cell
// of every upper-triangle tile in the order of tile_of(), word chunk by word chunk as the kernel walks them.
// stdin: T, then per case: R L minspan min_rows min_cov and R rows of L characters (none of them white space).
// stdout: first one line "TILE WORD_CHUNK MAX_BLOCKS"; then per case one line: the number of emitted cells, then per cell
// flat c0 c1 c2 c3 c4 c5 both_gap cov.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../squarna_amd/csrc/sq_covar.h"

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    printf("%d %d %d\n", SQ_COV_TILE, SQ_COV_WORD_CHUNK, SQ_COV_MAX_BLOCKS);
    std::vector<char> buf;
    while (T--) {
        int R, L, minspan, min_rows;
        long long min_cov;
        if (scanf("%d %d %d %d %lld", &R, &L, &minspan, &min_rows, &min_cov) != 5 || R < 1 || L < 1) return 1;
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
        const int64_t nT = ((int64_t)L + SQ_COV_TILE - 1) / SQ_COV_TILE, ntiles = SqCovar::tile_count(nT);
        std::vector<long long> out;
        long long emitted = 0;
        int64_t seen_row = 0, seen_col = -1;                            // tile_of() walks the triangle row after row
        for (int64_t k = 0; k < ntiles; k++) {
            int32_t ti, tj;
            SqCovar::tile_of(k, nT, ti, tj);
            if (seen_col + 1 < nT) seen_col++; else { seen_row++; seen_col = seen_row; }
            if (ti != seen_row || tj != seen_col) { fprintf(stderr, "tile_of(%lld) = (%d, %d)\n", (long long)k, ti, tj); return 2; }
            for (int vl = 0; vl < SQ_COV_TILE; vl++)
                for (int wl = 0; wl < SQ_COV_TILE; wl++) {
                    const int64_t v = (int64_t)ti * SQ_COV_TILE + vl, w = (int64_t)tj * SQ_COV_TILE + wl;   // (< Lpad)
                    int32_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};
                    for (int64_t wb = 0; wb < W; wb += SQ_COV_WORD_CHUNK)
                        for (int wd = 0; wd < SQ_COV_WORD_CHUNK; wd++) {
                            uint64_t a[SQ_COV_PLANES], b[SQ_COV_PLANES];
                            for (int p = 0; p < SQ_COV_PLANES; p++) {
                                a[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, v, W, Lpad)] : 0ull;
                                b[p] = wb + wd < W ? plane[(size_t)SqCovar::at(p, wb + wd, w, W, Lpad)] : 0ull;
                            }
                            SqCovar::accumulate(a, b, cnt);
                        }
                    const int64_t cov = SqCovar::finish(cnt);
                    if (!SqCovar::in_scope(v, w, L, minspan) || !SqCovar::emits(cnt, cov, min_rows, min_cov)) continue;
                    emitted++;
                    out.push_back((long long)(v * L + w));
                    for (int j = 0; j < 7; j++) out.push_back(cnt[j]);
                    out.push_back((long long)cov);
                }
        }
        printf("%lld", emitted);
        for (long long q : out) printf(" %lld", q);
        printf("\n");
    }
    return 0;
}
