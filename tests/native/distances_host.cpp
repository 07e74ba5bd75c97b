// Test-only host harness: runs the product's structure-distance logic (squarna_amd/csrc/sq_distances.h, the logic of
// sq_structure_distances) on the CPU as one thread, so tests can compare it with plain sets of pairs without a GPU: the planes
// from the partner rows, then every cell of every planned tile, word chunk by word chunk as the kernel walks them, with the
// mirror cells of the tiles off the diagonal, then the greedy filter with the leaders, group by group.  It checks by itself
// that the plan covers every cell of two rows of one group exactly once and plans no tile without such a cell, that every
// word of the bit matrix the filter reads was written exactly once, and that every cell of the block-diagonal matrix is
// addressed at most once and inside it.
// stdin: N, then per case: S Wmax G mode threshold, the G group sizes, and per row its width and that many partners.
// stdout: first one line "TILE WORD_CHUNK MAX_BLOCKS MAX_ROWS MAX_COLS MAX_PLANES FILTER_WORDS"; then per case one line: the
// planes, T and the 2 T numbers of the plan, S numbers each of status, npairs, neighbours, keep and leader, the cells and
// that many numbers of common.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../squarna_amd/csrc/sq_distances.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 2; } while (0)

int main()
{
    int N;
    if (scanf("%d", &N) != 1) return 1;
    printf("%d %d %d %d %d %d %d\n", SQ_DIST_TILE, SQ_DIST_WORD_CHUNK, SQ_DIST_MAX_BLOCKS, SQ_DIST_MAX_ROWS, SQ_DIST_MAX_COLS, SQ_DIST_MAX_PLANES,
           SQ_DIST_FILTER_WORDS);
    while (N--) {
        int S, Wmax, G, mode, threshold;
        if (scanf("%d %d %d %d %d", &S, &Wmax, &G, &mode, &threshold) != 5 || S < 1 || Wmax < 1 || G < 1 || S > SQ_DIST_MAX_ROWS ||
            Wmax > SQ_DIST_MAX_COLS)
            return 1;
        std::vector<int32_t> group_off((size_t)G + 1, 0), row_group;
        for (int g = 0; g < G; g++) {
            int n;
            if (scanf("%d", &n) != 1 || n < 0) return 1;
            group_off[(size_t)g + 1] = group_off[(size_t)g] + n;
            row_group.insert(row_group.end(), (size_t)n, g);
        }
        if (group_off[(size_t)G] != S) return 1;
        std::vector<int64_t> mat_off((size_t)G + 1);
        const int64_t cells = SqDistances::matrix_offsets(group_off.data(), G, mat_off.data());

        // ---- the planes
        const int np = SqDistances::planes(Wmax);
        const int64_t Wc = SqDistances::col_words(Wmax), Spad = SqDistances::spad(S), Wr = SqDistances::row_words(S);
        if (np > SQ_DIST_MAX_PLANES) FAIL("%d planes", np);
        std::vector<uint64_t> plane((size_t)SqDistances::plane_words(S, Wmax), 0), nbr((size_t)SqDistances::nbr_words(S), 0);
        std::vector<int32_t> status((size_t)S, 0), npairs((size_t)S, 0), neighbours((size_t)S, 0), leader((size_t)S, -7), common((size_t)cells, -1);
        std::vector<uint8_t> valid((size_t)S, 0), keep((size_t)S, 7);
        for (int r = 0; r < S; r++) {
            int width;
            if (scanf("%d", &width) != 1 || width < 0 || width > Wmax) return 1;
            std::vector<int32_t> p((size_t)width);
            for (int c = 0; c < width; c++)
                if (scanf("%d", &p[(size_t)c]) != 1) return 1;
            bool bad = false;
            for (int c = 0; c < width && !bad; c++) {
                const int32_t q = p[(size_t)c];
                const int32_t back = q >= 0 && SqDistances::partner_in_range(q, width) ? p[(size_t)q] : c;
                bad = SqDistances::column_bad(c, q, back, width);
            }
            status[(size_t)r] = bad;
            valid[(size_t)r] = !bad;
            for (int c = 0; c < width && !bad; c++) {
                const uint32_t bits = SqDistances::plane_bits(c, p[(size_t)c]);
                if (bits >> np) FAIL("row %d column %d sets a plane beyond the %d planes", r, c, np);
                for (int k = 0; k < np; k++)
                    if (bits >> k & 1u) plane[(size_t)SqIdentity::at(k, c / 64, r, Wc, Spad)] |= 1ull << (c % 64);
                npairs[(size_t)r] += bits & 1u;
            }
        }

        // ---- the plan and what it covers
        const int64_t nT = SqDistances::tiles(S), T = SqDistances::plan_tiles(row_group.data(), S, nullptr);
        std::vector<int32_t> tiles((size_t)(2 * T));
        if (SqDistances::plan_tiles(row_group.data(), S, tiles.data()) != T) FAIL("the plan's two passes differ");
        std::vector<int> covered((size_t)S * S, 0), written((size_t)SqDistances::nbr_words(S), 0), addressed((size_t)cells, 0);
        for (int64_t k = 0; k < T; k++) {
            const int32_t ta = tiles[(size_t)(2 * k)], tb = tiles[(size_t)(2 * k + 1)];
            if (!SqDistances::tile_in_range(ta, tb, nT)) FAIL("tile %lld = (%d, %d)", (long long)k, ta, tb);
            bool useful = false;
            for (int al = 0; al < SQ_DIST_TILE; al++) {
                uint64_t word = 0;
                const int64_t a = (int64_t)ta * SQ_DIST_TILE + al;                           // (< Spad)
                const int32_t ga = a < S ? row_group[(size_t)a] : -1;
                for (int bl = 0; bl < SQ_DIST_TILE; bl++) {
                    const int64_t b = (int64_t)tb * SQ_DIST_TILE + bl;
                    const int32_t gb = b < S ? row_group[(size_t)b] : -1;
                    int32_t c = 0;
                    for (int64_t wb = 0; wb < Wc; wb += SQ_DIST_WORD_CHUNK)
                        for (int wd = 0; wd < SQ_DIST_WORD_CHUNK; wd++) {
                            uint64_t pa[SQ_DIST_MAX_PLANES], pb[SQ_DIST_MAX_PLANES];
                            for (int p = 0; p < np; p++) {
                                pa[p] = wb + wd < Wc ? plane[(size_t)SqIdentity::at(p, wb + wd, a, Wc, Spad)] : 0ull;
                                pb[p] = wb + wd < Wc ? plane[(size_t)SqIdentity::at(p, wb + wd, b, Wc, Spad)] : 0ull;
                            }
                            c += SqDistances::common_word(pa, pb, np);
                        }
                    const bool va = a < S && valid[(size_t)a], vb = b < S && valid[(size_t)b];
                    const bool near = SqDistances::neighbours(a, b, ga, gb, va, vb, mode, threshold, a < S ? npairs[(size_t)a] : 0,
                                                              b < S ? npairs[(size_t)b] : 0, c);
                    if (near) word |= SqIdentity::row_bit(bl);
                    if (near && ta != tb) nbr[(size_t)(b * Wr + ta)] |= SqIdentity::row_bit(al);   // the mirror word
                    if (a < S && b < S) {
                        covered[(size_t)(a * S + b)]++;
                        if (ta != tb) covered[(size_t)(b * S + a)]++;
                        useful |= ga == gb;
                    }
                    if (va && vb && ga == gb) {
                        const int64_t first = group_off[(size_t)ga], n_g = group_off[(size_t)ga + 1] - first;
                        const int64_t at = SqDistances::cell(mat_off[(size_t)ga], first, n_g, a, b), mirror = SqDistances::cell(mat_off[(size_t)ga], first, n_g, b, a);
                        if (at < mat_off[(size_t)ga] || at >= mat_off[(size_t)ga + 1] || mirror < mat_off[(size_t)ga] || mirror >= mat_off[(size_t)ga + 1])
                            FAIL("cell (%lld, %lld) of group %d lies outside its block", (long long)a, (long long)b, ga);
                        common[(size_t)at] = c;
                        addressed[(size_t)at]++;
                        if (ta != tb) {
                            common[(size_t)mirror] = c;
                            addressed[(size_t)mirror]++;
                        }
                    }
                }
                if (a < S) {
                    nbr[(size_t)(a * Wr + tb)] = word;
                    written[(size_t)(a * Wr + tb)]++;
                }
            }
            if (ta != tb)
                for (int bl = 0; bl < SQ_DIST_TILE; bl++)
                    if ((int64_t)tb * SQ_DIST_TILE + bl < S) written[(size_t)(((int64_t)tb * SQ_DIST_TILE + bl) * Wr + ta)]++;
            if (!useful) FAIL("tile (%d, %d) holds no cell of one group", ta, tb);
        }
        for (int64_t a = 0; a < S; a++)
            for (int64_t b = 0; b < S; b++) {
                const bool same = row_group[(size_t)a] == row_group[(size_t)b];
                if (covered[(size_t)(a * S + b)] > 1 || (same && covered[(size_t)(a * S + b)] != 1))
                    FAIL("cell (%lld, %lld) is covered %d times", (long long)a, (long long)b, covered[(size_t)(a * S + b)]);
                if (same && valid[(size_t)a] && valid[(size_t)b]) {
                    const int32_t g = row_group[(size_t)a];
                    const int64_t first = group_off[(size_t)g];
                    if (addressed[(size_t)SqDistances::cell(mat_off[(size_t)g], first, group_off[(size_t)g + 1] - first, a, b)] != 1)
                        FAIL("cell (%lld, %lld) of the matrix was not written once", (long long)a, (long long)b);
                }
            }
        for (int v : written)
            if (v > 1) FAIL("a word of the bit matrix was written %d times", v);
        for (int32_t &c : common)
            if (c < 0) c = 0;                                                                // (the cells of invalid rows: cleared, never written)

        // ---- the counts and the filter, group by group
        for (int64_t a = 0; a < S; a++) {
            neighbours[(size_t)a] = valid[(size_t)a];
            for (int64_t w = 0; w < Wr; w++) neighbours[(size_t)a] += written[(size_t)(a * Wr + w)] ? __builtin_popcountll(nbr[(size_t)(a * Wr + w)]) : 0;
        }
        for (int g = 0; g < G; g++) {
            const int64_t first = group_off[(size_t)g], last = group_off[(size_t)g + 1];
            for (int64_t a = first; a < last; a++)
                for (int64_t w = SqDistances::first_word(first); w < SqIdentity::words_below(a); w++)
                    if (written[(size_t)(a * Wr + w)] != 1) FAIL("the filter reads word %lld of row %lld, which no tile wrote", (long long)w, (long long)a);
            std::vector<uint64_t> kept((size_t)SqDistances::group_words(first, last) + 1, 0);
            SqDistances::greedy(nbr.data(), Wr, first, last, valid.data(), kept.data(), keep.data(), leader.data());
        }
        printf("%d %lld ", np, (long long)T);
        for (int v : tiles) printf("%d ", v);
        for (int v : status) printf("%d ", v);
        for (int v : npairs) printf("%d ", v);
        for (int v : neighbours) printf("%d ", v);
        for (int v : keep) printf("%d ", (int)v);
        for (int v : leader) printf("%d ", v);
        printf("%lld ", (long long)cells);
        for (int v : common) printf("%d ", v);
        printf("\n");
    }
    return 0;
}
