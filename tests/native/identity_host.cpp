// Test-only host harness: runs the product's row-identity logic (squarna_amd/csrc/sq_identity.h, the logic of sq_row_identity)
// on the CPU as one thread, so tests can compare it with plain string counts without a GPU: the planes from the rows, then
// every cell of every upper-triangle tile in the order of tile_of(), word chunk by word chunk as the kernel walks them, with
// the mirror cells of the tiles off the diagonal, then the greedy filter over the neighbour bit matrix.
// stdin: N, then per case: R L denominator threshold_bp and R rows of L characters (none of them white space).
// stdout: first one line "TILE WORD_CHUNK MAX_BLOCKS MAX_ROWS MAX_COLS FILTER_WORDS"; then per case one line: R numbers each of len,
// bases, neighbours and keep, then R * R numbers each of same and both.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../squarna_amd/csrc/sq_identity.h"

int main()
{
    int N;
    if (scanf("%d", &N) != 1) return 1;
    printf("%d %d %d %d %d %d\n", SQ_ID_TILE, SQ_ID_WORD_CHUNK, SQ_ID_MAX_BLOCKS, SQ_ID_MAX_ROWS, SQ_ID_MAX_COLS, SQ_ID_FILTER_WORDS);
    std::vector<char> buf;
    while (N--) {
        int R, L, kind, T;
        if (scanf("%d %d %d %d", &R, &L, &kind, &T) != 4 || R < 1 || L < 1 || R > SQ_ID_MAX_ROWS || L > SQ_ID_MAX_COLS) return 1;
        const int64_t Wc = SqIdentity::col_words(L), Rpad = SqIdentity::rpad(R), Wr = SqIdentity::row_words(R);
        std::vector<uint64_t> plane((size_t)SqIdentity::plane_words(R, L), 0), nbr((size_t)SqIdentity::nbr_words(R), 0), kept((size_t)Wr, 0);
        std::vector<int32_t> len((size_t)R, 0), bases((size_t)R, 0), neighbours((size_t)R, 0), same((size_t)R * R, -1), both((size_t)R * R, -1);
        buf.assign((size_t)L + 2, 0);
        const std::string fmt = "%" + std::to_string(L + 1) + "s";
        for (int r = 0; r < R; r++) {
            if (scanf(fmt.c_str(), buf.data()) != 1 || (int)std::string(buf.data()).size() != L) return 1;
            for (int c = 0; c < L; c++) {
                const uint32_t bits = SqIdentity::plane_bits(SqCovar::cls((uint8_t)buf[(size_t)c]));
                for (int p = 0; p < SQ_ID_PLANES; p++)
                    if (bits >> p & 1u) plane[(size_t)SqIdentity::at(p, c / 64, r, Wc, Rpad)] |= 1ull << (c % 64);
                len[(size_t)r] += bits >> SQ_ID_RES & 1u;
                bases[(size_t)r] += bits >> SQ_ID_BASE & 1u;
            }
        }
        const int64_t nT = SqIdentity::tiles(R), ntiles = SqIdentity::tile_count(nT);
        std::vector<int> written((size_t)SqIdentity::nbr_words(R), 0);    // every word of the bit matrix: by exactly one tile
        for (int64_t k = 0; k < ntiles; k++) {
            int32_t ta, tb;
            SqIdentity::tile_of(k, nT, ta, tb);
            if (ta > tb || tb >= nT) { fprintf(stderr, "tile_of(%lld) = (%d, %d)\n", (long long)k, ta, tb); return 2; }
            for (int al = 0; al < SQ_ID_TILE; al++) {
                uint64_t word = 0;
                const int64_t a = (int64_t)ta * SQ_ID_TILE + al;                            // (< Rpad)
                for (int bl = 0; bl < SQ_ID_TILE; bl++) {
                    const int64_t b = (int64_t)tb * SQ_ID_TILE + bl;
                    int32_t s = 0, bo = 0;
                    for (int64_t wb = 0; wb < Wc; wb += SQ_ID_WORD_CHUNK)
                        for (int wd = 0; wd < SQ_ID_WORD_CHUNK; wd++) {
                            uint64_t pa[SQ_ID_PLANES], pb[SQ_ID_PLANES];
                            for (int p = 0; p < SQ_ID_PLANES; p++) {
                                pa[p] = wb + wd < Wc ? plane[(size_t)SqIdentity::at(p, wb + wd, a, Wc, Rpad)] : 0ull;
                                pb[p] = wb + wd < Wc ? plane[(size_t)SqIdentity::at(p, wb + wd, b, Wc, Rpad)] : 0ull;
                            }
                            SqIdentity::accumulate(pa, pb, s, bo);
                        }
                    const bool near = SqIdentity::neighbours(a, b, R, s, bo, a < R ? len[(size_t)a] : 0, b < R ? len[(size_t)b] : 0, L, kind, T);
                    if (near) word |= SqIdentity::row_bit(bl);
                    if (near && ta != tb) nbr[(size_t)(b * Wr + ta)] |= SqIdentity::row_bit(al);   // the mirror word
                    if (a < R && b < R) {
                        same[(size_t)(a * R + b)] = s;
                        both[(size_t)(a * R + b)] = bo;
                        if (ta != tb) {
                            same[(size_t)(b * R + a)] = s;
                            both[(size_t)(b * R + a)] = bo;
                        }
                    }
                }
                if (a < R) {
                    nbr[(size_t)(a * Wr + tb)] = word;
                    written[(size_t)(a * Wr + tb)]++;
                }
            }
            if (ta != tb)
                for (int bl = 0; bl < SQ_ID_TILE; bl++)
                    if ((int64_t)tb * SQ_ID_TILE + bl < R) written[(size_t)(((int64_t)tb * SQ_ID_TILE + bl) * Wr + ta)]++;
        }
        for (int w : written)
            if (w != 1) { fprintf(stderr, "a word of the bit matrix was written %d times\n", w); return 2; }
        for (int64_t a = 0; a < R; a++) {
            neighbours[(size_t)a] = 1;
            for (int64_t w = 0; w < Wr; w++) neighbours[(size_t)a] += __builtin_popcountll(nbr[(size_t)(a * Wr + w)]);
        }
        SqIdentity::greedy(nbr.data(), R, kept.data());
        for (int v : len) printf("%d ", v);
        for (int v : bases) printf("%d ", v);
        for (int v : neighbours) printf("%d ", v);
        for (int64_t a = 0; a < R; a++) printf("%d ", (int)(kept[(size_t)(a / 64)] >> (a % 64) & 1ull));
        for (int v : same) printf("%d ", v);
        for (int v : both) printf("%d ", v);
        printf("\n");
    }
    return 0;
}
