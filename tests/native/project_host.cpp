// Test-only host harness: runs the product's projection logic (squarna_amd/csrc/sq_project.h, the logic of sq_project_rows and
// sq_lift_rows) on the CPU as one thread, so tests can compare it with plain loops over characters without a GPU: the chunk
// walk of every row (the ballot of a chunk is formed lane by lane), the exclusive bases, col_of / pos_of, and per line the
// validity pass, the judgement of every paired column, the counts, and the lift through chunk_of + select64.  Every output
// buffer starts as a sentinel and the harness fails when a cell is left unwritten or written outside its row.  It checks by
// itself that col(pos(c)) == c for every residue column and that select64 agrees with clearing the lowest set bits.
// stdin: N, then per case: mode (0 project, 1 lift) R L K shared canonical_only min_loop, the R rows as strings of L
// characters, then for mode 0 the lines (K when shared, else R * K) of L partners each, for mode 1 per row "n w" and n lines
// of w partners (w >= the row's residues).
// stdout: first one line "THREADS MAX_BLOCKS MAX_COLS MAX_ROWS MAX_WORDS COUNTS"; then per case one line: Lmax, length[R],
// col_of[R * Lmax], pos_of[R * L], and for mode 0 partner[R * K * Lmax], cls[R * K * L], counts[R * K * 12], status[R * K],
// for mode 1 partner[R * K * L], status[R * K].
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../squarna_amd/csrc/sq_project.h"

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 2; } while (0)
static const int32_t UNWRITTEN = -77;

struct Map {
    std::vector<uint64_t> word;
    std::vector<int32_t> base;
    std::vector<uint8_t> cls;
    int32_t nW = 0, length = 0;
};

// the chunk walk of one row: the kernel's, with the wave's ballot formed lane by lane
static void walk(const uint8_t tab[256], const std::string &row, int32_t L, Map &m)
{
    m.nW = SqProject::words(L);
    m.word.assign((size_t)m.nW, 0);
    m.base.assign((size_t)m.nW + 1, 0);
    m.cls.assign((size_t)L, 0);
    for (int32_t j = 0; j < m.nW; j++) {
        uint64_t mask = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int32_t c = j * 64 + lane;
            const uint8_t k = c < L ? tab[(uint8_t)row[(size_t)c]] : (uint8_t)SQ_COV_GAP;
            if (c < L) m.cls[(size_t)c] = k;
            if (SqProject::is_residue(k)) mask |= (uint64_t)1 << lane;
        }
        m.word[(size_t)j] = mask;
        m.base[(size_t)j] = __builtin_popcountll(mask);
    }
    m.length = SqProject::exclusive_bases(m.base.data(), m.nW);
}

static void print_all(const std::vector<int32_t> &v)
{
    for (int32_t x : v) printf(" %d", x);
}

int main()
{
    int N;
    if (scanf("%d", &N) != 1) return 1;
    printf("%d %d %d %d %d %d\n", SQ_PROJ_THREADS, SQ_PROJ_MAX_BLOCKS, SQ_PROJ_MAX_COLS, SQ_PROJ_MAX_ROWS, SQ_PROJ_MAX_WORDS, SQ_PROJ_COUNTS);
    uint8_t tab[256];
    SqProject::fill_table(tab);
    for (uint64_t w : {0x1ull, 0x8000000000000000ull, 0xffffffffffffffffull, 0xa5a5a5a5deadbeefull, 0x0000000100000000ull}) {
        uint64_t rest = w;
        for (int k = 0; k < __builtin_popcountll(w); k++, rest &= rest - 1)
            if (SqProject::select64(w, k) != __builtin_ctzll(rest)) FAIL("select64(%llx, %d)", (unsigned long long)w, k);
    }
    while (N--) {
        int mode, R, L, K, shared, canonical_only, min_loop;
        if (scanf("%d %d %d %d %d %d %d", &mode, &R, &L, &K, &shared, &canonical_only, &min_loop) != 7 || mode < 0 || mode > 1 || R < 1 ||
            L < 1 || L > SQ_PROJ_MAX_COLS || K < 1 || min_loop < 0)
            return 1;
        std::vector<std::string> rows((size_t)R);
        std::vector<Map> maps((size_t)R);
        int32_t Lmax = 1;
        for (int r = 0; r < R; r++) {
            std::vector<char> buf((size_t)L + 1);
            char fmt[16];
            snprintf(fmt, sizeof fmt, "%%%ds", L);                   // (at most L characters; the test writes exactly L, without blanks)
            if (scanf(fmt, buf.data()) != 1) return 1;
            rows[(size_t)r] = buf.data();
            if ((int32_t)rows[(size_t)r].size() != L) return 1;
            walk(tab, rows[(size_t)r], L, maps[(size_t)r]);
            if (maps[(size_t)r].length > Lmax) Lmax = maps[(size_t)r].length;
        }
        std::vector<int32_t> length((size_t)R, UNWRITTEN), col_of((size_t)R * Lmax, UNWRITTEN), pos_of((size_t)R * L, UNWRITTEN);
        for (int r = 0; r < R; r++) {
            const Map &m = maps[(size_t)r];
            length[(size_t)r] = m.length;
            for (int32_t c = 0; c < L; c++) {
                const bool res = SqProject::residue_at(m.word.data(), c);
                const int32_t i = SqProject::pos(m.word.data(), m.base.data(), c);
                pos_of[(size_t)r * L + c] = res ? i : -1;
                if (res) {
                    if (i < 0 || i >= m.length) FAIL("pos %d of column %d, length %d", i, c, m.length);
                    if (SqProject::col(m.word.data(), m.base.data(), m.nW, i) != c) FAIL("col(pos(%d)) != %d", c, c);
                    if (col_of[(size_t)r * Lmax + i] != UNWRITTEN) FAIL("col_of written twice");
                    col_of[(size_t)r * Lmax + i] = c;
                }
            }
            for (int32_t i = m.length; i < Lmax; i++) col_of[(size_t)r * Lmax + i] = -1;
        }
        printf("%d", Lmax);
        print_all(length);
        print_all(col_of);
        print_all(pos_of);
        if (mode == 0) {
            const int nlines = shared ? K : R * K;
            std::vector<int32_t> structs((size_t)nlines * L);
            for (auto &x : structs)
                if (scanf("%d", &x) != 1) return 1;
            std::vector<int32_t> partner((size_t)R * K * Lmax, UNWRITTEN), cls((size_t)R * K * L, UNWRITTEN),
                counts((size_t)R * K * SQ_PROJ_COUNTS, UNWRITTEN), status((size_t)R * K, UNWRITTEN);
            const int64_t row_stride = shared ? 0 : (int64_t)K * L;
            for (int r = 0; r < R; r++)
                for (int k = 0; k < K; k++) {
                    const Map &m = maps[(size_t)r];
                    const int32_t *line = structs.data() + r * row_stride + (int64_t)k * L;
                    int32_t *out = partner.data() + ((size_t)r * K + k) * Lmax, *out_cls = cls.data() + ((size_t)r * K + k) * L;
                    int32_t cnt[SQ_PROJ_COUNTS] = {};
                    bool bad = false;
                    for (int32_t c = 0; c < L; c++) {
                        const int32_t p = line[c];
                        const int32_t back = p >= 0 && SqProject::partner_in_range(p, L) ? line[p] : c;
                        bad |= SqProject::column_bad(c, p, back, L);
                    }
                    if (!bad) {
                        for (int32_t c = 0; c < L; c++) {
                            const int32_t p = line[c];
                            int pc = SQ_PROJ_NONE;
                            bool keep = false, loop_drop = false;
                            if (p >= 0)
                                pc = SqProject::judge(m.cls.data(), m.word.data(), m.base.data(), c, p, canonical_only != 0, min_loop, keep, loop_drop);
                            const bool opens = p > c;
                            out_cls[c] = opens ? pc : SQ_PROJ_NONE;
                            if (SqProject::residue_at(m.word.data(), c)) {
                                const int32_t i = SqProject::pos(m.word.data(), m.base.data(), c);
                                if (out[i] != UNWRITTEN) FAIL("partner written twice");
                                out[i] = keep ? SqProject::pos(m.word.data(), m.base.data(), p) : -1;
                            }
                            if (opens) {
                                cnt[SQ_PROJ_CNT_PAIRS]++;
                                cnt[pc]++;
                                cnt[SQ_PROJ_CNT_DROPPED] += loop_drop;
                                cnt[SQ_PROJ_CNT_KEPT] += keep;
                            }
                        }
                        for (int32_t i = m.length; i < Lmax; i++) out[i] = -1;
                    } else {
                        for (int32_t i = 0; i < Lmax; i++) out[i] = -1;
                        for (int32_t c = 0; c < L; c++) out_cls[c] = SQ_PROJ_NONE;
                    }
                    for (int q = 0; q < SQ_PROJ_COUNTS; q++) counts[((size_t)r * K + k) * SQ_PROJ_COUNTS + q] = cnt[q];
                    status[(size_t)r * K + k] = bad ? SQ_PROJ_INVALID : SQ_PROJ_OK;
                }
            for (const auto *v : {&partner, &cls, &counts, &status})
                for (int32_t x : *v)
                    if (x == UNWRITTEN) FAIL("a cell was left unwritten");
            print_all(partner);
            print_all(cls);
            print_all(counts);
            print_all(status);
        } else {
            std::vector<int32_t> partner((size_t)R * K * L, UNWRITTEN), status((size_t)R * K, UNWRITTEN);
            for (int r = 0; r < R; r++) {
                const Map &m = maps[(size_t)r];
                int n, w;
                if (scanf("%d %d", &n, &w) != 2 || n < 0 || n > K || w < m.length) return 1;
                std::vector<int32_t> mine((size_t)n * w + 1);
                for (size_t q = 0; q < (size_t)n * w; q++)
                    if (scanf("%d", &mine[q]) != 1) return 1;
                for (int k = 0; k < K; k++) {
                    int32_t *out = partner.data() + ((size_t)r * K + k) * L;
                    const int32_t *line = mine.data() + (size_t)(k < n ? k : 0) * w;
                    bool bad = false;
                    for (int32_t i = 0; k < n && i < m.length; i++) {
                        const int32_t p = line[i];
                        const int32_t back = p >= 0 && SqProject::partner_in_range(p, m.length) ? line[p] : i;
                        bad |= SqProject::column_bad(i, p, back, m.length);
                    }
                    const bool valid = k < n && !bad;
                    for (int32_t c = 0; c < L; c++) {
                        int32_t to = -1;
                        if (valid && SqProject::residue_at(m.word.data(), c)) {
                            const int32_t p = line[SqProject::pos(m.word.data(), m.base.data(), c)];
                            if (p >= 0) to = SqProject::col(m.word.data(), m.base.data(), m.nW, p);
                        }
                        out[c] = to;
                    }
                    status[(size_t)r * K + k] = bad ? SQ_PROJ_INVALID : SQ_PROJ_OK;
                }
            }
            for (const auto *v : {&partner, &status})
                for (int32_t x : *v)
                    if (x == UNWRITTEN) FAIL("a cell was left unwritten");
            print_all(partner);
            print_all(status);
        }
        printf("\n");
    }
    return 0;
}
