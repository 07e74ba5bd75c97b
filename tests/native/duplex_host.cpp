// Test-only host harness: runs the product's duplex summary (squarna_amd/csrc/sq_duplex.h, the logic of sq_duplex_summary) on
// the CPU as one thread, so tests can compare it with sets of pairs without a GPU.
// stdin: T, then per case: Ltot nsolo ndup ncell_s ncell_d same, then nsolo + 1 solo cell offsets, nsolo solo lengths, ncell_s
// solo partner entries, ndup + 1 duplex cell offsets, ndup duplex lengths, ncell_d duplex partner entries (same = 1: none, the
// duplex table is the solo table), ndup first chains, ndup second chains, nsolo + 1 position offsets.
// stdout: per case one line: status, then per duplex: valid inter intra_a intra_b lost_a lost_b a_first a_last b_first b_last,
// then Ltot counts per position.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../squarna_amd/csrc/sq_duplex.h"

template <class V> static bool read_all(V &v)
{
    long long x;
    for (auto &c : v) { if (scanf("%lld", &x) != 1) return false; c = (typename V::value_type)x; }
    return true;
}

int main()
{
    int T;
    if (scanf("%d", &T) != 1) return 1;
    while (T--) {
        long long Ltot, ncell_s, ncell_d;
        int nsolo, ndup, same;
        if (scanf("%lld %d %d %lld %lld %d", &Ltot, &nsolo, &ndup, &ncell_s, &ncell_d, &same) != 6) return 1;
        std::vector<int64_t> cell_off_s((size_t)nsolo + 1), lengths_s((size_t)nsolo), cell_off_d((size_t)ndup + 1), lengths_d((size_t)ndup),
            pos_off((size_t)nsolo + 1);
        std::vector<int32_t> partner_s((size_t)ncell_s), partner_d((size_t)(same ? 0 : ncell_d)), a_rec((size_t)ndup), b_rec((size_t)ndup);
        if (!read_all(cell_off_s) || !read_all(lengths_s) || !read_all(partner_s) || !read_all(cell_off_d) || !read_all(lengths_d) ||
            !read_all(partner_d) || !read_all(a_rec) || !read_all(b_rec) || !read_all(pos_off)) return 1;
        SqDuplex s;
        s.partner_s = partner_s.data(); s.cell_off_s = cell_off_s.data(); s.lengths_s = lengths_s.data(); s.nsolo = nsolo;
        s.partner_d = same ? partner_s.data() : partner_d.data(); s.cell_off_d = cell_off_d.data(); s.lengths_d = lengths_d.data();
        s.ndup = ndup; s.a_rec = a_rec.data(); s.b_rec = b_rec.data(); s.pos_off = pos_off.data(); s.Ltot = Ltot;
        std::vector<int32_t> bound((size_t)Ltot, 0);
        std::vector<long long> out;
        int status = 0;
        for (int32_t k = 0; k < ndup; k++) {
            SqDuplexShape h;
            long long c[5] = {0, 0, 0, 0, 0}, a_first = -1, a_last = -1, b_first = -1, b_last = -1;
            bool valid = s.shape(k, h);
            if (valid) {
                const int32_t *A = s.solo_row(h.a), *B = s.solo_row(h.b), *D = s.duplex_row(k);
                const int32_t n = h.nA + 1 + h.nB;
                for (int32_t t = 0; t < n; t++) {
                    const int f = SqDuplex::entry(A, B, D, h.nA, h.nB, t);
                    if (f & SQ_D_INVALID) { valid = false; continue; }
                    c[0] += !!(f & SQ_D_INTER_A); c[1] += !!(f & SQ_D_INTRA_A); c[2] += !!(f & SQ_D_INTRA_B);
                    c[3] += !!(f & SQ_D_LOST_A); c[4] += !!(f & SQ_D_LOST_B);
                    if (f & SQ_D_INTER_A) {
                        if (a_first < 0) a_first = t;
                        a_last = t;
                        bound[(size_t)(pos_off[(size_t)h.a] + t)]++;
                    }
                    if (f & SQ_D_INTER_B) {
                        const int32_t u = t - h.nA - 1;
                        if (b_first < 0) b_first = u;
                        b_last = u;
                        bound[(size_t)(pos_off[(size_t)h.b] + u)]++;
                    }
                }
            }
            if (!valid) status = 2;
            for (long long q : {(long long)valid, c[0], c[1], c[2], c[3], c[4], a_first, a_last, b_first, b_last}) out.push_back(q);
        }
        printf("%d", status);
        for (long long q : out) printf(" %lld", q);
        for (int32_t q : bound) printf(" %d", q);
        printf("\n");
    }
    return 0;
}
