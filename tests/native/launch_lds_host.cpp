// The dynamic LDS layouts of the launched kernels (squarna_amd/csrc/sq_launch_lds.h) compiled for the host: one JSON object per
// input line.  A region prints as [byte offset, bytes per element, elements]; tests/test_launch_lds_host.py states the sizes a
// second time and checks the properties of the carving.
//   launch_lds_host fill     < "n"                                          launch_lds_host choose < "nsurv"
//   launch_lds_host masks    < "n letters"                                  launch_lds_host rank   < "waves bitwords keycap"
//   launch_lds_host state    < "maxn"                                       launch_lds_host pack   < "maxn tmax"
//   launch_lds_host scan     < "lds_n fbstride"                             launch_lds_host pairs  < "maxn"
//   launch_lds_host decide   < "maxn need_reacts mode nr_lim state_lim"     launch_lds_host limits < "bytes"
//   launch_lds_host score    < "lds_n lds_nr lds_ns cell_entries threads mode str_cap job_n"
//   launch_lds_host crossing < "cell_entries"     the smallest n whose mode-0 launch (float reactivities, 512 threads, 1,024 strands,
//                                                 the default staging limits) asks for more than SQ_LDS_PLAIN_MAX
#include <cstdio>
#include <cstring>
#include <string>
#include "../../squarna_amd/csrc/sq_launch_lds.h"

struct Json {
    std::string s = "{";
    void sep() { if (s.size() > 1) s += ", "; }
    void num(const char *k, long long v) { sep(); s += "\"" + std::string(k) + "\": " + std::to_string(v); }
    void reg(const char *k, size_t off, size_t size, size_t count)
    {
        sep();
        s += "\"" + std::string(k) + "\": [" + std::to_string(off) + ", " + std::to_string(size) + ", " + std::to_string(count) + "]";
    }
    void print() { s += "}"; puts(s.c_str()); }
};

static const int NR_LIM_DEFAULT = 4096;                 // SQ_SCORE_NR_LIM, SQ_SCORE_STATE_LIM when unset (sq_switches.h)
static const size_t STATE_LIM_DEFAULT = 24 * 1024;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    char line[256];
    if (cmd == "constants") {
        Json j;
        j.num("plain_max", SQ_LDS_PLAIN_MAX); j.num("block_max", SQ_LDS_BLOCK_MAX); j.num("fill_n", SQ_FILL_LDS_N);
        j.num("masks_max", SQ_MASKS_LDS_MAX); j.num("state_n", SQ_STATE_LDS_N); j.num("score_n", SQ_SCORE_LDS_N);
        j.num("refp_words", SQ_TAIL_REFP_WORDS); j.num("chunk", SQ_SCORE_CHUNK); j.num("strands", SQ_LDS_STRANDS);
        j.print();
        return 0;
    }
    while (fgets(line, sizeof line, stdin)) {
        long long a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int got = sscanf(line, "%lld %lld %lld %lld %lld %lld %lld %lld", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7);
        if (got < 1) continue;
        Json j;
        if (cmd == "fill") {
            const int n = (int)a[0];
            const SqFillLds L = sq_fill_lds(n);
            j.num("staged", sq_fill_staged(n));
            j.reg("attr", L.attr, 1, n); j.reg("inc4", L.inc4, 1, n); j.reg("chain", L.chain, 2, n); j.reg("react", L.react, 8, n);
            j.num("total", (long long)L.total);
        } else if (cmd == "masks") {
            const int n = (int)a[0], letters = (int)a[1];
            const SqMasksLds L = sq_bits_masks_lds(n, letters);
            j.num("fit", sq_bits_masks_fit(L)); j.num("nw", L.nw); j.num("bits_nw", sq_bits_nw(n));
            j.reg("ccode", L.ccode, 1, n); j.reg("rcode", L.rcode, 1, n); j.reg("inc", L.inc, 1, n);
            j.reg("M", L.M, 4, (size_t)letters * L.mw); j.reg("R", L.R, 4, (size_t)L.nw * letters);
            j.num("total", (long long)L.total);
        } else if (cmd == "state") {
            const int lds_n = sq_state_lds_n((int)a[0]);
            const SqStateLds L = sq_state_lds(lds_n);
            static char base[SQ_LDS_PLAIN_MAX];
            const SqStateArrays A = sq_state_carve(base, L);              // (what the kernel uses: must be the offsets)
            j.num("lds_n", lds_n);
            j.num("carved", (char *)A.P - base == (long)L.P && (char *)A.U - base == (long)L.U && (char *)A.SU - base == (long)L.SU &&
                                (char *)A.E - base == (long)L.E);
            // (a structure of n <= lds_n nt fills n + 1 entries of each array)
            j.reg("P", L.P, 2, (size_t)lds_n + 1); j.reg("U", L.U, 2, (size_t)lds_n + 1);
            j.reg("SU", L.SU, 2, (size_t)lds_n + 1); j.reg("E", L.E, 1, (size_t)lds_n + 1);
            j.num("total", (long long)L.total);
        } else if (cmd == "scan") {
            const SqStateScanLds L = sq_state_scan_lds((int)a[0], (int)a[1]);
            j.num("state", (long long)L.state.total); j.num("scan", (long long)L.scan); j.num("scan6", (long long)sq_scan6_lds((int)a[1]));
            j.num("total", (long long)L.total);
        } else if (cmd == "decide") {
            const int maxn = (int)a[0], mode = (int)a[2];
            const int lds_n = sq_score_lds_n(maxn), lds_nr = sq_score_lds_nr(maxn, a[1] != 0, (int)a[3]);
            j.num("lds_n", lds_n); j.num("lds_nr", lds_nr); j.num("lds_ns", sq_score_lds_ns(lds_n, lds_nr, maxn, mode, (size_t)a[4]));
        } else if (cmd == "score") {
            const int job_n = (int)a[7];
            const SqScoreLds L = sq_score_lds((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6]);
            const SqScoreJobLds J = sq_score_lds_job(L, job_n);
            j.num("ci_fits", J.ci_fits); j.num("reacts_fit", J.reacts_fit); j.num("state_fits", J.state_fits);
            j.reg("ci", J.ci, 1, job_n); j.reg("reacts", J.reacts, 8, job_n);
            j.reg("P", L.P, 2, (size_t)job_n + 1); j.reg("U", L.U, 2, (size_t)job_n + 1); j.reg("SU", L.SU, 2, (size_t)job_n + 1);
            j.num("state_np", L.state_np);
            j.reg("cell", L.cell, 8, (size_t)a[3]);
            j.reg("surv_bps", L.surv_bps, 8, L.surv_n); j.reg("surv_key", L.surv_key, 4, L.surv_n); j.reg("surv_len", L.surv_len, 2, L.surv_n);
            j.reg("str", L.str, SQ_STRAND_BYTES, L.str_cap); j.reg("skip", L.skip, 2, L.str_cap);
            j.num("total", (long long)L.total);
        } else if (cmd == "choose") {
            const int ns = (int)a[0];
            const SqChooseLds L = sq_pool_choose_lds(ns);
            j.reg("fin", L.fin, 8, ns); j.reg("q", L.q, 4, ns); j.reg("key", L.key, 4, ns); j.reg("ord", L.ord, 2, ns);
            j.num("total", (long long)L.total);
        } else if (cmd == "rank") {
            const int waves = (int)a[0], bw = (int)a[1], keycap = (int)a[2];
            const int refp = sq_tail_refp_lds(bw);
            const SqTailRankLds L = sq_tail_rank_lds(waves, bw, keycap, refp);
            j.num("refp_lds", refp);
            j.reg("bits", L.bits, 4, (size_t)waves * bw); j.reg("key", L.key, 8, 3 * (size_t)keycap); j.reg("pri", L.pri, 1, keycap);
            j.reg("codes", L.codes, 1, 32 * (size_t)bw); j.reg("refp", L.refp, 2, refp ? 32 * (size_t)bw : 0);
            j.num("total", (long long)L.total);
        } else if (cmd == "pack") {
            const SqTailPackLds L = sq_tail_pack_lds((int)a[0], (int)a[1]);
            j.num("rowcap", L.rowcap); j.num("ext_of_rowcap", (long long)sq_tail_pack_ext(L.rowcap));
            j.reg("row", L.row, 2, L.rowcap); j.reg("ext", L.ext, 16, sq_extend_lds_bytes((int)a[1]) / 16);
            j.num("ext_bytes", (long long)sq_extend_lds_bytes((int)a[1])); j.num("total", (long long)L.total);
        } else if (cmd == "pairs") {
            j.reg("row", 0, 4, (size_t)a[0]); j.num("total", (long long)sq_tail_pairs_lds((int)a[0]));
        } else if (cmd == "limits") {
            j.num("raise", sq_lds_needs_raise((size_t)a[0])); j.num("fits", sq_lds_fits((size_t)a[0]));
        } else if (cmd == "crossing") {
            // every n up to the reactivity limit at which the answer changes (it is not monotone: the state copies leave at some n)
            bool was = false; int k = 0;
            for (int n = 1; n <= NR_LIM_DEFAULT; n++) {
                const int lds_n = sq_score_lds_n(n), lds_nr = sq_score_lds_nr(n, true, NR_LIM_DEFAULT);
                const int lds_ns = sq_score_lds_ns(lds_n, lds_nr, n, 0, STATE_LIM_DEFAULT);
                const bool now = sq_lds_needs_raise(sq_score_lds(lds_n, lds_nr, lds_ns, (int)a[0], 512, 0, SQ_LDS_STRANDS).total);
                if (now != was) { const std::string key = "change" + std::to_string(k++); j.num(key.c_str(), n); }
                was = now;
            }
        } else return 2;
        j.print();
    }
    return 0;
}
