// sq_fold_chain.hip -- chained rounds of width-1 pools (poollim 1, and the optimistic chains in front of the device pools):
// ONE launch of the persistent round kernel (sq_rounds.hip) per chain of structures, or rounds of launched kernels
// chained on the device (sq_chain.hip).
#include "sq_fold_run.h"
#include "sq_scan.h"

bool sq_rounds_shape(const sq_batch *b, int S, int maxn, int maxt, bool su, bool ties, int fly_letters, int &thr, SqRoundsArgs &ra)
{
    const int thr_env = sq_tuning().rounds_threads;
    // threads per structure: by length -- and, while the launch leaves the chip empty (a shard of a multi-GPU run, a
    // small batch), twice / four times that: a structure's rounds are a chain of dependent passes over its list that
    // more waves shorten (S1000 x 128: 1.21 -> 0.99 ms at 512 threads)
    // (end of round 6, 10,000 / 1,024 / 1,000 chains on one box: 300 nt 64 / 128 / 256 threads 1.93 / 2.08 / 2.63 ms; 1,000 nt
    // 128 / 256 / 512: 1.54 / 1.27 / 1.69; 2,000 nt 256 / 512 / 1,024: 6.59 / 6.28 / 8.33)
    thr = maxn <= 320 ? 64 : (maxn <= 450 ? 128 : (maxn < 1800 ? 256 : 512));                      // (1,500 nt x 1,000: 256 / 512 threads 2.93 / 3.21 ms)
    // (up to one block of 1,024 per CU: S2000 x 125 3.10 -> 2.80 ms with 1,024 instead of 512 threads; S1000 x 128 0.86 / 0.76 /
    // 0.75 ms with 256 / 512 / 1,024 -- there the pass over the list is no longer what a round waits for)
    while (!thr_env && thr < SQ_ROUNDS_THREADS && thr < maxn / 2 && ((int64_t)S * thr * 2 <= (int64_t)256 * 1024 || (S <= 256 && thr * 2 <= maxn / 2 + 64))) thr *= 2;   // (the chip's 256 x 16 wave slots: 1,250 chains of 300 nt 0.50 -> 0.47 ms at 128 threads, 512 of 1,000 nt 1.05 -> 0.99 at 512; 2,500 x 300 nt stay at 64: 0.65 against 0.72)
    if (thr_env) { thr = 64; while (thr * 2 <= thr_env) thr *= 2; }   // (a power of two: the survivor ring is indexed with a mask)
    ra.lds_n = maxn; ra.str_cap = 2 * maxt + 2; ra.tmax = maxt; ra.cell_entries = b->cell_entries;
    ra.su = su ? 1 : 0;
    // Pools that may branch (their chains can hand a job to the device pools): when the lists sized for a structure's BOUND
    // of stems -- n / (2 minlen): 1,178 at 4,700 nt, where a row takes ~370 -- keep a CU to one block, they are sized for
    // fewer (the largest of a few steps that lets two blocks of 512 threads share a CU); a structure that outgrows them
    // stops like one that meets a tie.  SQ_ROUNDS_TLDS=n: that size by hand (tests force the hand-over)
    if (ties && !thr_env) {
        const int tenv = b->sw.rounds_tlds;
        auto fits2 = [&](int t) { return sq_rounds_lds(ra.lds_n, 2 * t + 2, t, ra.cell_entries, 512, ra.su).total + 2048 <= 80 * 1024; };
        if (tenv) { if (tenv < maxt) { ra.tmax = tenv; ra.str_cap = 2 * tenv + 2; } }
        else if (S > 256 && maxn >= 1024 && !fits2(maxt))
            for (int t : {1024, 768, 640, 512, 448}) if (t < maxt && fits2(t)) { ra.tmax = t; ra.str_cap = 2 * t + 2; thr = std::max(thr, 512); break; }
    }
    // (long sequences: the per-position arrays and strand lists of ONE block fill most of a CU's LDS -- 90 KB at 4,700 nt --, so
    // the CU holds one block however many there are: it takes the wave slots the others cannot use.  512 rows of an
    // alignment ran as 512 blocks of four waves on 256 CUs)
    while (!thr_env && thr < SQ_ROUNDS_THREADS && thr < maxn / 2) {
        const size_t l1 = sq_rounds_lds(ra.lds_n, ra.str_cap, ra.tmax, ra.cell_entries, thr, ra.su).total + 2048;
        const size_t l2 = sq_rounds_lds(ra.lds_n, ra.str_cap, ra.tmax, ra.cell_entries, 2 * thr, ra.su).total + 2048;
        const size_t cu = 160 * 1024, r1 = std::min<size_t>(cu / l1 * thr, 1024), r2 = l2 <= 158 * 1024 ? std::min<size_t>(cu / l2 * 2 * thr, 1024) : 0;
        // (only while the LDS keeps a CU below half of its wave slots: a dozen one-wave blocks of 300-nt structures per CU
        // are better off as they are -- doubled, 10,000 chains of 300 nt took 2.08 instead of 1.93 ms)
        if (r2 > r1 && r1 <= 512) thr *= 2; else break;
    }
    ra.bound = b->score_bound ? 1 : 0; ra.ctx_min = 0; ra.ties = ties ? 1 : 0;
    {
        const int wmin = b->sw.wave_walk_min;
        ra.wave_min = wmin > 0 ? wmin : 0x7fffffff; ra.wave_lanes = b->sw.wave_walk_lanes; ra.no_early = b->sw.no_early_walk ? 1 : 0;
    }
    ra.fly = 0;
    while (thr > 64 && sq_rounds_lds(ra.lds_n, ra.str_cap, ra.tmax, ra.cell_entries, thr, ra.su).total + 2048 > 158 * 1024) thr /= 2;   // (long sequences: the survivor ring gives way)
    if (sq_rounds_lds(ra.lds_n, ra.str_cap, ra.tmax, ra.cell_entries, thr, ra.su).total + 2048 > 158 * 1024) return false;
    if (fly_letters > 0) {                         // the masks take the LDS of the strands and stems (the structure is empty during the scan)
        const SqRoundsLds lo = sq_rounds_lds(ra.lds_n, ra.str_cap, ra.tmax, ra.cell_entries, thr, ra.su);
        // (every length since the end of round 6: 10,000 chains of 100 / 150 / 250 / 300 / 350 nt 1.165 -> 1.128 / 1.337 -> 1.256 /
        // 1.787 -> 1.639 / 2.29 -> 2.12 / 2.607 -> 2.444 ms, S1000 x 1,024 1.47 -> 1.31.  Round 5 had measured S300 x 10,000 at
        // 1.78 with the bit kernel's matrices against 1.84 and kept them below 400 nt; the kernel has changed since.  SQ_FLY_MIN_N
        // sets a shortest length again)
        const int fly_min = sq_tuning().fly_min_n;
        if (maxn >= fly_min && fly_letters <= SQ_FLY_MAXL && sq_bits_fly_bytes(maxn, fly_letters) <= (size_t)(lo.off_tab - lo.off_str)) ra.fly = fly_letters;
    }
    return true;
}

// the chains of chain_jobs, as many structures per chain as the round buffers hold at once (one chain after the other)
void SqFoldRun::chain_fold(LoopStats &stats)
{
    std::vector<JobPool> &pools = *pools_p;
    SqLane &ln = b->lane_full;
    hipStream_t st = b->stream;
    const double tl0 = now_s();
    stats.tstart = tl0 - tfold0;
    struct Wall { double t0; double &dst; ~Wall() { dst = now_s() - t0; } } wall{tl0, stats.twall};
    auto fail = [&](int rc, const std::string &msg, int cap = 0) { stats.rc = rc; stats.err = msg; stats.cap = cap; };
    if (!b->chain.h_stems) {
        void *p0 = nullptr, *p1 = nullptr, *p2 = nullptr, *p3 = nullptr;
        if (sq_pinned_get(&p0, sizeof(SqStemOut) * (size_t)std::max<int64_t>(b->chain_T, 1)) ||
            sq_pinned_get(&p1, 8 * (size_t)b->njobs) || sq_pinned_get(&p2, 64) ||
            sq_pinned_get(&p3, sizeof(SqChain) * (size_t)b->njobs)) { fail(2, sq_last_error()); return; }
        b->chain.h_stems = (SqStemOut *)p0; b->chain.h_fin = (unsigned long long *)p1;
        b->chain.h_nfin = (volatile uint32_t *)p2; b->h_chain = (SqChain *)p3;
        b->chain_toff.resize(b->njobs);
        int32_t t = 0;
        for (int j = 0; j < b->njobs; j++) { b->chain_toff[j] = t; t += chain_tcap(b->jobs[j].n, b->psets[b->job_pset[j]].minlen); }
    }
    std::vector<int> finished;                          // queue items: sequences to rank (>= 0), chain entries (< 0)
    auto job_finished = [&](int j) {
        if (early_tail && --g_left[b->job_seq[j]] == 0) finished.push_back(b->job_seq[j]);
    };
    *b->chain.h_nfin = 0;
    bool first_chain = true;
    uint32_t nfin_seen = 0, nfin_goal = 0;              // entries of the finished list: handed on / expected after this chain
    // as many structures per chain as the round buffers hold at once (one chain after the other)
    const int64_t avail = b->cand_records - b->cand_reserved;
    size_t next_job = 0;
    while (next_job < chain_jobs.size() && !stats.rc) {
        std::vector<int> jobs;                              // structure index -> job
        int maxn = 0, maxt = 0; int64_t cand_off = 0, maxcap = 0; bool need_reacts = false;
        for (; next_job < chain_jobs.size(); next_job++) {
            const int j = chain_jobs[next_job];
            JobPool &P = pools[j];
            if (P.maxstemnum == 0) { P.fin.emplace_back(); job_finished(j); continue; }   // :1168-1174 full before the first round
            const SqJob &J = b->jobs[j];
            if ((int)jobs.size() == ln.max_structs || cand_off + J.cand_cap > avail) break;
            const int sx = (int)jobs.size();
            SqStruct &d = ln.h_structs[sx];
            d.job = j; d.slot = sx; d.subopt = P.cursubopt; d.cand_off = cand_off;
            cand_off += J.cand_cap; maxcap = std::max<int64_t>(maxcap, J.cand_cap);
            SqChain &cr = b->h_chain[sx];
            cr.toff = b->chain_toff[j]; cr.tcap = chain_tcap(J.n, b->psets[b->job_pset[j]].minlen);
            cr.nstems = 0; cr.anycross = 0; cr.maxstems = P.maxstemnum;
            d.strand_off = 4 * cr.toff; d.nstrand = 0;
            maxn = std::max(maxn, J.n); maxt = std::max(maxt, cr.tcap);
            need_reacts |= !J.default_reacts && !(J.react_levels > 0 && b->pset_classes[J.pset] * J.react_levels <= 32);
            jobs.push_back(j);
        }
        tq.push(finished);
        const int S = (int)jobs.size();
        if (S == 0) continue;
        nfin_goal += (uint32_t)S;
        SqRoundIO io;
        io.h_structs = ln.d_structs; io.h_strands = b->chain.strands; io.d_structs = ln.d_structs; io.d_strands = b->chain.strands;
        io.h_out = ln.h_out; io.d_out = ln.d_out; io.h_cap = 0; io.out_cap = 0;
        io.h_ctr = ln.h_ctr; io.h_seq = ln.h_seq;
        SqScanArgs scan = b->scan;
        scan.ctr = ln.d_ctr;
        // ONE launch for all rounds of these structures (sq_rounds.hip: a persistent block per structure) when every job
        // qualifies: per-position arrays and lists that fit the block's LDS.  Decided BEFORE anything is enqueued: a chain of
        // pools that may branch which the kernel cannot take goes to the device pools as it is, and the init kernel -- which
        // reads the pinned records the next chain overwrites -- is then never launched
        bool rounds_ok = !sw.no_rounds;
        for (int j : jobs) rounds_ok = rounds_ok && b->jobs[j].n <= SQ_ROUNDS_MAXN;
        int thr = 64;
        SqRoundsArgs ra;
        memset(&ra, 0, sizeof(ra));
        if (rounds_ok) {
            bool su = false;
            for (int j : jobs) if (b->seq_has_sep[(size_t)b->job_seq[j]]) { su = true; break; }
            rounds_ok = sq_rounds_shape(b, S, maxn, maxt, su, chain_ties, lazy_bits ? b->nletters : 0, thr, ra);
        }
        if (ra.fly == 0) { const int pr = sq_prepare_scan(b); if (pr) { fail(pr, sq_last_error()); return; } }
        if (!rounds_ok && chain_ties) {                       // (the launched rounds do not look for ties: the pools take these jobs)
            for (int j : jobs) tied_jobs.push_back(j);
            nfin_goal -= (uint32_t)S;
            continue;
        }
        hipLaunchKernelGGL(sq_chain_init_kernel, dim3((S + 255) / 256), dim3(256), 0, st, ln.h_structs, b->h_chain, ln.d_structs,
                           b->chain, scan, S, first_chain ? 1 : 0);
        first_chain = false;
        const uint32_t depth = sq_tuning().chain_depth;
        const uint32_t seq0 = *ln.round_seq;
        uint32_t launched = 0, done = 0;
        const bool relaxed = sq_relaxed_waits(b);
        const uint64_t poll_mask = relaxed ? 0x3FFF : 0xFFFFF;
        uint64_t spins = 0;
        volatile uint32_t *flag = ln.h_seq;
        const double tr0 = now_s();
        std::vector<std::pair<int, double>> round_t;
        if (rounds_ok) {
            const SqRoundsLds lo = sq_rounds_lds(ra.lds_n, ra.str_cap, ra.tmax, ra.cell_entries, thr, ra.su);
            {
                if (lo.total > 60 * 1024) sq_max_dynamic_lds((const void *)sq_rounds_kernel, 158 * 1024);   // (the kernel has static LDS too: 160 KB in all)
                {
                    ProfScope ps(b, 7, 0);
                    hipLaunchKernelGGL(sq_rounds_kernel, dim3(S), dim3(thr), lo.total, st, b->ctx, ln.d_structs, scan, b->chain, ra);
                }
                { const hipError_t le = hipGetLastError(); if (le != hipSuccess) { hipFuncAttributes fa; memset(&fa, 0, sizeof(fa)); hipFuncGetAttributes(&fa, (const void *)sq_rounds_kernel); fprintf(stderr, "[sq_fold] persistent rounds launch: S %d threads %d LDS %zu | kernel: maxThreadsPerBlock %d numRegs %d static LDS %zu maxDynamic %d local %zu\n", S, thr, lo.total, fa.maxThreadsPerBlock, fa.numRegs, fa.sharedSizeBytes, fa.maxDynamicSharedSizeBytes, fa.localSizeBytes); fail(sq_check(le, "persistent rounds launch"), sq_last_error()); } }
                const uint32_t seq = ++*ln.round_seq;
                hipLaunchKernelGGL(sq_chain_done_kernel, dim3(1), dim3(1), 0, st, io, scan, b->chain, seq);
                launched = 1;
                b->last_paths |= 4;
                if (dev_tail && !chain_ties && !b->prof_on && !any_ehn && !sw.no_defer_wait && next_job == chain_jobs.size() &&
                    nfin_goal == (uint32_t)S) {
                    deferred.on = true; deferred.goal = nfin_goal;
                    if (timing) fprintf(stderr, "[sq_fold] persistent rounds: the wait is deferred behind the device tail\n");
                    stats.nrounds += 1;
                    stats.tround += now_s() - tr0;
                    return;
                }
                if (timing) fprintf(stderr, "[sq_fold] persistent rounds: waiting (dev_tail %d ties %d prof %d pending %d next_job %zu of %zu goal %u S %d)\n", (int)dev_tail, (int)chain_ties, (int)b->prof_on, pending != nullptr, next_job, chain_jobs.size(), nfin_goal, S);
                { const int wr = sq_wait_word(b, flag, seq, st, "persistent rounds"); if (wr) fail(wr, sq_last_error()); }
                if (!stats.rc) {
                    const SqCounters ctr = *ln.h_ctr;
                    if (ctr.cand_ovf) fail(-3, "candidate capacity exceeded (raise cand_per_nt)", SQ_CAP_CANDIDATES);
                    else if (ctr.out_ovf) fail(-3, "stem capacity of a chained structure exceeded", SQ_CAP_FIXED);
                    else if (ctr.level_ovf) fail(-3, "more than 64 pseudoknot levels", SQ_CAP_FIXED);
                    else {
                        const uint32_t nf = *b->chain.h_nfin;
                        if (nf != nfin_goal) fail(2, "persistent rounds left structures unfinished");
                        if (chain_ties) for (uint32_t q = nfin_seen; q < nf; q++) if ((b->chain.h_fin[q] >> 62) & 1ull) tied_jobs.push_back((int)(uint32_t)b->chain.h_fin[q]);
                        if (!dev_tail) for (uint32_t q = nfin_seen; q < nf; q++) finished.push_back(-(int)q - 1);
                        nfin_seen = nf;
                        tq.push(finished);
                    }
                }
            }
        }
        while (!rounds_ok && nfin_seen < nfin_goal) {
            while (launched - done < depth) {               // rounds enqueued ahead of the device
                if ((int)launched > maxt + 2) { fail(2, "chained rounds do not terminate"); break; }
                // (algorithmic bytes: NOT per launch -- a launch also covers the structures that are already final; they are
                // booked below from the evaluations the list of finished structures records)
                if (const int lr = sq_launch_round_kernels(b, st, S, maxn, maxcap, need_reacts, 0.0, 0, io, scan, ln.d_structs, b->chain.strands, true)) { fail(lr, sq_last_error()); break; }
                const uint32_t seq = ++*ln.round_seq;
                hipLaunchKernelGGL(sq_chain_done_kernel, dim3(1), dim3(1), 0, st, io, scan, b->chain, seq);
                launched++;
            }
            if (stats.rc) break;
            const uint32_t d2 = *flag - seq0;
            if (d2 != done && d2 <= launched) {
                std::atomic_thread_fence(std::memory_order_acquire);
                done = d2; spins = 0;
                if (timing) round_t.push_back({(int)done, (now_s() - tr0) * 1e3});
                const SqCounters ctr = *ln.h_ctr;
                if (ctr.cand_ovf) { fail(-3, "candidate capacity exceeded (raise cand_per_nt)", SQ_CAP_CANDIDATES); break; }
                if (ctr.out_ovf) { fail(-3, "stem capacity of a chained structure exceeded", SQ_CAP_FIXED); break; }
                if (ctr.level_ovf) { fail(-3, "more than 64 pseudoknot levels", SQ_CAP_FIXED); break; }
                const uint32_t nf = *b->chain.h_nfin;
                if (!dev_tail) for (uint32_t q = nfin_seen; q < nf; q++) finished.push_back(-(int)q - 1);   // (device tail: the log has them)
                nfin_seen = nf;
                tq.push(finished);
                continue;
            }
            if ((++spins & poll_mask) == 0) {
                const hipError_t q = hipStreamQuery(st);
                if (q != hipErrorNotReady && q != hipSuccess) { fail(sq_check(q, "chained rounds"), sq_last_error()); break; }
                if (q == hipSuccess && *flag - seq0 != launched) { fail(2, "chained round did not signal completion"); break; }
            }
            sq_wait_step(spins, relaxed);
        }
        stats.nrounds += (int)launched;
        if (timing && (now_s() - tr0) > 8e-3) {
            fprintf(stderr, "[sq_fold] slow chain:");
            for (auto &rt : round_t) fprintf(stderr, " r%d@%.2f", rt.first, rt.second);
            fprintf(stderr, "\n");
        }
        // rounds still in flight find no live structure; they must be through before the buffers are used again
        hipStreamSynchronize(st);
        stats.tround += now_s() - tr0;
        if (b->prof_on && !stats.rc) {
            // 2 N^2 bytes per AnnotateStems evaluation = per round a structure was LIVE in (its stems + the
            // round that found none); exactly what sq_result_evals reports
            double bytes = 0;
            for (uint32_t q = nfin_goal - (uint32_t)S; q < nfin_goal; q++) {
                const unsigned long long e = b->chain.h_fin[q];
                if ((e >> 62) & 1ull) continue;
                const double n = b->jobs[(int)(uint32_t)e].n;
                const double ev = (double)((e >> 32) & 0x3FFFFFFFu) + ((e >> 63) ? 0.0 : 1.0);
                bytes += ev * 2.0 * n * n;
            }
            b->prof[rounds_ok ? 7 : 2].bytes += bytes;        // (the persistent round kernel covers the evaluations of all its rounds)
        }
    }
}
