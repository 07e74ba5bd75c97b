// sq_fold_pool.hip -- pools wider than one booked on the device (sq_pool.hip, sq_pool_round.hip): the plan of a fold's
// rounds, the rounds, and the device log of final structures as host lists for the host tail.
#include "sq_fold_run.h"

bool sq_pool_plan(const sq_batch *b, const SqLane &ln, int S0, int maxn, int64_t maxcap, SqPoolPlan &p)
{
    const SqFoldSwitches &sw = b->sw;
    const SqPoolIO &PI = b->pool_io;
    const int64_t avail = b->cand_records - b->cand_reserved;
    int slots = std::min(PI.smax, ln.max_structs);
    if (sw.pool_slots > 0) slots = std::min(slots, sw.pool_slots);   // (tests: force the overflow path)
    // structures whose candidates fit the arena at once; larger generations go through state .. choose in chunks
    // root lists (sequences beyond the scanning round kernel's 256 nt, up to 1,024): 16 bytes per run of the EMPTY structure
    // of every job, behind the structures' regions of the arena
    const int64_t root_units = (maxcap + 1) / 2;
    // kept lists (the batch reserved their pages: SQ_BATCH_POOL_LISTS): the same kernel, the parent's list in the root list's place
    const bool kept_mode = b->kept.on && !sw.no_pool_kept;
    bool root_mode = (sw.pool_root || kept_mode) && !sw.no_pool_round && maxn > SQ_PR_MAXN && maxn <= SQ_PR_ROOT_MAXN &&
                     (int64_t)S0 * root_units + std::max<int64_t>(maxcap, 1) <= avail;
    const int64_t avail_s = root_mode ? avail - (int64_t)S0 * root_units : avail;
    int chunk = (int)std::min<int64_t>(slots, avail_s / std::max<int64_t>(maxcap, 1));
    if (sw.pool_chunk > 0) chunk = std::min(chunk, sw.pool_chunk);   // (tests: force chunked rounds)
    if (S0 > slots || chunk < 1) return false;
    // On kept lists a structure keeps no candidates in the arena: its region only takes the runs within range of the best
    // finalscore that LDS has no room for -- SQ_KEPT_SLICE units, not the thousands a scan's output needs -- and a round is
    // one launch (at 500 nt the arena held the candidates of 8,224 structures: a generation of 170,000 went through it in
    // twenty launches of four waves of blocks each).  The root kernel still stages a job's runs in a full region: its
    // launches keep the regions' size.
    const int chunk_root = chunk;
    const int64_t kslice = 512;
    const bool kept_round = root_mode && kept_mode &&
                            sq_pool_round_lds(maxn, 2 * PI.pt + 2, b->cell_entries, sw.pool_round_nsurv ? std::max(sw.pool_round_nsurv, 128) : 128, PI.pt).total <= 60 * 1024;
    if (kept_round) {
        chunk = (int)std::min<int64_t>(slots, ((int64_t)chunk_root * maxcap) / kslice);
        if (sw.pool_chunk > 0) chunk = std::min(chunk, sw.pool_chunk);
    }
    p.slots = slots; p.chunk = chunk; p.chunk_root = chunk_root; p.maxcap = kept_round ? kslice : maxcap;
    p.root_mode = root_mode; p.kept_round = kept_round;
    // short sequences: a round is ONE kernel (sq_pool_round.hip) + the scan kernel -- on a crowded chip because wave slots
    // are what it runs out of, for a batch alone because two launches per round instead of six shorten the greedy loop
    // (SRtest150: 1.43 -> 1.28 ms, and the loop depends less on how fast the host turns a round around)
    SqPoolRoundArgs &pra = p.pra;
    bool round_kernel = (maxn <= SQ_PR_MAXN || root_mode) && !sw.no_pool_round;   // (jobs with a dense matrix too: sq_cellrun.h reads their cells there)
    if (round_kernel) {
        pra.lds_n = maxn; pra.str_cap = 2 * PI.pt + 2; pra.cell_entries = b->cell_entries;
        // survivors of :492 kept in LDS (the rest spill to the arena): on a crowded chip LDS is what the round kernel's waves
        // and everybody else's compete for -- 22 bytes x 256 survivors were half of a wave's 10 KB, and most structures have
        // a few dozen (round 4, a sweep of the count: 64 -> +5 % on the headline, 16 .. 64 within a per cent of each other)
        const bool crowded_fold = b->inflight > 1 || b->njobs >= 4096;
        pra.surv_cap = sw.pool_round_nsurv ? std::max(sw.pool_round_nsurv, root_mode ? 128 : 0) : (root_mode ? (kept_round ? 128 : 256) : (crowded_fold ? 64 : (maxn <= 96 ? 128 : 256))); pra.bound = b->score_bound ? 1 : 0;
        pra.tmax = PI.pt; pra.parity = 0; pra.lo = 0; pra.ahead = 0;
        pra.root = root_mode ? 1 : 0; pra.root_units = (int32_t)root_units; pra.root_off = (int64_t)chunk_root * maxcap;
        pra.kept = b->kept; pra.kept.on = kept_round ? 1 : 0;
        if (sq_pool_round_lds(pra.lds_n, pra.str_cap, pra.cell_entries, pra.surv_cap, pra.tmax).total > 60 * 1024) round_kernel = false;
    }
    p.round_kernel = round_kernel;
    return true;
}

// the pools of pool_jobs_v.  0: done, 1: capacity overflow (repeat on the host), < 0 / > 1: error in stats
int SqFoldRun::pool_fold(LoopStats &stats)
{
    std::vector<JobPool> &pools = *pools_p;
    SqLane &ln = b->lane_full;
    hipStream_t st = b->stream;
    SqPoolIO &PI = b->pool_io;
    const double tl0 = now_s();
    stats.tstart = tl0 - tfold0;
    struct Wall { double t0; double &dst; ~Wall() { dst = now_s() - t0; } } wall{tl0, stats.twall};
    auto fail = [&](int rc, const std::string &msg, int cap = 0) { stats.rc = rc; stats.err = msg; stats.cap = cap; return 2; };
    if (!PI.h_hdr) {
        void *p2 = nullptr, *p3 = nullptr, *p4 = nullptr, *p5 = nullptr, *p6 = nullptr;
        if (sq_pinned_get(&p2, sizeof(SqPoolHdr) * SQ_POOL_HDR_RING) || sq_pinned_get(&p3, sizeof(SqPoolJob) * (size_t)b->njobs) ||
            sq_pinned_get(&p4, sizeof(SqChain) * (size_t)b->njobs) || sq_pinned_get(&p5, sizeof(SqPoolJob) * (size_t)b->njobs) ||
            sq_pinned_get(&p6, 4 * (size_t)b->njobs)) return fail(2, sq_last_error());
        PI.h_hdr = (SqPoolHdr *)p2; PI.h_jobs = (SqPoolJob *)p3;
        b->h_pool_recs = (SqChain *)p4; b->h_pool_jobs = (SqPoolJob *)p5; b->h_pool_jobrec = (int32_t *)p6;
    }
    std::vector<int> jobs;
    int maxn = 0; int64_t maxcap = 0; bool need_reacts = false;
    for (int j : pool_jobs_v) {
        JobPool &P = pools[j];
        if (P.maxstemnum == 0) { P.fin.emplace_back(); continue; }   // :1123-1129 full before the first round
        const SqJob &J = b->jobs[j];
        maxn = std::max(maxn, J.n); maxcap = std::max<int64_t>(maxcap, J.cand_cap);
        need_reacts |= !J.default_reacts && !(J.react_levels > 0 && b->pset_classes[J.pset] * J.react_levels <= 32);
        jobs.push_back(j);
    }
    const int S0 = (int)jobs.size();
    if (S0 == 0) return 0;
    { const int pr = sq_prepare_scan(b); if (pr) return fail(pr, sq_last_error()); }
    SqPoolPlan plan;
    if (!sq_pool_plan(b, ln, S0, maxn, maxcap, plan)) return 1;
    const int slots = plan.slots, chunk = plan.chunk, chunk_root = plan.chunk_root;
    const bool root_mode = plan.root_mode, kept_round = plan.kept_round, round_kernel = plan.round_kernel;
    SqPoolRoundArgs &pra = plan.pra;
    for (int j = 0; j < b->njobs; j++) b->h_pool_jobrec[j] = -1;
    for (int sx = 0; sx < S0; sx++) {
        const int j = jobs[sx];
        const JobPool &P = pools[j];
        const int toff = sx * PI.pt;                     // generation 0, slot sx
        SqStruct &d = ln.h_structs[sx];
        d.job = j; d.strand_off = 2 * toff; d.nstrand = 0; d.slot = sx; d.subopt = P.cursubopt; d.cand_off = (int64_t)(sx % chunk_root) * maxcap;
        SqChain &cr = b->h_pool_recs[sx];
        cr.toff = toff; cr.tcap = PI.pt; cr.nstems = 0; cr.anycross = 0; cr.maxstems = P.maxstemnum;
        SqPoolJob &pj = b->h_pool_jobs[sx];
        pj.first = sx; pj.count = 1; pj.cursize = 1; pj.job = j;
        pj.cursubopt = P.cursubopt; pj.suboptinc = P.suboptinc; pj.suboptmax = P.suboptmax; pj.maxstems = P.maxstemnum; pj.evals = 0;
        b->h_pool_jobrec[j] = sx;
    }
    PI.slots = slots; PI.chunk = chunk; PI.poollim = o.poollim; PI.maxcap = plan.maxcap; PI.njobs = S0;   // (the kernels take the batch's record)
    PI.kept_ctr = kept_round ? b->kept.ctr : nullptr;
    if (PI.kept_ctr) hipMemsetAsync(PI.kept_ctr, 0, 16, st);
    const SqPoolIO pio = PI;
    SqScanArgs scan = b->scan;
    scan.ctr = ln.d_ctr;
    hipLaunchKernelGGL(sq_pool_init_kernel, dim3((std::max(S0, b->njobs) + 255) / 256), dim3(256), 0, st, ln.h_structs, b->h_pool_recs,
                       b->h_pool_jobs, b->h_pool_jobrec, (int32_t *)pio.jobrec_of, b->njobs, pio, scan, S0);
    auto wait_seq = [&](uint32_t seq, bool at_least = false) -> int {
        const int wr = sq_wait_word(b, ln.h_seq, seq, st, "pool round", at_least);
        return wr ? fail(wr, sq_last_error()) : 0;
    };
    if (round_kernel) b->last_paths |= 8;
    if (round_kernel && root_mode) {
        // the jobs' root lists: AnnotateStems of every job's empty structure, once (one wave per job)
        const size_t rl = sq_pool_root_lds(pra.lds_n, pra.cell_entries);
        if (rl > 60 * 1024) sq_max_dynamic_lds((const void *)sq_pool_root_kernel, 160 * 1024);
        // (in launches of at most `chunk` jobs: the kernel stages a job's runs in its empty structure's region of the arena,
        // and structures a chunk apart share a region)
        SqPoolIO pio_root = pio;
        pio_root.chunk = chunk_root; pio_root.maxcap = maxcap;
        for (int lo = 0; lo < S0; lo += chunk_root) {
            pra.lo = lo;
            hipLaunchKernelGGL(sq_pool_root_kernel, dim3(std::min(chunk_root, S0 - lo)), dim3(64), rl, st, b->ctx, scan, pio_root, pra);
        }
        pra.lo = 0;
        b->last_paths |= 64;
        if (kept_round) b->last_paths |= 128;
    }
    const size_t ext_lds = sq_extend_lds_bytes(pio.pt);          // the extend kernel's level scratch (dynamic LDS)
    if (ext_lds > 64 * 1024) sq_max_dynamic_lds((const void *)sq_pool_extend_kernel, 160 * 1024);
    const double tr0 = now_s();
    int parity = 0, S = S0, rounds = 0;
    bool overflow = false;
    // A batch alone: its rounds are a chain of short kernels, and waiting for a round's size before launching the next put
    // the host's turn-around -- a PCIe round trip and two launch latencies -- between every two of them (half of the greedy
    // loop of one SRtest150 batch).  With the one-kernel round the rounds are enqueued AHEAD instead: every launch covers
    // all the slots, blocks beyond the generation's size leave at once (sq_pool_round_kernel reads the size the scan kernel
    // left), and the host only follows the ring of published headers to learn when the pools have run empty.  Rounds
    // launched behind the last one find an empty generation.  (A crowded chip hides the turn-around behind other batches'
    // work and has tens of thousands of slots: it keeps the exact grids.)
    const int ahead_env = sw.pool_ahead;
    // (the slots in at most four launches per round: a generation larger than the candidate arena goes through it in chunks)
    const bool ahead = round_kernel && ahead_env > 0 && !(b->inflight > 1 || b->njobs >= 4096) && slots <= 8192 && (int64_t)chunk * 4 >= slots;
    if (ahead) {
        SqRoundIO io;
        io.h_strands = pio.strands; io.d_strands = pio.strands;
        io.h_out = ln.h_out; io.d_out = ln.d_out; io.h_cap = 0; io.out_cap = 0;
        io.h_ctr = ln.h_ctr; io.h_seq = ln.h_seq;
        io.h_structs = pio.structs; io.d_structs = pio.structs;
        int launched = 0, par_l = 0;
        bool stop = false;
        b->last_paths |= 32;
        while (!stop || rounds < launched) {
            while (!stop && launched - rounds < ahead_env) {
                if (launched > 4 * PI.pt + 8) return fail(2, "pool rounds do not terminate");
                pra.parity = par_l; pra.ahead = 1;
                for (int lo = 0; lo < slots; lo += chunk) {
                    pra.lo = lo;
                    if (const int lr = sq_launch_round_kernels(b, st, std::min(chunk, slots - lo), maxn, maxcap, need_reacts, 0.0, 0, io, scan, pio.structs + (size_t)par_l * pio.smax + lo, pio.strands, true, true, &pra)) return fail(lr, sq_last_error());
                }
                const uint32_t seq = ++*ln.round_seq;
                hipLaunchKernelGGL(sq_pool_scan_kernel, dim3(1), dim3(1024), 0, st, pio, scan, io, par_l, seq);
                launched++; par_l ^= 1;
            }
            const uint32_t seq = *ln.round_seq - (uint32_t)(launched - rounds - 1);   // the oldest round still out
            if (wait_seq(seq, true)) return 2;                  // (the rounds behind it write the same word: at least this one)
            rounds++;
            const SqCounters ctr = *ln.h_ctr;
            if (ctr.cand_ovf) return fail(-3, "candidate capacity exceeded (raise cand_per_nt)", SQ_CAP_CANDIDATES);
            if (ctr.level_ovf) return fail(-3, "more than 64 pseudoknot levels", SQ_CAP_FIXED);
            const SqPoolHdr hh = pio.h_hdr[seq % SQ_POOL_HDR_RING];
            if (timing && sw.pool_debug) fprintf(stderr, "[pool] round %d (of %d enqueued): next generation %u, nfin %u, ovf %u, active jobs %u\n", rounds, launched, hh.S[(rounds & 1)], hh.nfin, hh.ovf, hh.active_jobs);
            b->last_peak = std::max<int64_t>(b->last_peak, hh.peak);
            if (hh.ovf) { overflow = true; stop = true; }
            if (hh.S[rounds & 1] == 0) stop = true;         // (round r has parity r & 1; its scan kernel wrote the size of round r + 1)
        }
        S = 0;
    }
    while (S > 0) {
        b->last_peak = std::max<int64_t>(b->last_peak, S);
        SqStruct *cur = pio.structs + (size_t)parity * pio.smax;
        SqRoundIO io;
        io.h_strands = pio.strands; io.d_strands = pio.strands;
        io.h_out = ln.h_out; io.d_out = ln.d_out; io.h_cap = 0; io.out_cap = 0;
        io.h_ctr = ln.h_ctr; io.h_seq = ln.h_seq;
        for (int lo = 0; lo < S; lo += chunk) {              // (stream order: a chunk's chosen stems are out before the next one reuses the arena)
            io.h_structs = cur + lo; io.d_structs = cur + lo;
            pra.parity = parity; pra.lo = lo;
            if (const int lr = sq_launch_round_kernels(b, st, std::min(chunk, S - lo), maxn, maxcap, need_reacts, 0.0, 0, io, scan, cur + lo, pio.strands, true, true,
                                                       round_kernel ? &pra : nullptr)) return fail(lr, sq_last_error());
        }
        const uint32_t seq = ++*ln.round_seq;
        hipLaunchKernelGGL(sq_pool_scan_kernel, dim3(1), dim3(b->inflight > 1 ? 256 : 1024), 0, st, pio, scan, io, parity, seq);
        // (4 waves share a parent's children; on a crowded chip ONE takes them all: most parents have one or two, and a wave
        // that finds nothing to do still takes a slot for a microsecond or two -- 593 k -> 601 k)
        const int ext_crowd = sq_tuning().pool_extend_waves;
        const bool crowded = b->inflight > 1 || b->njobs >= 4096;
        if (!round_kernel)       // (the round kernel's structures extend themselves and log themselves)
            hipLaunchKernelGGL(sq_pool_extend_kernel, dim3(S, crowded ? ext_crowd : 4), dim3(64), ext_lds, st, b->ctx, scan, pio, parity);
        if (wait_seq(seq)) return 2;
        rounds++;
        const SqCounters ctr = *ln.h_ctr;
        if (ctr.cand_ovf) return fail(-3, "candidate capacity exceeded (raise cand_per_nt)", SQ_CAP_CANDIDATES);
        if (ctr.level_ovf) return fail(-3, "more than 64 pseudoknot levels", SQ_CAP_FIXED);
        const SqPoolHdr hh = pio.h_hdr[seq % SQ_POOL_HDR_RING];
        if (timing && sw.pool_debug) fprintf(stderr, "[pool] round %d: S %d -> %u, nfin %u, ovf %u, active jobs %u\n", rounds, S, hh.S[parity ^ 1], hh.nfin, hh.ovf, hh.active_jobs);
        if (hh.ovf) { overflow = true; break; }
        parity ^= 1;
        S = (int)hh.S[parity];
        if (rounds > 4 * PI.pt + 8) return fail(2, "pool rounds do not terminate");
    }
    {   // the last extend kernel's log entries and flags, the evaluation counts
        SqRoundIO io;
        io.h_structs = pio.structs; io.h_strands = pio.strands; io.d_structs = pio.structs; io.d_strands = pio.strands;
        io.h_out = ln.h_out; io.d_out = ln.d_out; io.h_cap = 0; io.out_cap = 0; io.h_ctr = ln.h_ctr; io.h_seq = ln.h_seq;
        const uint32_t seq = ++*ln.round_seq;
        hipLaunchKernelGGL(sq_pool_publish_kernel, dim3(1), dim3(256), 0, st, pio, scan, io, seq);
        if (wait_seq(seq)) return 2;
    }
    stats.nrounds = rounds;
    stats.tround = now_s() - tr0;
    if (timing && PI.kept_ctr) {
        uint32_t kc[4] = {0, 0, 0, 0};
        hipMemcpy(kc, PI.kept_ctr, 16, hipMemcpyDeviceToHost);
        fprintf(stderr, "[pool] kept lists: %u pages per generation, most taken %u, structures that left no list %u\n", b->kept.npages, kc[2], kc[3]);
    }
    const SqPoolHdr hh = pio.h_hdr[*ln.round_seq % SQ_POOL_HDR_RING];
    if (overflow || hh.ovf) {
        tq.flush();                                      // (the optimistic chains' entries are still being turned into lists by the queue's workers)
        for (int j : greedy_jobs) { pools[j].fin.clear(); pools[j].evals = 0; }
        // (the device log holds the structures the aborted pools had finished: they leave it for the host loop's.  The E / H / N
        // stemsets of the device RunAlgo stay -- their finish kernels append on the side streams: wait for them first, the
        // host loop that follows is the slow path anyway.  Round 3 emptied the whole log here and lost those stemsets)
        for (int q = 0; q < 4; q++) if (b->side[q]) hipStreamSynchronize(b->side[q]);
        hipLaunchKernelGGL(sq_fin_keep_algos_kernel, dim3(1), dim3(1024), 0, st, b->d_fin, b->d_fin_ctr, b->fin_cap, b->d_job_evals, b->tail.job_cnt, b->njobs);
        return 1;
    }
    if ((*ln.h_ctr).level_ovf) return fail(-3, "more than 64 pseudoknot levels", SQ_CAP_FIXED);
    // finstemsets of every job: its log entries in (round, kind, position) order.  With the device tail the log is
    // consumed where it is; the host needs it only when the batch falls back to the host tail (pool_collect).
    pool_jobs = jobs;
    pool_hdr = hh;
    pool_logged = true;
    if (!dev_tail) { const int rc2 = pool_collect(); pool_logged = false; if (rc2) return fail(rc2, sq_last_error()); }
    if (!dev_tail) for (int sx = 0; sx < S0; sx++) pools[jobs[sx]].evals += pio.h_jobs[sx].evals;
    if (b->prof_on)                                      // 2 N^2 bytes per evaluation (live structures only)
        for (int sx = 0; sx < S0; sx++) { const double n = b->jobs[jobs[sx]].n; b->prof[2].bytes += (double)pio.h_jobs[sx].evals * 2.0 * n * n; }
    return 0;
}

// the device pools' log -> pools[].fin of their jobs, in (round, kind, position) order (the host tail's input)
int SqFoldRun::pool_collect()
{
    std::vector<JobPool> &pools = *pools_p;
    const SqPoolHdr &hh = pool_hdr;
    const int S0 = (int)pool_jobs.size();
    std::vector<SqPoolFin> Fv(hh.nfin);
    std::vector<SqPoolStem> Sv(hh.nfin_stems);
    if (hh.nfin) HIPCK(hipMemcpy(Fv.data(), b->d_fin, sizeof(SqPoolFin) * (size_t)hh.nfin, hipMemcpyDeviceToHost));
    if (hh.nfin_stems) HIPCK(hipMemcpy(Sv.data(), b->d_fin_stems, sizeof(SqPoolStem) * (size_t)hh.nfin_stems, hipMemcpyDeviceToHost));
    const SqPoolFin *F = Fv.data();
    std::vector<uint32_t> start((size_t)b->njobs + 1, 0), ord(hh.nfin);
    // (entries below SQ_FIN_KIND_G0 are E / H / N stemsets: not the pools')
    for (uint32_t q = 0; q < hh.nfin; q++) if (F[q].round_kind >= SQ_FIN_KIND_G0) start[(size_t)F[q].job + 1]++;
    for (int j = 0; j < b->njobs; j++) start[(size_t)j + 1] += start[j];
    {
        std::vector<uint32_t> fillp(start.begin(), start.end() - 1);
        for (uint32_t q = 0; q < hh.nfin; q++) if (F[q].round_kind >= SQ_FIN_KIND_G0) ord[fillp[F[q].job]++] = q;
    }
    auto one_job = [&](int sx) {
        const int j = pool_jobs[sx];
        uint32_t *p0 = ord.data() + start[j], *p1 = ord.data() + start[(size_t)j + 1];
        std::sort(p0, p1, [&](uint32_t x, uint32_t y) {
            if (F[x].round_kind != F[y].round_kind) return F[x].round_kind < F[y].round_kind;
            return F[x].pos < F[y].pos;
        });
        auto &fin = pools[j].fin;
        fin.reserve(fin.size() + (size_t)(p1 - p0));
        for (uint32_t *p = p0; p < p1; p++) {
            const SqPoolFin &e = F[*p];
            const SqPoolStem *src = Sv.data() + e.stem_off;
            std::vector<HStem> stems((size_t)e.nstems);
            for (int t = 0; t < e.nstems; t++) stems[t] = HStem{src[t].i, src[t].j, src[t].len, 0.0, 0.0};
            fin.push_back(std::move(stems));
        }
    };
    if (hh.nfin >= 8192) sq_pool(b)->parallel_for(S0, one_job);
    else for (int sx = 0; sx < S0; sx++) one_job(sx);
    return 0;
}
