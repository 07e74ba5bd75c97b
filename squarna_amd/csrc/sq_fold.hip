// sq_fold.hip -- sq_fold: the greedy pool loop of every job of a batch on the device drivers (persistent rounds, device pools) with the host loop as their fallback, E / H / N beside it, the ranking tail behind it; sq_fold_concurrent.
// The fold's state and stages: sq_fold_run.h; the chained rounds: sq_fold_chain.hip; the device pools: sq_fold_pool.hip.
#include "sq_fold_run.h"

SqFoldRun::PoolsDrop::~PoolsDrop()
{
    if (!p) return;
    // (pools that hold nothing -- chains and pools on the device drivers with the device tail: their structures never
    // reach the host lists -- go at once: starting the helper thread cost ~25 us of a 0.74-ms fold of 128 chains)
    bool empty = true;
    for (const JobPool &P : *p) if (!P.cur.empty() || !P.nxt.empty() || !P.fin.empty()) { empty = false; break; }
    if (empty) delete p; else std::thread([q = p] { CpuScope cpu_(11); delete q; }).detach();
}

// the log of final structures and the per-job evaluation counts start empty; every job's pool its paramset's range
void SqFoldRun::begin()
{
    // The ranking tail runs on the device (sq_tail_dev.hip) over the device log of final structures whenever the options
    // allow; the host tail below is its fallback.  The log and the per-job evaluation counts start empty.
    dev_tail = sq_tail_device_wanted(b, o);
    // the scoring kernel's two short cuts, per fold (tests fold the same batch with and without them)
    b->score_bound = !sw.no_score_bound;
    b->score_ctx = !sw.no_score_context;
    b->packed_ok = false;
    hipLaunchKernelGGL(sq_fold_begin_kernel, dim3((b->njobs + 256) / 256), dim3(256), 0, b->stream, b->d_fin_ctr, b->d_job_evals,
                       b->tail.job_cnt, b->njobs);
    pools_p = pools_drop.p = new std::vector<JobPool>(b->njobs);
    std::vector<JobPool> &pools = *pools_p;
    algos.resize(b->njobs);
    for (int j = 0; j < b->njobs; j++) {
        const sq_paramset &ps = b->psets[b->job_pset[j]];
        algos[j] = o.algos ? o.algos : ps.algorithms;       // :1065-1066
        JobPool &P = pools[j];
        P.cursubopt = ps.suboptmin;                         // :1069
        P.suboptinc = (ps.suboptmax - ps.suboptmin) / ps.suboptsteps;   // :1071
        P.suboptmax = ps.suboptmax; P.maxstemnum = ps.maxstemnum;
    }
}

// a-1, once per job and per fold (:1076): never reused from an earlier call, a fold is the whole path.  A fold whose every
// job is scanned exactly once -- width-1 pools on the persistent round kernel, no E / H / N -- does not write the bit
// matrices at all: the kernel's only scan forms the words it needs from letter masks in LDS (SqBitsFly, sq_scan.h; the bit
// kernel was 215 us of the 1.47 ms of an S1000 x 1,024 fold).  Every other path asks for the matrices (sq_prepare_scan).
// (a job whose dense matrix the FILL forms -- caller matrices, bpp terms, a multiplier of its own: score x mul or score + bpp
// in the fp64 arena, sq_kernels.hip -- needs that launch: the round kernel reads those cells as they are.  Only the rows
// weighted by the alignment's shared matrix are formed elsewhere)
int SqFoldRun::prepare_matrices()
{
    bool any_fill = false;
    for (int j = 0; j < b->njobs; j++) {
        any_ehn |= (algos[j] & (uint32_t)(SQ_ALGO_E | SQ_ALGO_H | SQ_ALGO_N)) != 0;
        any_fill |= b->jobs[j].has_ext != 0 && !b->jobs[j].mat64_diag;
    }
    lazy_bits = o.poollim == 1 && !sw.no_chain && !sw.no_rounds && !any_ehn && !any_fill && !b->interchainonly && b->nletters > 0 && !sw.no_fly_bits;
    b->bits_ready = false;
    return lazy_bits ? 0 : sq_fill_impl(b, 0);
}

// Edmonds / Hungarian / Nussinov paramsets (:1094-1100); their stemsets precede the greedy ones.
// The reference iterates a Python set of letters (unspecified order); we use E, H, N.
int SqFoldRun::algos_begin()
{
    ta = now_s();
    if (timing) fprintf(stderr, "[sq_fold] setup before E/H/N begin: %.3f ms (bit matrix launch + job pools)\n", (ta - fold_timer.t0) * 1e3);
    // (with the device tail: RunAlgo's filters on the device too when the batch qualifies, sq_algos_dev.hip)
    int r;
    { CpuScope cpu_(9); r = sq_algos_begin(b, algos, pending, o.levellimit, dev_tail); }   // AnnotateStems + matching kernels on side streams
    dev_algos = sq_algos_on_device(pending);
    b->last_paths = dev_algos ? 2 : 0;
    if (timing && pending) fprintf(stderr, "[sq_fold] RunAlgo for E / H / N: %s\n", dev_algos ? "on the device (sq_algos_dev.hip)" : "host-driven");
    if (r) return r;
    tbegin = now_s() - ta;
    tfold0 = now_s();
    return 0;
}

// Width-1 pools (poollim == 1): the greedy rounds are chained on the device (sq_chain.hip) when all structures fit
// the round buffers at once; otherwise (and for wider pools) the host drives the rounds.
int SqFoldRun::choose_drivers()
{
    for (int j = 0; j < b->njobs; j++) if (algos[j] & SQ_ALGO_G) greedy_jobs.push_back(j);
    use_chain = o.poollim == 1 && !sw.no_chain && !greedy_jobs.empty();   // (per fold: tests compare the drivers in one process)
    if (use_chain)
        for (int j : greedy_jobs)
            if (chain_tcap(b->jobs[j].n, b->psets[b->job_pset[j]].minlen) > SQ_CHAIN_TMAX ||
                b->jobs[j].cand_cap > b->cand_records - b->cand_reserved) use_chain = false;
    if (!use_chain) { const int r = sq_prepare_scan(b); if (r) return r; }   // (the host-driven lanes and the pools scan the matrices; asked for before any second thread runs)
    // Wider pools: booked on the device as well (sq_pool.hip) when the batch has the slot arrays (structures of at most
    // SQ_CHAIN_TMAX stems) and one structure per greedy job fits the round buffers; any capacity overflow during the fold makes
    // the host repeat it with its own loop.
    use_pool = !use_chain && o.poollim > 1 && !sw.no_pool && !greedy_jobs.empty() && b->pool_io.pt > 0;
    // the jobs each device driver takes.  Pools that may branch (poollim > 1) but rarely do -- range factor 1.0: only a run
    // that ties with the best AND shares a base with it branches (:769-789): `fastest` at the default pool limit, the
    // alignment's rows -- first run as chains on the persistent round kernel, which stops a structure at the first such tie;
    // the device pools then fold what is left (tied_jobs) and every other job
    if (use_chain) chain_jobs = greedy_jobs;
    if (use_pool) {
        for (int j : greedy_jobs) {
            const SqJob &J = b->jobs[j];
            const sq_paramset &ps = b->psets[b->job_pset[j]];
            const bool opt = !sw.no_opt_chain && !sw.no_rounds && ps.suboptmin == 1.0 && ps.suboptmax == 1.0 && J.n <= SQ_ROUNDS_MAXN &&
                             chain_tcap(J.n, ps.minlen) <= SQ_CHAIN_TMAX && J.cand_cap <= b->cand_records - b->cand_reserved;
            (opt ? chain_jobs : pool_jobs_v).push_back(j);
        }
        chain_ties = !chain_jobs.empty();
    }
    if (!use_chain && !use_pool) host_pools_init();
    return 0;
}

void SqFoldRun::host_pools_init()
{
    std::vector<JobPool> &pools = *pools_p;
    for (int j : greedy_jobs) {
        JobPool &P = pools[j];
        P.cur.clear(); P.nxt.clear(); P.fin.clear(); P.evals = 0; P.cursize = 1;
        P.cursubopt = b->psets[b->job_pset[j]].suboptmin;
        P.cur.emplace_back(); P.cur.back().job = j;       // :1105 one empty structure
    }
}

// the tails' bookkeeping, the tail queue, the lanes of the host loop
void SqFoldRun::tails_setup()
{
    for (int k = 0; k < 8; k++) g_t[k] = 0;
    // a-10 tail per sequence
    seq_jobs.resize(b->nseq);
    for (int j = 0; j < b->njobs; j++) seq_jobs[b->job_seq[j]].push_back(j);
    tail_cost.assign(b->nseq, 0.0);
    mark("job lists");
    tailed.assign(b->nseq, 0);
    // Early tails: without E/H/N stemsets a sequence is complete the moment the pools of its greedy jobs are empty;
    // the lanes report such sequences after every round and a helper thread ranks them on the worker pool while
    // the rounds of the other sequences go on.
    early_tail = pending == nullptr && !dev_tail;
    g_left = std::vector<std::atomic<int>>(early_tail ? b->nseq : 0);
    job_done.assign(early_tail ? b->njobs : 0, 0);
    if (early_tail) {
        for (int s2 = 0; s2 < b->nseq; s2++) g_left[s2] = 0;
        for (int j : greedy_jobs) g_left[b->job_seq[j]]++;
    }
    if (early_tail || use_chain || chain_ties) tq.start = [this] { sq_pool(b); tq.worker = std::thread([this] { tail_worker(); }); };
    mark("tail queue");
    // Two lanes when the batch is big enough: the jobs are dealt alternately (by sequence) to two host threads, each
    // driving its rounds on half of the round buffers; the kernels of both queue on the batch stream, so while one
    // lane's host code books a round the other lane's kernels run.  Jobs are independent: same results.
    const SqTuning &tu = sq_tuning();
    two_lanes = tu.fold_lanes >= 2 && !b->prof_on && (int)greedy_jobs.size() >= tu.lane_min_jobs &&
                (int)greedy_jobs.size() <= b->max_structs;   // (a lane holds half of the slots)
    sq_pool(b);                                             // (created before any second thread can ask for it)
}

void SqFoldRun::tail_one(int s)
{
    std::vector<JobPool> &pools = *pools_p;
    CpuScope cpu_(0);
    const double tt0 = timing ? now_s() : 0;
    struct TT { bool on; double t0; double &dst; ~TT() { if (on) dst = now_s() - t0; } } tt{timing, tt0, tail_cost[s]};
    std::vector<const std::vector<std::vector<HStem>> *> per_job;   // (freed later by the thread that allocated them)
    int64_t ev = 0;
    for (int j : seq_jobs[s]) { per_job.push_back(&pools[j].fin); ev += pools[j].evals; }
    const bool hr = has_ref && has_ref[s];
    const int32_t *rp = hr ? ref_pairs + 2 * (size_t)ref_off[s] : nullptr;
    const int nref = hr ? ref_off[s + 1] - ref_off[s] : 0;
    b->results[s] = SeqResult();
    sq_tail(b, s, o, per_job, seq_jobs[s], rp, nref, hr, b->results[s]);
    b->results[s].evals = ev;
}

// chained rounds: entry q of the device's list of finished structures (job | stems << 32 | by-count << 63) becomes
// the job's final stem list; handled by the queue's workers so that the thread that enqueues the rounds never waits
void SqFoldRun::chain_finish(uint32_t q)
{
    std::vector<JobPool> &pools = *pools_p;
    const unsigned long long e = b->chain.h_fin[q];
    if ((e >> 62) & 1ull) return;                       // a structure that stopped at a tie: the device pools fold its job
    const int j = (int)(uint32_t)e, nst = (int)((e >> 32) & 0x3FFFFFFFu);
    const bool by_count = (e >> 63) != 0;
    JobPool &P = pools[j];
    static_assert(sizeof(HStem) == sizeof(SqStemOut), "stem records must match");
    std::vector<HStem> stems((size_t)nst);
    if (nst) memcpy(stems.data(), b->chain.h_stems + b->chain_toff[j], sizeof(HStem) * (size_t)nst);
    P.fin.push_back(std::move(stems));
    P.evals += nst + (by_count ? 0 : 1);                // one evaluation per round the structure took part in
    const int s2 = b->job_seq[j];
    // (optimistic chains in front of the device pools: a sequence's other jobs may still be the pools', and a capacity overflow
    // there hands EVERY greedy job to the host loop -- nothing is ranked before the pools are through)
    if (early_tail && !chain_ties && --g_left[s2] == 0) { tail_one(s2); tailed[s2] = 1; }
}

// the tail queue's helper thread: sequences to rank (items >= 0) and chain entries (items < 0), on the worker pool
void SqFoldRun::tail_worker()
{
    if (b->device >= 0) hipSetDevice(b->device);
    for (;;) {
        std::vector<int> take;
        {
            std::unique_lock<std::mutex> lk(tq.mu);
            tq.cv.wait(lk, [&] { return !tq.items.empty() || tq.closed; });
            take.swap(tq.items);
            if (take.empty()) return;               // closed and drained
            tq.busy = true;
        }
        sq_pool(b)->parallel_for((int)take.size(), [&](int k) {
            if (take[k] < 0) chain_finish((uint32_t)(-(take[k] + 1)));       // (items < 0: chain entries)
            else { tail_one(take[k]); tailed[take[k]] = 1; }
        });
        { std::lock_guard<std::mutex> lk(tq.mu); tq.busy = false; }
        tq.idle_cv.notify_all();
    }
}

// the greedy pool loop (:1102-1199) for a subset of the jobs, on one lane of round buffers
void SqFoldRun::greedy_loop(SqLane &ln, const std::vector<int> &myjobs, LoopStats &stats)
{
    std::vector<JobPool> &pools = *pools_p;
    std::vector<SView> round;
    std::vector<int> owner;                             // job of each view
    std::vector<std::vector<HStem>> res;
    std::vector<int> finished;                          // sequences completed since the last report
    auto job_finished = [&](int j) {
        if (!early_tail || job_done[j]) return;
        job_done[j] = 1;
        if (--g_left[b->job_seq[j]] == 0) finished.push_back(b->job_seq[j]);
    };
    const double tl0 = now_s();
    stats.tstart = tl0 - tfold0;
    struct Wall { double t0; double &dst; ~Wall() { dst = now_s() - t0; } } wall{tl0, stats.twall};
    for (;;) {
        round.clear(); owner.clear();
        for (int j : myjobs) {
            JobPool &P = pools[j];
            if (P.cur.empty()) { job_finished(j); continue; }
            if (P.cur.size() > P.cursize) {             // :1162-1165
                P.cursize = P.cur.size();
                if (P.cursubopt < P.suboptmax) P.cursubopt += P.suboptinc;
            }
            bool anyfull = false;                       // :1168-1174
            for (auto &s : P.cur) if ((double)s.stems.size() == P.maxstemnum) { anyfull = true; break; }
            if (anyfull) {
                std::vector<HStruct> keep;
                for (auto &s : P.cur) {
                    if ((double)s.stems.size() == P.maxstemnum) P.fin.push_back(std::move(s.stems));
                    else keep.push_back(std::move(s));
                }
                P.cur.swap(keep);
                if (P.cur.empty()) { job_finished(j); continue; }
            }
            for (size_t k = 0; k < P.cur.size(); k++) {
                round.push_back(SView{j, P.cursubopt, &P.cur[k]});
                owner.push_back(j);
            }
            P.evals += (int64_t)P.cur.size();
        }
        tq.push(finished);
        if (round.empty()) break;
        { const double t0 = now_s(); stats.rc = sq_run_round_impl(b, ln, round, 0, res, nullptr); stats.tround += now_s() - t0; stats.nrounds++; }
        if (stats.rc) { stats.err = sq_last_error(); stats.cap = sq_last_capacity(); return; }
        // :1179-1196.  The entries of one job are contiguous in `round` and only touch that job's pool, so jobs
        // are independent; per job the entries are still handled in order.  Big rounds are shared among the
        // worker pool in contiguous slices (children mostly reuse their parent's storage: no allocator traffic).
        auto grow = [&](size_t q0, size_t q1) {
            CpuScope cpu_(3);
            for (size_t q = q0; q < q1; q++) {
                const int j = owner[q];
                JobPool &P = pools[j];
                const std::vector<HStem> &news = res[q];
                const HStruct &parent = *round[q].st;
                if (!news.empty()) {
                    const size_t stopper = P.cursize >= (size_t)o.poollim ? 1 : news.size();
                    for (size_t k = 0; k < stopper; k++) {
                        P.nxt.emplace_back();
                        sq_extend_struct(parent, news[k], P.nxt.back(), k + 1 == stopper);   // the last child inherits the vectors
                    }
                } else {
                    P.fin.push_back(std::move(const_cast<HStruct &>(parent).stems));   // the structure is final and leaves the pool
                }
            }
            for (size_t q = q0; q < q1; q++)
                if (q == q0 || owner[q] != owner[q - 1]) {   // once per job of the slice
                    JobPool &P = pools[owner[q]];
                    P.cur.swap(P.nxt);
                    P.nxt.clear();                      // (capacity stays)
                }
        };
        const size_t par_min = sq_tuning().grow_par;
        if (round.size() >= par_min) {
            const int nsl = sq_pool(b)->size() * 4;
            std::vector<size_t> cut(nsl + 1);
            for (int t = 0; t <= nsl; t++) {
                size_t q = round.size() * (size_t)t / (size_t)nsl;
                while (q > 0 && q < round.size() && owner[q] == owner[q - 1]) q++;   // slices end on job boundaries
                cut[t] = q;
            }
            sq_pool(b)->parallel_for(nsl, [&](int t) { if (cut[t] < cut[t + 1]) grow(cut[t], cut[t + 1]); }, round.size() >= 2048 ? 1 : 0);
        } else grow(0, round.size());
    }
}

// the host loop on two lanes: contiguous halves of the greedy jobs, the second lane on a thread and a stream of its own
int SqFoldRun::two_lane_loop()
{
    std::vector<int> part[2];
    // contiguous halves of equal estimated cost (~ n^3: rounds x cells), so that the lanes do not share cache
    // lines of neighbouring jobs' pools
    double total = 0, acc = 0;
    auto cost = [&](int j) { const double n = b->seq_off[b->job_seq[j] + 1] - b->seq_off[b->job_seq[j]]; return n * n * n + 1.0; };
    for (int j : greedy_jobs) total += cost(j);
    for (int j : greedy_jobs) { part[acc * 2 < total ? 0 : 1].push_back(j); acc += cost(j); }
    const int64_t avail = b->cand_records - b->cand_reserved;
    for (int k = 0; k < 2; k++) {
        SqLane &H = b->lane_half[k];
        H.cand0 = k ? avail / 2 : 0;
        H.cand_records = k ? avail - avail / 2 : avail / 2;
    }
    // the second lane has its own stream (its half-size kernels run beside the first lane's), ordered behind
    // everything the batch stream holds so far (bit matrix, uploads)
    if (!b->lane_stream) {
        HIPCK(sq_stream_get(b->device, &b->lane_stream));
        HIPCK(sq_event_get(b->device, &b->lane_ev));
    }
    HIPCK(hipEventRecord(b->lane_ev, b->stream));
    HIPCK(hipStreamWaitEvent(b->lane_stream, b->lane_ev, 0));
    b->lane_half[1].stream = b->lane_stream;
    std::thread other([&] { if (b->device >= 0) hipSetDevice(b->device); greedy_loop(b->lane_half[1], part[1], st1); });
    greedy_loop(b->lane_half[0], part[0], st0);
    other.join();
    if (!st0.rc && st1.rc) { st0.rc = st1.rc; st0.err = st1.err; st0.cap = st1.cap; }
    return 0;
}

// the greedy part on the drivers chosen: optimistic chains and the device pools, chains, or the host loop -- which also
// repeats a fold whose device pools ran out of a capacity
int SqFoldRun::greedy_part()
{
    mark("loop start");
    b->last_driver = use_pool ? 2 : use_chain ? 1 : 0;
    b->last_peak = use_chain ? (int64_t)greedy_jobs.size() : 0;
    if (use_pool && chain_ties) {
        // the optimistic chains first; their structures that met a tie hand their jobs to the pools
        chain_fold(st0);
        if (st0.rc) { tq.close(); sq_set_capacity_error(st0.rc == -3 ? st0.cap : 0, st0.err); return st0.rc; }
        b->last_paths |= 16;
        std::sort(tied_jobs.begin(), tied_jobs.end());
        pool_jobs_v.insert(pool_jobs_v.end(), tied_jobs.begin(), tied_jobs.end());
        std::sort(pool_jobs_v.begin(), pool_jobs_v.end());
        if (timing) fprintf(stderr, "[sq_fold] optimistic chains: %zu jobs, %zu met a tie and go to the device pools (with %zu others)\n",
                            chain_jobs.size(), tied_jobs.size(), pool_jobs_v.size() - tied_jobs.size());
        st0 = LoopStats();
    }
    if (use_pool) {
        const int pr = pool_jobs_v.empty() ? 0 : pool_fold(st0);
        if (pr == 1) { b->last_driver = 3; b->last_peak = 0; }
        if (pr == 1 && timing) fprintf(stderr, "[sq_fold] device pools: a capacity was exceeded, the host loop repeats the greedy part\n");
        if (pr == 1) {                                       // a capacity was exceeded: the host's own loop takes the fold
            st0 = LoopStats();
            use_pool = false;
            tq.flush();                                      // (no worker is still filling the lists the host loop starts from)
            host_pools_init();
            greedy_loop(b->lane_full, greedy_jobs, st0);
        }
    } else if (use_chain) {
        chain_fold(st0);
    } else if (!two_lanes) {
        greedy_loop(b->lane_full, greedy_jobs, st0);
    } else {
        const int r = two_lane_loop();
        if (r) return r;
    }
    tq.close();
    if (st0.rc) { sq_set_capacity_error(st0.rc == -3 ? st0.cap : 0, st0.err); return st0.rc; }
    tloop = now_s() - tfold0;
    ttail0 = now_s();
    return 0;
}

void SqFoldRun::take_sets(std::vector<JobSets> &sets, bool edmonds)
{
    std::vector<JobPool> &pools = *pools_p;
    for (auto it = sets.rbegin(); it != sets.rend(); ++it) {
        if ((it->algo == SQ_ALGO_E) != edmonds || it->streamed) continue;
        for (size_t k = 0; k < it->jobs.size(); k++) {
            JobPool &P = pools[it->jobs[k]];
            P.fin.insert(P.fin.begin(), std::move(it->sets[k]));
            P.evals++;
        }
    }
}

// E / H / N stemsets precede the greedy ones of their job (:1094-1100), in the order E, H, N.  Hungarian and
// Nussinov are final first; Edmonds is streamed job by job, and a sequence is ranked (its tail) the moment its
// last Edmonds graph is matched -- the other sequences do not wait for the largest graph of the batch.
int SqFoldRun::collect_algos()
{
    std::vector<JobPool> &pools = *pools_p;
    // (the known structures go to the device now: the tail's launches then follow the wait for the matching kernels directly)
    b->tail_refs_state = 0;
    if (dev_tail) (void)sq_tail_refs(b, ref_off, ref_pairs, has_ref);
    const double t0 = now_s();
    std::vector<std::atomic<int>> e_left(b->nseq);
    for (int s = 0; s < b->nseq; s++) e_left[s] = 0;
    for (int j = 0; j < b->njobs; j++) if (algos[j] & SQ_ALGO_E) e_left[b->job_seq[j]]++;
    SqAlgoEndHooks hooks;
    hooks.after_short = [&](std::vector<JobSets> &sets) { take_sets(sets, false); };
    hooks.on_e_job = [&](int j, std::vector<HStem> &set) {       // pool worker: job j's Edmonds stemset is final
        JobPool &P = pools[j];
        P.fin.insert(P.fin.begin(), std::move(set));
        P.evals++;
        const int s = b->job_seq[j];
        if (!dev_tail && --e_left[s] == 0) { tail_one(s); tailed[s] = 1; }
    };
    std::vector<JobSets> sets;
    int r;
    { CpuScope cpu_(10); r = sq_algos_end(b, pending, o.levellimit, sets, &hooks); }
    pending = nullptr;
    if (r) return r;
    bool streamed = false;
    for (const JobSets &js : sets) streamed |= js.streamed;
    if (!streamed) take_sets(sets, false);               // (the hook did not run: no Edmonds jobs, or not staged)
    take_sets(sets, true);
    if (timing) fprintf(stderr, "[sq_fold] E/H/N: begin %.3f ms, wait+collect (+ tails of finished sequences) after the greedy loop %.3f ms\n", tbegin * 1e3, (now_s() - t0) * 1e3);
    return 0;
}

// every final structure the HOST holds -- the E / H / N stemsets, the greedy ones when the host's own loop ran, the empty
// structure of a job with maxstemnum 0 -- joins the device log.  rt: 0 appended, 1 more than the log holds (the host tail
// takes the batch); the return value is an error
int SqFoldRun::append_host_lists(int &rt)
{
    std::vector<JobPool> &pools = *pools_p;
    size_t nent = 0, nst = 0;
    for (int j = 0; j < b->njobs; j++) { nent += pools[j].fin.size(); for (const auto &f : pools[j].fin) nst += f.size(); }
    rt = nent > (size_t)b->fin_cap || nst > (size_t)b->fin_stem_cap ? 1 : 0;
    if (!rt && nent) {
        const size_t need = sizeof(SqPoolFin) * nent + sizeof(SqPoolStem) * nst + 8 * (size_t)b->njobs + 64;
        if (b->h_app_cap < need) {
            hipStreamSynchronize(b->stream);
            sq_pinned_put(b->h_app); b->h_app = nullptr; b->h_app_cap = 0;
            void *p = nullptr;
            if (sq_pinned_get(&p, need + need / 2)) return 2;
            b->h_app = (char *)p; b->h_app_cap = need + need / 2;
        }
        SqPoolFin *ef = (SqPoolFin *)b->h_app;
        SqPoolStem *es = (SqPoolStem *)(b->h_app + sizeof(SqPoolFin) * nent);
        long long *ev = (long long *)(b->h_app + sizeof(SqPoolFin) * nent + ((sizeof(SqPoolStem) * nst + 7) & ~(size_t)7));
        size_t qe = 0, qs = 0;
        const bool host_greedy = b->last_driver == 0 || b->last_driver == 3;
        for (int j = 0; j < b->njobs; j++) {
            const JobPool &P = pools[j];
            // (RunAlgo on the device: its stemsets are in the log already, the host lists hold greedy structures only)
            const int nalgo = dev_algos ? 0 : __builtin_popcount(algos[j] & (uint32_t)(SQ_ALGO_E | SQ_ALGO_H | SQ_ALGO_N));
            ev[j] = std::max<int64_t>(P.evals - nalgo, 0);
            for (size_t k = 0; k < P.fin.size(); k++) {           // [E][H][N] first, then the greedy structures, in list order
                const std::vector<HStem> &f = P.fin[k];
                ef[qe++] = SqPoolFin{j, (int)k < nalgo ? (uint32_t)k : SQ_FIN_KIND_G0, (int32_t)k, (int32_t)f.size(), (uint32_t)qs, 0u};
                for (const HStem &t : f) es[qs++] = SqPoolStem{(int16_t)t.i, (int16_t)t.j, (int16_t)t.len, 0};
            }
        }
        if (host_greedy) HIPCK(hipMemcpyAsync(b->d_job_evals, ev, 8 * (size_t)b->njobs, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(sq_fin_append_kernel, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, b->stream, ef, es, (int)nent,
                           b->d_fin, b->d_fin_stems, b->d_fin_ctr, b->fin_cap, b->fin_stem_cap);
    }
    return 0;
}

// ---- the device tail (sq_tail_dev.hip): the host's final structures join the device log, then the tail kernels rank every
// sequence and write the packed results; no per-sequence host code
int SqFoldRun::device_tail()
{
    if (!dev_tail) return 0;
    CpuScope cpu_(0);
    int rt = 0;
    { const int r = append_host_lists(rt); if (r) return r; }
    if (!rt) rt = sq_tail_device(b, o, ref_off, ref_pairs, has_ref);
    if (deferred.on) {
        // (the tail's last word is behind the round kernel's in stream order: after an error of the tail the stream is
        // drained first)
        if (rt) hipStreamSynchronize(b->stream);
        std::atomic_thread_fence(std::memory_order_acquire);
        const SqCounters ctr = *b->lane_full.h_ctr;
        if (ctr.cand_ovf) { sq_set_capacity_error(SQ_CAP_CANDIDATES, "candidate capacity exceeded (raise cand_per_nt)"); return -3; }
        if (ctr.out_ovf) { sq_set_capacity_error(SQ_CAP_FIXED, "stem capacity of a chained structure exceeded"); return -3; }
        if (ctr.level_ovf) { sq_set_error("more than 64 pseudoknot levels"); return -3; }
        if (*b->chain.h_nfin != deferred.goal) { sq_set_error("persistent rounds left structures unfinished"); return 2; }
    }
    if (rt == 0) {
        tails_done = true;
        b->last_paths |= 1;
    }
    else if (rt != 1) return rt;
    else {
        // the host tail takes the batch
        if (timing) fprintf(stderr, "[sq_fold] device tail: not applicable to this batch, the host tail runs\n");
        return collect_device_lists();
    }
    return 0;
}

// the structures the device drivers left in the log as host lists (the host tail's input)
int SqFoldRun::collect_device_lists()
{
    std::vector<JobPool> &pools = *pools_p;
    if (dev_algos) {
        // the E / H / N stemsets the device-side RunAlgo logged: to the front of their job's list, in the order E, H, N
        uint32_t ctr[4] = {0, 0, 0, 0};
        HIPCK(hipMemcpy(ctr, b->d_fin_ctr, 16, hipMemcpyDeviceToHost));
        const uint32_t nf = std::min(ctr[0], b->fin_cap), ns2 = std::min(ctr[1], b->fin_stem_cap);
        std::vector<SqPoolFin> Fv(nf);
        std::vector<SqPoolStem> Sv(ns2);
        if (nf) HIPCK(hipMemcpy(Fv.data(), b->d_fin, sizeof(SqPoolFin) * (size_t)nf, hipMemcpyDeviceToHost));
        if (ns2) HIPCK(hipMemcpy(Sv.data(), b->d_fin_stems, sizeof(SqPoolStem) * (size_t)ns2, hipMemcpyDeviceToHost));
        for (uint32_t kind = SQ_FIN_KIND_N + 1; kind-- > 0;)      // N, then H, then E: each goes in front
            for (uint32_t q = 0; q < nf; q++) {
                const SqPoolFin &e = Fv[q];
                if (e.round_kind != kind) continue;
                std::vector<HStem> stems((size_t)e.nstems);
                for (int t = 0; t < e.nstems; t++) { const SqPoolStem &x = Sv[e.stem_off + t]; stems[t] = HStem{x.i, x.j, x.len, 0.0, 0.0}; }
                JobPool &P = pools[e.job];
                P.fin.insert(P.fin.begin(), std::move(stems));
                P.evals++;
            }
    }
    if (b->last_driver == 1 || (b->last_paths & 16)) {
        const uint32_t nf = *b->chain.h_nfin;
        for (uint32_t q = 0; q < nf; q++) chain_finish(q);
    }
    if (b->last_driver == 2 && pool_logged) {
        // (the E / H / N stemsets are already at the front of the lists: the greedy structures go behind them)
        const int rc2 = pool_collect();
        if (rc2) return rc2;
        for (size_t sx = 0; sx < pool_jobs.size(); sx++) pools[pool_jobs[sx]].evals += b->pool_io.h_jobs[sx].evals;
    }
    return 0;
}

// the remaining sequences: the batch's worker pool shares the tail, longest first (deterministic output)
void SqFoldRun::host_tails()
{
    if (tails_done) return;
    std::vector<JobPool> &pools = *pools_p;
    std::vector<int> order;
    std::vector<int64_t> cost(b->nseq, 0);
    for (int s = 0; s < b->nseq; s++) {
        if (tailed[s]) continue;
        order.push_back(s);
        for (int j : seq_jobs[s]) cost[s] += (int64_t)pools[j].fin.size() * (b->seq_off[s + 1] - b->seq_off[s]);
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost[x] > cost[y]; });
    sq_pool(b)->parallel_for((int)order.size(), [&](int k) { tail_one(order[k]); });
}

void SqFoldRun::report(long long cpu_fold0) const
{
    const double tround = st0.tround + st1.tround;
    const int nrounds = st0.nrounds + st1.nrounds;
    if (timing) {
        double mx = 0, sum = 0; int arg = 0;
        for (int q = 0; q < b->nseq; q++) { sum += tail_cost[q]; if (tail_cost[q] > mx) { mx = tail_cost[q]; arg = q; } }

        fprintf(stderr, "[sq_fold] tail: sum %.3f ms, max %.3f ms (seq %d, n=%d, %zu structures kept)\n", sum * 1e3, mx * 1e3, arg,
                b->seq_off[arg + 1] - b->seq_off[arg], b->results[arg].preds.size());
    }
    if (timing)
        fprintf(stderr, "[sq_fold] rounds=%d loop=%.3fms (round driver %.3f: prep %.3f gpu+wait %.3f post %.3f; pool %.3f) tail=%.3fms\n",
                nrounds, tloop * 1e3, tround * 1e3, g_t[0] * 1e3, g_t[1] * 1e3, g_t[2] * 1e3, (tloop - tround) * 1e3,
                (now_s() - ttail0) * 1e3);
    if (g_cpuacc_on) {
        static const char *nm[12] = {"tails", "collect", "edges", "grow|stemfilter", "post", "launch|hook", "wait", "annotate", "caller", "begin", "end", "teardown"};
        fprintf(stderr, "[sq_fold cpu ms]");
        g_cpuacc[8] += CpuScope::now() - cpu_fold0;
        for (int k = 0; k < 12; k++) fprintf(stderr, " %s %.2f", nm[k], g_cpuacc[k].exchange(0) * 1e-6);
        fprintf(stderr, "\n");
    }
    if (timing && use_chain)
        fprintf(stderr, "[sq_fold] chained rounds: start %.3f ms after the E/H/N launch, wall %.3f ms, %d rounds enqueued\n",
                st0.tstart * 1e3, st0.twall * 1e3, st0.nrounds);
    if (timing && two_lanes && !use_chain)
        fprintf(stderr, "[sq_fold] lanes: 0 start %.3f wall %.3f driver %.3f (%d rounds); 1 start %.3f wall %.3f driver %.3f (%d rounds)\n",
                st0.tstart * 1e3, st0.twall * 1e3, st0.tround * 1e3, st0.nrounds, st1.tstart * 1e3, st1.twall * 1e3, st1.tround * 1e3, st1.nrounds);
}

extern "C" int sq_fold(sq_batch *b, const sq_fold_opts *opts, const int32_t *ref_off, const int32_t *ref_pairs,
                       const uint8_t *has_ref)
{
    if (!b || !opts) { sq_set_error("bad argument"); return -1; }
    if (opts->poollim < 1) { sq_set_error("poollim must be positive"); return -1; }
    SqSlackGuard slack_guard;
    const long long cpu_fold0 = g_cpuacc_on ? CpuScope::now() : 0;
    sq_read_fold_switches(b->sw);
    SqFoldRun F(b, *opts, ref_off, ref_pairs, has_ref);     // (torn down in reverse: the tail queue, E / H / N, the pools)
    F.begin();
    int r = F.prepare_matrices();                           // a-1: the bit matrices, unless the round kernel forms its words
    if (!r) r = F.algos_begin();                            // E / H / N on side streams, beside the greedy part
    if (!r) r = F.choose_drivers();                         // chains, device pools or the host loop
    if (r) return r;
    F.tails_setup();
    if ((r = F.greedy_part())) return r;
    if ((r = F.collect_algos())) return r;                  // E / H / N stemsets to the front of their jobs' lists
    if ((r = F.device_tail())) return r;
    F.host_tails();
    F.report(cpu_fold0);
    return 0;
}

extern "C" int32_t sq_fold_driver(const sq_batch *b) { return b ? b->last_driver : -1; }
extern "C" int32_t sq_fold_paths(const sq_batch *b) { return b ? b->last_paths : -1; }
extern "C" int64_t sq_fold_peak_structs(const sq_batch *b) { return b ? b->last_peak : -1; }

extern "C" int sq_batch_set_inflight(sq_batch *b, int32_t n)
{
    if (!b) { sq_set_error("bad argument"); return -1; }
    b->inflight = n < 1 ? 1 : n;
    b->side_streams = b->inflight >= 3 ? 2 : 3;
    return 0;
}

extern "C" int sq_fold_concurrent(sq_batch *const *batches, int32_t nbatch, const sq_fold_opts *opts,
                                  const int32_t *const *ref_off, const int32_t *const *ref_pairs, const uint8_t *const *has_ref)
{
    return sq_fold_concurrent_n(batches, nbatch, opts, ref_off, ref_pairs, has_ref, 1);
}

extern "C" int sq_fold_concurrent_n(sq_batch *const *batches, int32_t nbatch, const sq_fold_opts *opts,
                                    const int32_t *const *ref_off, const int32_t *const *ref_pairs, const uint8_t *const *has_ref,
                                    int32_t reps)
{
    if (!batches || nbatch <= 0 || !opts || reps < 1) { sq_set_error("bad argument"); return -1; }
    for (int k = 0; k < nbatch; k++) if (!batches[k]) { sq_set_error("bad argument"); return -1; }
    std::vector<int> rc(nbatch, 0);
    std::vector<std::string> msg(nbatch);
    // every stream less keeps the long kernels of one batch out of another batch's hardware queue (GPU_MAX_HW_QUEUES)
    for (int k = 0; k < nbatch; k++) if (batches[k]) {
        batches[k]->side_streams = nbatch >= 3 ? 2 : 3;
        batches[k]->inflight = nbatch;
    }
    auto work = [&](int k) {
        if (k > 0 && batches[k]->device >= 0) hipSetDevice(batches[k]->device);
        for (int r = 0; r < reps && !rc[k]; r++)
            rc[k] = sq_fold(batches[k], opts, ref_off ? ref_off[k] : nullptr, ref_pairs ? ref_pairs[k] : nullptr,
                            has_ref ? has_ref[k] : nullptr);
        if (rc[k]) msg[k] = sq_last_error();                 // (the error text is per thread)
    };
    std::vector<std::thread> th;
    for (int k = 1; k < nbatch; k++) th.emplace_back(work, k);
    work(0);
    for (auto &t : th) t.join();
    // (a later fold of one of these batches alone is a fold with one batch in flight)
    for (int k = 0; k < nbatch; k++) if (batches[k]) { batches[k]->inflight = 1; batches[k]->side_streams = 3; }
    for (int k = 0; k < nbatch; k++) if (rc[k]) { sq_set_error(msg[k]); return rc[k]; }
    return 0;
}

