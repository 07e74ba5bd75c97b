// sq_fold_run.h -- the state of one sq_fold and its stages (sq_fold.hip: set-up, the host loop, E / H / N, the tails;
// sq_fold_chain.hip: the chained rounds; sq_fold_pool.hip: the device pools).  Internal to those three files.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include "sq_host_int.h"

// ---- a-7: greedy pool loop for every job at once (SQRNdbnseq.py:1102-1199) ----------------------
struct alignas(128) JobPool {                // (own cache lines: two lanes work on neighbouring jobs)
    std::vector<HStruct> cur;                // curstemsets
    std::vector<HStruct> nxt;                // next round's curstemsets (kept between rounds: no reallocation)
    std::vector<std::vector<HStem>> fin;     // finstemsets (greedy part)
    double cursubopt = 0, suboptinc = 0, suboptmax = 0, maxstemnum = 0;
    size_t cursize = 1;
    int64_t evals = 0;
};

// what one driver of the greedy part reports
struct LoopStats { double tround = 0, twall = 0, tstart = 0; int nrounds = 0; int rc = 0; int cap = 0; std::string err; };   // (cap: SQ_CAP_* of a status -3)

// Early tails and chain entries, handed to a helper thread that shares them out on the worker pool
struct TailQueue {
    std::mutex mu; std::condition_variable cv, idle_cv; std::vector<int> items; bool closed = false, busy = false;
    std::thread worker;
    std::function<void()> start; std::once_flag once; // (the worker starts with the first push -- the lanes push from threads of their own --:
                                                     // a fold whose drivers and tail stay on the device never feeds the queue, and
                                                     // starting + joining a thread was ~40 us of it)
    void push(std::vector<int> &v) { if (v.empty()) return; if (start) std::call_once(once, start); { std::lock_guard<std::mutex> lk(mu); items.insert(items.end(), v.begin(), v.end()); } cv.notify_one(); v.clear(); }
    // everything pushed so far has been handled when this returns (the worker stays: later pushes are served as before)
    void flush() { if (!worker.joinable()) return; std::unique_lock<std::mutex> lk(mu); idle_cv.wait(lk, [&] { return items.empty() && !busy; }); }
    void close() { if (!worker.joinable()) return; { std::lock_guard<std::mutex> lk(mu); closed = true; } cv.notify_one(); worker.join(); }
    ~TailQueue() { close(); }
};

// Launch shape of the persistent round kernel (sq_rounds.hip) for S structures of at most maxn nt and maxt stems: threads
// per block and the kernel's arguments.  su: some structure's sequence holds a separator; ties: the chains stop at a tie
// (optimistic chains in front of the device pools); fly_letters: the letters of a fold that writes no bit matrices (0: it
// does).  False when the block's LDS cannot hold even 64 threads' worth (the launched rounds take the chain).
bool sq_rounds_shape(const sq_batch *b, int S, int maxn, int maxt, bool su, bool ties, int fly_letters, int &thr, SqRoundsArgs &ra);

// The device pools' plan for S0 structures of generation 0 (longest sequence maxn, largest candidate region maxcap):
// structure slots, chunk of a launch, the form of a round (sq_pool_round.hip's kernel, over root / kept lists, or the
// launched kernels) and its arguments.  False when generation 0 does not fit (the host loop takes the fold).
struct SqPoolPlan {
    int slots = 0, chunk = 0, chunk_root = 0;
    int64_t maxcap = 0;                      // (of the launches: a kept list's slice on kept lists)
    bool root_mode = false, kept_round = false, round_kernel = false;
    SqPoolRoundArgs pra;
};
bool sq_pool_plan(const sq_batch *b, const SqLane &ln, int S0, int maxn, int64_t maxcap, SqPoolPlan &p);

struct SqFoldRun {
    sq_batch *const b;
    const sq_fold_opts &o;
    const int32_t *const ref_off, *const ref_pairs;
    const uint8_t *const has_ref;
    const SqFoldSwitches &sw;
    const bool timing;
    struct FoldTimer { double t0; bool on; ~FoldTimer() { if (on) fprintf(stderr, "[sq_fold] total %.3f ms (incl. teardown)\n", (now_s() - t0) * 1e3); } } fold_timer;
    // (the pools -- thousands of small vectors -- are torn down by a helper thread after the fold returns)
    struct PoolsDrop { std::vector<JobPool> *p = nullptr; ~PoolsDrop(); } pools_drop;
    std::vector<JobPool> *pools_p = nullptr;
    std::vector<uint32_t> algos;
    bool dev_tail = false, any_ehn = false, lazy_bits = false, dev_algos = false;
    SqAlgoAsync *pending = nullptr;
    struct PendGuard {                                      // error paths: wait for the side streams, release the arena
        sq_batch *b; SqAlgoAsync *&p;
        ~PendGuard() { if (p) { sq_algos_abandon(b, p); p = nullptr; } }
    } guard{b, pending};
    // the drivers of the greedy part and the jobs each takes
    std::vector<int> greedy_jobs, chain_jobs, pool_jobs_v, tied_jobs;
    std::vector<int> pool_jobs;                              // structure slot of generation 0 -> job (device pools)
    bool use_chain = false, use_pool = false, chain_ties = false, early_tail = false, two_lanes = false;
    // the device pools' log, for the host tail (pool_collect): its last header
    bool pool_logged = false;
    SqPoolHdr pool_hdr{};
    // One launch that covers every chain, the ranking tail on the device, no E / H / N beside it: the tail's kernels are
    // enqueued right behind the round kernel and the host waits ONCE, for the tail's last word -- the chain's own completion
    // (capacity flags, the count of finished structures) is looked at afterwards (the wait between the two was 40-65 us of every
    // fold: a flag's way to the host, then seven launches' way back)
    struct { bool on = false; uint32_t goal = 0; } deferred;
    // a-10 tail per sequence
    std::vector<std::vector<int32_t>> seq_jobs;
    std::vector<double> tail_cost;
    std::vector<char> tailed;
    std::vector<std::atomic<int>> g_left;
    std::vector<char> job_done;
    LoopStats st0, st1;
    double ta = 0, tbegin = 0, tfold0 = 0, tloop = 0, ttail0 = 0;
    bool tails_done = false;
    TailQueue tq;                                            // (last: its worker uses everything above)

    SqFoldRun(sq_batch *b_, const sq_fold_opts &o_, const int32_t *ref_off_, const int32_t *ref_pairs_, const uint8_t *has_ref_)
        : b(b_), o(o_), ref_off(ref_off_), ref_pairs(ref_pairs_), has_ref(has_ref_), sw(b_->sw), timing(b_->sw.timing),
          fold_timer{now_s(), b_->sw.timing} {}
    void mark(const char *what) const { if (timing) fprintf(stderr, "[sq_fold]   +%.3f ms %s\n", (now_s() - tfold0) * 1e3, what); }

    // sq_fold.hip: the stages in the order sq_fold runs them
    void begin();
    int prepare_matrices();
    int algos_begin();
    int choose_drivers();
    void tails_setup();
    int greedy_part();
    int collect_algos();
    int device_tail();
    void host_tails();
    void report(long long cpu_fold0) const;
    // ... and their parts
    void host_pools_init();
    void tail_one(int s);
    void chain_finish(uint32_t q);
    void tail_worker();
    void greedy_loop(SqLane &ln, const std::vector<int> &myjobs, LoopStats &stats);
    int two_lane_loop();
    void take_sets(std::vector<JobSets> &sets, bool edmonds);
    int append_host_lists(int &rt);
    int collect_device_lists();
    // sq_fold_chain.hip
    void chain_fold(LoopStats &stats);
    // sq_fold_pool.hip
    int pool_fold(LoopStats &stats);
    int pool_collect();
};
