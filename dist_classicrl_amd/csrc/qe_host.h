// qe_host.h -- host-side state of libqlearn_engine.so shared by its translation units: the engine / environment /
// rollout-slot structures, small helpers, and the launch entry points whose kernel instantiations are compiled
// in separate files (qe_inst_lane.hip: persistent path, qe_inst_step.hip: step-wise / wide / turnstile paths and
// evaluation), one object per (table dtype, environment), so that the library builds in parallel.  Which of them a
// rollout runs is decided in qe_engine.hip (rollout_path; lane_build for the persistent builds).
#pragma once
#include "../../include/qlearn_engine.h"

#include <time.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "qe_kernels.h"
#include "qe_rollout_lane.h"
#include "qe_rollout_runs.h"
#include "qe_step_turn.h"

using namespace qe;

namespace qe {
struct NStepWin;  // the windows of the n-step rules (qe_rollout_nstep.h)
struct TreeWin;   // the windows of n-step Tree Backup (qe_rollout_tree.h)
template <typename T>
struct TraceSlots;  // the slots of the eligibility traces (qe_rollout_trace.h)
struct DynaModel;   // the learned model and visited list of Dyna-Q (qe_rollout_dyna.h)
struct VisitPlanes; // the visit counts and the bonus plane (qe_rollout_visit.h)
}

// records the text qe_last_error() returns (thread-local) and hands `code` back
__attribute__((visibility("hidden"))) int qe_fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return qe_fail(_e == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_NO_DEVICE,        \
                           "HIP error %d (%s) at %s:%d: %s", (int)_e, hipGetErrorString(_e), \
                           __FILE__, __LINE__, #expr);                                       \
    } while (0)

template <typename U>
struct DevBuf {
    U* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max(n, (size_t)256);
        hipError_t e = hipMalloc((void**)&p, want * sizeof(U));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

template <typename U>
struct PinnedBuf {  // page-locked host staging: async copies without a host-side temporary
    U* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max(n + n / 2, (size_t)1024);
        hipError_t e = hipHostMalloc((void**)&p, want * sizeof(U), hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

constexpr int MAX_TOKEN_ROUNDS = 24;   // chip-wide rounds before the single-workgroup clean-up (wide mode)
constexpr int64_t LISTED_MIN_AGENTS = 16384;  // from here on the rounds walk compacted lists
constexpr int LISTED_MIN_ROUNDS = 6;   // ... and only when at least this many rounds run
constexpr int LISTED_RECOMPACT = 3;    // rounds on the first list before the second compaction
constexpr unsigned LISTED_GRID = 1024; // blocks of a listed round (grid-stride)
constexpr long long HOST_LOG_CAP = 1 << 18;  // episode-log entries of a slot's host result block (persistent path)

// The kernels a rollout runs, chosen once per call by rollout_path (qe_engine.hip).  The values are the path bits of
// qe_rollout_stats::kernel_variant (QE_VARIANT_* below).
enum class RolloutPath : int { Stepwise = 1, Persistent = 2, Wide = 3, Turnstile = 4, Eval = 5 };

// Everything one in-flight rollout owns, so that the next rollout can be enqueued before the results
// of the previous one are read back.
struct RolloutSlot {
    Ctrl* ctrl = nullptr;
    DevBuf<unsigned long long> thr, ep_key, ep_key_packed;
    DevBuf<double> lr;
    DevBuf<float> ep_ret, ep_ret_packed;
    PinnedBuf<unsigned long long> h_thr, h_key;
    PinnedBuf<double> h_lr;
    PinnedBuf<float> h_ret;
    PinnedBuf<Ctrl> h_ctrl;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, sched_ready = nullptr;
    std::vector<hipEvent_t> sample_ev;  // event pairs around sampled dominant-kernel launches
    bool busy = false, timed = true;
    RolloutPath path = RolloutPath::Stepwise;  // of the rollout in flight
    int n_samples = 0;
    int64_t steps = 0, N = 0, launches = 0;
    int64_t variant = 0;  // qe_rollout_stats::kernel_variant of the rollout in flight
    int32_t* trace_host = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int rounds = 4;  // token rounds per step of this call (wide mode)
    unsigned long long turn_epoch = 0;  // turnstile path: record tag of this call's step 0
    int64_t plan_offset = -1;  // >= 0: schedules come from the engine's plan at this offset
    // Host result block (persistent path): page-locked, host-coherent memory the rollout kernel writes
    // itself -- control words, final observations / env state / running returns, episode log -- so that
    // qe_rollout_end neither synchronises a stream nor issues a copy: it spins on hb->seq.
    HostBlock* hb = nullptr;
    int32_t* hb_obs = nullptr;
    uint32_t* hb_aux = nullptr;
    float* hb_acc = nullptr;
    unsigned long long* hb_key = nullptr;
    float* hb_ret = nullptr;
    size_t hb_agents = 0;
    unsigned long long seq = 0;  // value hb->seq takes when the rollout in flight has published
    bool fast = false;           // the rollout in flight publishes through the host block
    bool inline_sched = false;   // ... and carries its schedule values in its kernel arguments
    InlineSched sched{};
    struct qe_env* env = nullptr;  // environment of the rollout in flight
    void release() {
        if (ctrl) (void)hipFree(ctrl);
        ctrl = nullptr;
        for (void* h : {(void*)hb, (void*)hb_obs, (void*)hb_aux, (void*)hb_acc, (void*)hb_key, (void*)hb_ret})
            if (h) (void)hipHostFree(h);
        hb = nullptr; hb_obs = nullptr; hb_aux = nullptr; hb_acc = nullptr; hb_key = nullptr; hb_ret = nullptr;
        hb_agents = 0;
        thr.release(); ep_key.release(); lr.release(); ep_ret.release();
        ep_key_packed.release(); ep_ret_packed.release();
        h_thr.release(); h_key.release(); h_lr.release(); h_ret.release(); h_ctrl.release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (sched_ready) (void)hipEventDestroy(sched_ready);
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        graph_exec = nullptr;
        for (hipEvent_t x : sample_ev) (void)hipEventDestroy(x);
        sample_ev.clear();
        ev0 = ev1 = sched_ready = nullptr;
    }
};

struct qe_replay;

// Population engine (qe_create_population): `runs` independent single-agent runs, run r in table rows r*S .. r*S+S-1
// (k_rollout_runs, qe_population.hip).  runs == 0: an ordinary engine.
struct PopState {
    int64_t runs = 0, S = 0;           // runs, states of one run (the engine's S is runs * S: table I/O sees the whole table)
    DevBuf<RunSched> eps, lr;          // per-run schedule descriptors (their values advance in the kernel)
    DevBuf<double> gamma;
    DevBuf<uint32_t> status;           // per run, per call: 1 = some step found no selectable action
    DevBuf<long long> ep_count;        // per run, per call: episodes ended ...
    DevBuf<float> ep_sum;              // ... and the float32 sequential sum of their returns
    struct EpisodeLog {
        DevBuf<int32_t> seg_cnt, seg_step, off, out_step;  // per-run segments of a launch, compacted copy
        DevBuf<float> seg_ret, out_ret;
        PinnedBuf<int32_t> h_cnt, h_step;
        PinnedBuf<float> h_ret;
        std::vector<int32_t> step;     // episode log of the latest call in (run, episode) order
        std::vector<float> ret;
        void release() {
            seg_cnt.release(); seg_step.release(); off.release(); out_step.release(); seg_ret.release(); out_ret.release();
            h_cnt.release(); h_step.release(); h_ret.release();
        }
    } log;
    // Per-run draw counters: run r's next step is qe_engine::step_ctr + step_off[r].  step_off is only read while
    // off_any (some offset is non-zero: an episode-based evaluation ended the runs after different step counts).
    DevBuf<unsigned long long> step_off;
    bool off_any = false;
    struct EpisodeMode {               // greedy evaluation, episode mode
        DevBuf<long long> used;        // steps each run took in the call ...
        DevBuf<uint8_t> done;          // ... and whether it has reached its episode count
        PinnedBuf<uint8_t> h_done;
        void release() { used.release(); done.release(); h_done.release(); }
    } epi;
    // Update rule of every run (qe_update_rule).  SARSA carries the action chosen for a run's next step from launch to
    // launch and call to call: pending[r], -1 = none (allocated on first use; k_rollout_runs_td, qe_rollout_runs_td.h).
    int rule = QE_RULE_Q_LEARNING;
    DevBuf<int32_t> pending;
    // Double estimator (qe_population_set_double): table B, the engine's dtype, shape and row stride; the engine's own
    // table is A.  NULL: off (k_double_rollout / k_double_evaluate, qe_rollout_double.h).
    void* table_b = nullptr;
    // n-step rules (qe_population_set_n_step): the horizon, 1 = the one-step kernels above.  n > 1: every run's
    // window of at most n - 1 transitions between launches, [slot][runs], oldest first (k_nstep_rollout,
    // qe_rollout_nstep.h); allocated when the horizon is set.
    struct Window {
        int n = 1;
        DevBuf<int32_t> len, s, a;
        DevBuf<float> r;
        void release() {
            len.release(); s.release(); a.release(); r.release();
            n = 1;
        }
    } win;
    // n-step Tree Backup (qe_population_set_tree_backup): the horizon, 1 = the one-step kernel above.  n > 1: every run's
    // window of at most n - 1 entries between launches, [slot][runs], oldest first; an action word carries the entry's
    // greedy flag in its top bit (k_tree_rollout, qe_rollout_tree.h); allocated when the horizon is set.
    struct TreeWindow {
        int n = 1;
        DevBuf<int32_t> len, s, a;
        DevBuf<float> r;
        void release() {
            len.release(); s.release(); a.release(); r.release();
            n = 1;
        }
    } tree;
    // Eligibility traces (qe_population_set_traces): k slots per run, 0 = off (the kernels above).  On: every run's
    // slots between launches, [slot][runs] (e holds k * runs values of the table dtype; a slot whose value is 0 is
    // free), and every run's lambda (k_trace_rollout, qe_rollout_trace.h); allocated when traces are set.
    struct Traces {
        int k = 0, kind = 0;
        DevBuf<int32_t> s, a;
        DevBuf<double> e;
        DevBuf<double> lambda;
        std::vector<double> h_lambda;
        void release() {
            s.release(); a.release(); e.release(); lambda.release();
            h_lambda.clear();
            k = 0;
        }
    } trace;
    // Dyna-Q (qe_population_set_planning): planning updates per step, 0 = off (the kernels above).  On: every run's
    // learned model, one 8-byte entry per table cell ([runs][S * ld]: next_obs | terminated << 31 or 0xFFFFFFFF = unseen,
    // then the reward's bits), the table offsets of its seen cells in order of first observation ([runs][S * A]) and their
    // count (k_dyna_rollout, qe_rollout_dyna.h); allocated when planning is set, kept until it is set to 0.
    struct Model {
        int planning = 0;
        DevBuf<uint2> entry;
        DevBuf<int32_t> visited, count;
        void release() {
            entry.release(); visited.release(); count.release();
            planning = 0;
        }
    } dyna;
    // Visit counts (qe_population_set_visits): off = the kernels above.  On: every run's counts N, uint32, and the
    // derived bonus plane B = bonus(beta, N) in the table dtype, both indexed like the table ([runs * S, ld]; the
    // padding columns of B hold 0), and every run's beta (k_visit_rollout, qe_rollout_visit.h); allocated when counting
    // is set, kept until it is set off.  After every call B == bonus(beta, N) in every cell.
    struct Visits {
        bool on = false, lr = false, any_bonus = false;
        DevBuf<uint32_t> n;
        DevBuf<uint8_t> b;             // runs * S * ld values of the table dtype, as bytes
        DevBuf<double> beta;
        std::vector<double> h_beta;
        void release() {
            n.release(); b.release(); beta.release();
            h_beta.clear();
            on = lr = any_bonus = false;
        }
    } visit;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void release() {
        eps.release(); lr.release(); gamma.release(); status.release(); ep_count.release(); ep_sum.release();
        log.release(); epi.release(); win.release(); tree.release(); trace.release(); dyna.release(); visit.release();
        step_off.release(); pending.release();
        if (table_b) (void)hipFree(table_b);
        table_b = nullptr;
        off_any = false;
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    }
};

struct qe_engine {
    qe_replay* replay = nullptr;  // ring the fused rollouts push their transitions into (qe_replay_attach)
    int device = 0;
    int dtype = QE_F32;
    int64_t S = 0;
    int32_t A = 0, ld = 0, L = 1, lshift = 0;
    double gamma = 0.97;
    uint64_t seed = 0, step_ctr = 0;
    double wall_clock_khz = 100000.0;  // rate of wall_clock64() (s_memrealtime), ticks per millisecond
    uint32_t agent_offset = 0;
    int num_cus = 64;
    int opt_path = 0;  // QE_OPT_ROLLOUT_PATH
    // turnstile path: record tag of the next call's step 0.  The low 32 bits are the tag; 0 = a cleared record, so a
    // call never starts on, reaches or crosses a multiple of 2^32 (turn_setup moves it past and clears the records)
    unsigned long long turn_epoch = 1;
    bool turn_clear = false;            // qe_debug_set_turn_epoch: zero the records before the next turnstile call
    DevBuf<TurnRow> turn_rows;          // turnstile path: [S][2] touchers of a row per step parity, allocated on first use
    bool turn_no_memory = false;        // ... that allocation failed: the path is not taken by this engine
    int turn_blocks_per_cu[5] = {0, 0, 0, 0, 0};  // resident workgroups of k_step_turn per CU, by environment kind (0: not yet asked)
    hipStream_t debug_stream = nullptr;        // qe_debug_occupy_cus
    int opt_graph = 1; // QE_OPT_USE_GRAPH
    int opt_rounds = 0; // QE_OPT_TOKEN_ROUNDS (0 = automatic)
    int auto_rounds = 4; // wide mode: rounds chosen from the previous call's statistics
    int64_t listed_min = LISTED_MIN_AGENTS;  // QE_OPT_LISTED_MIN_AGENTS
    int opt_timing = 1;  // QE_OPT_EVENT_TIMING: bracket rollouts with HIP events (persistent path: off = in-kernel clock only)
    int opt_host_block = 1;  // QE_OPT_HOST_BLOCK: persistent rollouts publish through the host result block
    int opt_turn_forward = 1;  // QE_OPT_TURN_FORWARD: value forwarding in the progress words of the turnstile path
    int opt_stamp_bits = 0;    // QE_OPT_STAMP_HASH_BITS: 0 = automatic, else log2 of the hashed touch-counter slots
    int opt_turn_poll = 0;     // QE_OPT_TURN_POLL: 1 = progress words are polled with sc1 loads, 0 (default) = with returning atomics
    int opt_lane_ordered = 0;  // QE_OPT_LANE_ORDERED_PATH: 0 = automatic, 1 = dataflow kernel, 2 = full build, 3 = sparse build
    int lane_light = -1;       // automatic choice for the next launch (same values; -1: not decided yet; lane_build)
    unsigned long long seq_ctr = 0;
    double host_begin_us = 0.0;  // diagnostics (QE_PRINT_HOST)
    hipStream_t stream = nullptr;
    bool own_stream = true;
    void* q = nullptr;
    unsigned long long* stamps = nullptr;
    Ctrl* ctrl = nullptr;
    uint32_t* tok = nullptr;  // [2][S] wide-mode tokens, allocated on first use, all TOK_INF at rest
    // schedules
    DevBuf<unsigned long long> thr;
    DevBuf<double> lr;
    // batch-API scratch (qe_choose_actions / qe_learn / qe_table_cells)
    DevBuf<int32_t> b_s, b_a, b_n, b_out, b_list;
    DevBuf<float> b_r, b_acc;
    DevBuf<uint8_t> b_term, b_pred;
    DevBuf<uint32_t> b_aux, b_mask, b_bitmap;
    DevBuf<double> b_vals, b_vinc;
    // episode log
    DevBuf<unsigned long long> ep_key;
    DevBuf<float> ep_ret;
    long long ep_cap = 1 << 22;
    std::vector<std::pair<unsigned long long, float>> ep_host, ep_tmp;
    // delta log (caller-owned buffer)
    DeltaEntry* dlog = nullptr;
    long long dlog_cap = 0, dlog_count = 0;
    DevBuf<unsigned> delta_bad;     // [0]: records the apply kernels skipped because their cell lies outside the table
    bool delta_bad_armed = false;   // an apply step ran since the word was last read
    DevBuf<int32_t> trace;
    // replica exchange: ping-pong buffers and digit counts of the radix sort of the remote records (qe_delta_sort.h)
    DevBuf<DeltaEntry> ds_a, ds_b;
    DevBuf<unsigned> ds_hist;
    // schedule plan (qe_schedule_plan): values of a whole training call, consumed by the rollouts
    DevBuf<unsigned long long> plan_thr;
    DevBuf<double> plan_lr;
    PinnedBuf<unsigned long long> h_plan_thr;
    PinnedBuf<double> h_plan_lr;
    int64_t plan_count = 0, plan_cursor = 0;
    unsigned timing_skip = 0;      // launches since the engine was created (timed-launch cadence)
    double ms_per_step_est = 0.0;  // device time per step of the last timed launch
    hipEvent_t plan_ready = nullptr;
    PinnedBuf<uint8_t> h_stage;         // page-locked staging of the unfused batch API (one call at a time)
    DevBuf<uint8_t> warm_scratch;       // 1 MB of device memory for warm_pinned()
    hipStream_t copy_stream = nullptr;  // result read-back beside the compute stream
    RolloutSlot slots[2];               // two rollouts may be in flight (begin k+1 before end k)
    PopState pop;                       // population engine (qe_create_population), else pop.runs == 0
    std::vector<struct qe_env*> envs;   // environments created on this engine (qe_destroy detaches them)
    size_t esize() const { return dtype == QE_F32 ? 4 : 8; }
};

struct qe_replay {
    int device = 0;
    int64_t capacity = 0, position = 0;
    bool full = false;
    DevBuf<int64_t> s, a, n, idx, o_s, o_a, o_n;
    DevBuf<double> r, o_r;
    DevBuf<uint8_t> d, o_d;
    DevBuf<unsigned> bad;
    hipStream_t stream = nullptr;
    qe_engine* attached = nullptr;  // engine whose fused rollouts push into this ring
};

struct qe_env {
    qe_engine* e = nullptr;  // null once the engine has been destroyed: only qe_env_destroy is valid then
    int device = 0;
    qe_env_params p{};
    int64_t N = 0;
    DevBuf<int32_t> s, a, n, list, pend_list;
    DevBuf<float> r, acc;
    DevBuf<uint8_t> term, pred, masks;
    DevBuf<uint32_t> aux, bitmap, adv_bitmap;
    DevBuf<uint32_t> turn_next;            // turnstile path: [2][N][2] overflow-list links, allocated on first use
    DevBuf<double> vinc;
    // QE_ENV_TABLE: outcome records (4 words each), start support ({thr, state} pairs), per-state mask words
    DevBuf<uint32_t> tbl_rec, tbl_start, tbl_mask;
    int32_t tbl_k = 0, tbl_n_start = 0;
    // host copy of (observations, env-internal state, running returns) left by the latest rollout's
    // result block; valid until anything else changes the device state
    const int32_t* mirror_obs = nullptr;
    const uint32_t* mirror_aux = nullptr;
    const float* mirror_acc = nullptr;
};

// States an environment of this engine moves in: the table's rows, or those of one run of a population.
inline int64_t env_states(const qe_engine* e) { return e->pop.runs ? e->pop.S : e->S; }

// Entry points that a population engine does not serve (everything that assumes one table shared by all agents).
inline int not_on_population(const qe_engine* e, const char* what) {
    if (e && e->pop.runs) return qe_fail(QE_ERR_UNSUPPORTED, "%s is not available on a population engine (qe_population_rollout)", what);
    return QE_OK;
}

inline EnvCtx make_envctx(const qe_engine* e, const qe_env_params* p, const uint32_t* maskbits, int masked) {
    EnvCtx ev{};
    ev.S = env_states(e);
    ev.A = e->A;
    ev.n_words = (e->A + 31) / 32;
    ev.maskbits = maskbits;
    if (p) {
        ev.kind = p->kind; ev.masked = p->masked; ev.seed = p->seed; ev.p_term_256 = p->p_term_256;
        ev.side = p->side; ev.episode_len = p->episode_len; ev.agent_offset = p->agent_offset;
    } else {
        ev.kind = -1; ev.masked = masked;
    }
    return ev;
}

// The parameters of a device environment's kernels (make_envctx + the table of a QE_ENV_TABLE environment).
inline EnvCtx make_envctx(const qe_engine* e, const qe_env* env) {
    EnvCtx ev = make_envctx(e, &env->p, nullptr, 0);
    if (env->p.kind == QE_ENV_TABLE) {
        ev.tbl_rec = (const uint4*)env->tbl_rec.p;
        ev.tbl_start = (const uint2*)env->tbl_start.p;
        ev.tbl_mask = env->tbl_mask.p;
        ev.tbl_k = env->tbl_k;
        ev.tbl_n_start = env->tbl_n_start;
    }
    return ev;
}

// Touch counters of the step-wise / wide kernels: one slot per row, or -- tables of more than 2^22 rows, whose counter array
// (16 B per row) would not stay in the Infinity Cache -- 2^21 hashed slots (QE_OPT_STAMP_HASH_BITS forces a size).
inline uint32_t stamp_hash_mask(const qe_engine* e) {
    if (e->opt_stamp_bits == 1) return 0u;  // one slot per row, whatever the size
    int bits = e->opt_stamp_bits ? e->opt_stamp_bits : (e->S > ((int64_t)1 << 22) ? 21 : 0);
    while (bits > 0 && ((int64_t)1 << bits) > e->S) --bits;  // (the array holds S slots)
    return bits > 0 ? (uint32_t)(((int64_t)1 << bits) - 1) : 0u;
}

template <typename T>
Ctx<T> base_ctx(qe_engine* e, int64_t N) {
    Ctx<T> c{};
    c.q = (T*)e->q; c.S = e->S; c.A = e->A; c.ld = e->ld; c.L = e->L; c.lshift = e->lshift;
    c.N = N; c.stamps = e->stamps; c.ctrl = e->ctrl;
    c.stamp_mask = stamp_hash_mask(e);
    c.thr = (const QE_AS4 unsigned long long*)e->thr.p; c.lr = (const QE_AS4 double*)e->lr.p;
    c.seed_lo = (uint32_t)e->seed; c.seed_hi = (uint32_t)(e->seed >> 32);
    c.agent_offset = e->agent_offset; c.step0 = e->step_ctr; c.gamma = e->gamma;
    c.ep_key = e->ep_key.p; c.ep_ret = e->ep_ret.p; c.ep_cap = e->ep_cap;
    return c;
}

template <typename T>
Ctx<T> env_ctx(qe_engine* e, qe_env* env) {
    Ctx<T> c = base_ctx<T>(e, env->N);
    c.s = env->s.p; c.a = env->a.p; c.n = env->n.p; c.r = env->r.p; c.term = env->term.p;
    c.pred = (T*)env->pred.p; c.aux = env->aux.p; c.acc = env->acc.p;
    c.inv_bitmap = env->bitmap.p; c.inv_list = env->list.p; c.vinc = env->vinc.p;
    c.agent_offset = env->p.agent_offset;
    return c;
}

inline unsigned grid_for(int64_t threads, int block) { return (unsigned)((threads + block - 1) / block); }

// Turnstile path (qe_step_turn.h): its workgroups wait for each other inside the launch, so all of them must be
// resident -- TURN_BLOCK threads each.  How many fit a CU is asked of the runtime for the very kernel that will be
// launched (hipOccupancyMaxActiveBlocksPerMultiprocessor, turn_occupancy<T, Env> in qe_inst_step.hip); a quarter of the
// chip is left out of the count, for kernels that share it with the rollout (the collectives of the replica exchange
// run beside the next chunk).  The progress counts are 16 bits.
constexpr int TURN_RESERVE_DIV = 4;   // 1 / TURN_RESERVE_DIV of the CUs is not counted on
inline bool turn_fits(const qe_engine* e, int64_t N, int blocks_per_cu) {
    const int64_t blocks = (N * e->L + TURN_BLOCK - 1) / TURN_BLOCK;
    const int64_t cus = (int64_t)e->num_cus - e->num_cus / TURN_RESERVE_DIV;
    return N <= 60000 && blocks_per_cu > 0 && blocks <= cus * blocks_per_cu && e->ld <= 256;
}
// one launch per rollout on one CU, one agent per lane with its whole row in registers (qe_rollout_lane.h; rollout_path)
inline bool persistent_path(const qe_engine* e, const qe_env* env, int learn) {
    return learn && env->N <= LANE_MAX_AGENTS && e->ld <= 64 && (e->opt_path == 0 || e->opt_path == 2);
}

constexpr int MAX_SAMPLES = 256;

constexpr int GRAPH_STEPS = 50;  // vector steps per captured graph (step-wise / wide paths)

// ---- launch entry points, instantiated per (table dtype, environment) in qe_inst_lane.hip / qe_inst_step.hip ----
// qe_rollout_stats::kernel_variant: which kernel build a rollout ran (tests assert the build they mean to cover).
//   bits 0-3   path: 1 step-wise (k_step_fast + k_step_slow), 2 persistent (k_rollout_lane), 3 wide (token rounds),
//              4 turnstile (k_step_turn), 5 greedy evaluation (k_eval)
//   persistent path only: bits 4-5 LEAN (0 generic, 1 plain training rollout, 2 + delta log), bit 6 HELP (draw-producing
//   wavefronts), bit 7 FULL (every lane an agent), bit 8 SEQ (built without the general ordered path), bit 9 the
//   512-agent build, bit 10 the dataflow kernel (k_rollout_df), bits 12-19 NV (16-byte loads per fp32 row), bit 20
//   masked environment; path 6 = population (k_rollout_runs) and path 7 = population greedy evaluation
//   (k_evaluate_runs), both with the same NV and masked bits; path 8 = population with an on-policy update rule
//   (k_rollout_runs_td): those NV and masked bits, and the rule (qe_update_rule) in bits 4-5; path 9 = population with
//   the double estimator (k_double_rollout) and path 10 = its greedy evaluation (k_double_evaluate), NV and masked bits;
//   path 11 = population with an n-step on-policy rule (k_nstep_rollout): the rule in bits 4-5, NV and masked as path 6,
//   and n in bits 24-28, which no other path uses; path 12 = population with eligibility traces (k_trace_rollout): the
//   rule in bits 4-5 (0 = Watkins's Q(lambda), 1 = SARSA(lambda)), NV and masked as path 6, K in bits 24-29 and the trace
//   kind in bit 30, which no other field of that path uses; path 13 = population with Dyna-Q (k_dyna_rollout): NV and
//   masked as path 6, and the planning updates per step in bits 24-30; path 14 = population with visit counts
//   (k_visit_rollout): NV and masked as path 6, visit_lr in bit 4 and "some beta > 0" in bit 5; path 15 = population with
//   n-step Tree Backup (k_tree_rollout): NV and masked as path 6, and n in bits 24-28
constexpr int64_t QE_VARIANT_DATAFLOW = 1 << 10;  // persistent path: k_rollout_df (qe_rollout_df.h)
constexpr int64_t QE_VARIANT_STEPWISE = (int64_t)RolloutPath::Stepwise, QE_VARIANT_PERSISTENT = (int64_t)RolloutPath::Persistent,
                  QE_VARIANT_WIDE = (int64_t)RolloutPath::Wide, QE_VARIANT_TURNSTILE = (int64_t)RolloutPath::Turnstile,
                  QE_VARIANT_EVAL = (int64_t)RolloutPath::Eval;
constexpr int64_t QE_VARIANT_RUNS = 6;  // population path (k_rollout_runs): bits 12-19 NV, bit 20 masked, as persistent
constexpr int64_t QE_VARIANT_RUNS_EVAL = 7;  // population greedy evaluation (k_evaluate_runs): the same NV and masked bits
constexpr int64_t QE_VARIANT_RUNS_TD = 8;  // population, SARSA / Expected SARSA (k_rollout_runs_td): + the rule in bits 4-5
constexpr int64_t QE_VARIANT_RUNS_DOUBLE = 9;        // population, Double Q-learning (k_double_rollout): NV and masked bits
constexpr int64_t QE_VARIANT_RUNS_DOUBLE_EVAL = 10;  // ... and its greedy evaluation (k_double_evaluate)
constexpr int64_t QE_VARIANT_RUNS_NSTEP = 11;  // population, n-step SARSA / Expected SARSA (k_nstep_rollout): as path 8, + n in bits 24-28
constexpr int64_t QE_VARIANT_RUNS_DYNA = 13;   // population, Dyna-Q (k_dyna_rollout): NV and masked bits, + planning updates in bits 24-30
constexpr int64_t QE_VARIANT_RUNS_TRACE = 12;  // population, SARSA(lambda) / Watkins's Q(lambda) (k_trace_rollout): + K in bits 24-29, kind in bit 30
constexpr int64_t QE_VARIANT_RUNS_VISIT = 14;  // population, visit counts (k_visit_rollout): NV and masked bits, + visit_lr in bit 4, bonus in bit 5
constexpr int64_t QE_VARIANT_RUNS_TREE = 15;   // population, n-step Tree Backup (k_tree_rollout): NV and masked bits, + n in bits 24-28
// build: 1 dataflow, 2 full, 3 sparse (lane_build in qe_engine.hip; the generic builds take what these do not)
template <typename T, class Env>
int launch_persistent(qe_engine* e, qe_env* env, RolloutSlot& sl, const Ctx<T>& c, const EnvCtx& ev, int64_t steps, int mode,
                      int build);
template <typename T, class Env>
int launch_stepwise(qe_engine* e, RolloutSlot& sl, const Ctx<T>& c, const EnvCtx& ev, int64_t steps, bool turn);
template <typename T, class Env>
int launch_eval(qe_engine* e, RolloutSlot& sl, const Ctx<T>& c, const EnvCtx& ev, int64_t steps);
// What every launch of a population kernel takes: the stream, the runs and the environment, the row stride and mask
// build that pick the instantiation, and the steps of this launch.
template <typename T>
struct RunsLaunch {
    hipStream_t stream;
    RunsCtx<T> c;
    EnvCtx ev;
    int ld;
    bool masked;
    long long steps;
};

// The (NV, masked) build of a population kernel for a row stride (the qe_inst_runs*.hip units): go(integral_constant<int, NV>, bool_constant<masked>).
template <class Env, class F>
inline int64_t runs_by_build(int ld, bool masked, F go) {
    using Yes = std::true_type;
    using No = std::false_type;
    if constexpr (std::is_same<Env, HashEnv>::value || std::is_same<Env, TableEnv>::value) {  // any A, masked or not
        auto by_mask = [&](auto nv) { return masked ? go(nv, Yes{}) : go(nv, No{}); };
        switch (ld) {  // a power of two (row_stride), at most 64
            case 4: return by_mask(std::integral_constant<int, 1>{});
            case 8: return by_mask(std::integral_constant<int, 2>{});
            case 16: return by_mask(std::integral_constant<int, 4>{});
            case 32: return by_mask(std::integral_constant<int, 8>{});
            default: return by_mask(std::integral_constant<int, 16>{});
        }
    } else if constexpr (std::is_same<Env, TttEnv>::value) {
        return go(std::integral_constant<int, 4>{}, Yes{});  // A = 9 -> row stride 16
    } else {
        return go(std::integral_constant<int, 1>{}, No{});  // GridLake (A = 4) and the bandit (A = 2)
    }
}

// One launch of the population kernel of `path` (QE_VARIANT_RUNS*): go(nv, mk, grid, block) launches its (NV, masked)
// build and returns the variant bits of its own (0: none); returns the launch's kernel_variant.
template <class Env, typename T, class F>
inline int64_t launch_runs_build(const RunsLaunch<T>& l, int64_t path, F go) {
    const dim3 grid(grid_for(l.c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(l.ld, l.masked, [&](auto nv, auto mk) -> int64_t {
        return path | go(nv, mk, grid, block) | ((int64_t)decltype(nv)::value << 12) | ((int64_t)decltype(mk)::value << 20);
    });
}

// population path: one launch of l.steps steps of every run (qe_inst_runs.hip); returns its kernel_variant
template <typename T, class Env>
int64_t launch_runs(const RunsLaunch<T>& l);
// ... with the update rule `rule` (QE_RULE_SARSA: `pending` holds every run's pending action; QE_RULE_EXPECTED_SARSA),
// qe_inst_runs_td.hip; a build the rule is not compiled for returns QE_ERR_UNSUPPORTED (see runs_td_supported)
template <typename T, class Env>
int64_t launch_runs_td(const RunsLaunch<T>& l, int rule, int32_t* pending);
// ... with the n-step form of that rule and the runs' windows `w` (qe_inst_runs_nstep.hip)
template <typename T, class Env>
int64_t launch_nstep_runs(const RunsLaunch<T>& l, int rule, int32_t* pending, const NStepWin& w);
// ... with n-step Tree Backup, Q-learning's n-step form, and the runs' windows `w` (qe_inst_runs_tree.hip)
template <typename T, class Env>
int64_t launch_tree_runs(const RunsLaunch<T>& l, const TreeWin& w);
// ... with eligibility traces: `rule` is QE_RULE_Q_LEARNING or QE_RULE_SARSA, `w` the runs' slots (qe_inst_runs_trace.hip)
template <typename T, class Env>
int64_t launch_trace_runs(const RunsLaunch<T>& l, int rule, int32_t* pending, const TraceSlots<T>& w);
// ... with Dyna-Q: Q-learning's step, then w.n planning updates from the runs' learned models (qe_inst_runs_dyna.hip)
template <typename T, class Env>
int64_t launch_dyna_runs(const RunsLaunch<T>& l, const DynaModel& w);
// ... with visit counts: Q-learning's step with the bonus plane on the pick and, optionally, the 1/N rate
// (qe_inst_runs_visit.hip); `any_bonus`: some run's beta is above 0 (bit 5 of the variant)
template <typename T, class Env>
int64_t launch_visit_runs(const RunsLaunch<T>& l, const VisitPlanes& w, bool any_bonus);
// The (table dtype, NV) builds of k_visit_rollout that are compiled: the kernel holds two rows, and a build ships only
// if it fits the register file without scratch (DESIGN 4.3c lists the others; qe_population_set_visits refuses them).
constexpr bool visit_supported(bool f32, int nv) { return true; }
// ... and one launch of its greedy evaluation (episodes == 0: step mode; else used / done per run, see k_evaluate_runs)
template <typename T, class Env>
int64_t launch_evaluate_runs(const RunsLaunch<T>& l, long long episodes, long long* used, uint8_t* done);
// ... and the double estimator (qe_inst_runs_double.hip): training and greedy evaluation over the tables l.c.q and table_b
template <typename T, class Env>
int64_t launch_double_runs(const RunsLaunch<T>& l, T* table_b);
template <typename T, class Env>
int64_t launch_double_evaluate(const RunsLaunch<T>& l, long long episodes, long long* used, uint8_t* done, const T* table_b);
// resident workgroups per CU of the k_step_turn build this engine would launch (occupancy query), 0 on failure
template <typename T, class Env>
int turn_occupancy(const qe_engine* e);
