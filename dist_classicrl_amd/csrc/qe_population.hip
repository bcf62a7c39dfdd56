// qe_population.hip -- host side of the population path (include/qlearn_engine.h, "population"): M independent
// single-agent runs in one [M * S, ld] table.  Which kernel trains them is launch_training's to say, what each method
// carries between launches and calls is PopState's (qe_host.h); the two calls share one skeleton (PopCall), which cuts
// them into launches, compacts the per-run episode-log segments and reports.  The per-run draw counters live here too.
#include "qe_host.h"
#include "qe_rollout_dyna.h"
#include "qe_rollout_nstep.h"
#include "qe_rollout_trace.h"
#include "qe_rollout_tree.h"
#include "qe_rollout_visit.h"

namespace {

// One launch covers at most this many env-steps (runs x steps): well under a second at every shape the population is
// measured at (tools/population_rate.py), so a launch never holds the device for long.
constexpr long long RUNS_STEP_BUDGET = 1ll << 25;
// Episode-log entries of one launch: every run gets a segment of one entry per step of the launch (at most one
// episode ends per step), so the launches of a logged call are at most RUNS_LOG_BUDGET / runs steps long.
constexpr long long RUNS_LOG_BUDGET = 1ll << 23;

// Exclusive prefix sum of the runs' segment counts of a launch (one workgroup; off[M] = total).
__global__ __launch_bounds__(1024) void k_runs_log_scan(const int32_t* cnt, int64_t M, int32_t* off) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (M + 1023) / 1024;
    const int64_t b = std::min<int64_t>(M, tid * per), e = std::min<int64_t>(M, b + per);
    long long mine = 0;
    for (int64_t k = b; k < e; ++k) mine += cnt[k];
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long run = part[tid] - mine;
    for (int64_t k = b; k < e; ++k) {
        off[k] = (int32_t)run;
        run += cnt[k];
    }
    if (tid == 1023) off[M] = (int32_t)part[1023];
}

// The real entries of every run's segment, packed in run order.
__global__ __launch_bounds__(256) void k_runs_log_pack(const int32_t* cnt, const int32_t* off, const int32_t* seg_step,
                                                       const float* seg_ret, long long seg_len, int64_t M, int32_t* out_step,
                                                       float* out_ret) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const int32_t n = cnt[r], o = off[r];
    for (int32_t k = 0; k < n; ++k) {
        out_step[o + k] = seg_step[r * seg_len + k];
        out_ret[o + k] = seg_ret[r * seg_len + k];
    }
}

template <class F>
int64_t by_env(int kind, F f) {
    switch (kind) {
        case QE_ENV_HASH: return f(HashEnv{});
        case QE_ENV_GRID: return f(GridEnv{});
        case QE_ENV_BANDIT: return f(BanditEnv{});
        case QE_ENV_TICTACTOE: return f(TttEnv{});
        case QE_ENV_TABLE: return f(TableEnv{});
    }
    return -1;
}

int need_population(const qe_engine* e) {
    if (!e) return qe_fail(QE_ERR_INVALID, "engine is NULL");
    if (!e->pop.runs) return qe_fail(QE_ERR_INVALID, "not a population engine (qe_create_population)");
    return QE_OK;
}

// Steps per launch of a call of `steps` steps of M runs (the budgets above).  `planning`: table updates a step makes
// beside its own (Dyna-Q), which share the step budget -- a launch holds the device no longer with them than without.
long long launch_len(int64_t M, int64_t steps, bool log, int planning = 0) {
    long long per_launch = std::max<long long>(1, RUNS_STEP_BUDGET / M / (1 + planning));
    if (log) per_launch = std::min<long long>(per_launch, std::max<long long>(1, RUNS_LOG_BUDGET / M));
    if (steps > 0) per_launch = std::min<long long>(per_launch, steps);
    return per_launch;
}

int log_reserve(PopState::EpisodeLog& G, size_t m, long long per_launch) {
    const size_t seg = m * (size_t)per_launch;
    HIP_TRY(G.seg_cnt.ensure(m)); HIP_TRY(G.off.ensure(m + 1)); HIP_TRY(G.seg_step.ensure(seg)); HIP_TRY(G.seg_ret.ensure(seg));
    HIP_TRY(G.out_step.ensure(seg)); HIP_TRY(G.out_ret.ensure(seg)); HIP_TRY(G.h_cnt.ensure(m + 1));
    return QE_OK;
}

// Episode log of a call, launch-major: per launch, each run's entries in order.
struct CallLog {
    std::vector<int32_t> cnt, step;
    std::vector<float> ret;
};

// Compacts the segments the launch of `k` steps has just written and appends them to `L` (synchronises the stream).
int log_launch(qe_engine* e, long long k, CallLog& L, int64_t& launches) {
    PopState::EpisodeLog& G = e->pop.log;
    const int64_t M = e->pop.runs;
    const size_t m = (size_t)M;
    hipLaunchKernelGGL(k_runs_log_scan, dim3(1), dim3(1024), 0, e->stream, (const int32_t*)G.seg_cnt.p, M, G.off.p);
    hipLaunchKernelGGL(k_runs_log_pack, dim3(grid_for(M, 256)), dim3(256), 0, e->stream, (const int32_t*)G.seg_cnt.p,
                       (const int32_t*)G.off.p, (const int32_t*)G.seg_step.p, (const float*)G.seg_ret.p, k, M,
                       G.out_step.p, G.out_ret.p);
    launches += 2;
    HIP_TRY(hipMemcpyAsync(G.h_cnt.p, G.seg_cnt.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(G.h_cnt.p + m, G.off.p + m, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t total = (size_t)G.h_cnt.p[m];
    L.cnt.insert(L.cnt.end(), G.h_cnt.p, G.h_cnt.p + m);
    if (total) {
        HIP_TRY(G.h_step.ensure(total)); HIP_TRY(G.h_ret.ensure(total));
        HIP_TRY(hipMemcpyAsync(G.h_step.p, G.out_step.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(G.h_ret.p, G.out_ret.p, total * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        L.step.insert(L.step.end(), G.h_step.p, G.h_step.p + total);
        L.ret.insert(L.ret.end(), G.h_ret.p, G.h_ret.p + total);
    }
    return QE_OK;
}

// Launch-major -> (run, episode) order, into G.step / G.ret (qe_population_log).
void log_finish(PopState::EpisodeLog& G, size_t m, const CallLog& L, const std::vector<long long>& counts) {
    std::vector<size_t> at(m + 1, 0);
    for (size_t r = 0; r < m; ++r) at[r + 1] = at[r] + (size_t)counts[r];
    G.step.resize(L.step.size());
    G.ret.resize(L.ret.size());
    size_t src = 0;
    for (size_t l = 0; l < L.cnt.size() / std::max<size_t>(m, 1); ++l)
        for (size_t r = 0; r < m; ++r)
            for (int32_t j = 0; j < L.cnt[l * m + r]; ++j, ++src) {
                G.step[at[r]] = L.step[src];
                G.ret[at[r]] = L.ret[src];
                ++at[r];
            }
}

// QE_ERR_INDEX naming the (first eight) runs with bit 0 of their status set, else QE_OK.
int fail_empty(const std::vector<uint32_t>& st) {
    for (size_t r = 0; r < st.size(); ++r)
        if (st[r] & 1u) {
            std::string runs;
            int named = 0;
            for (size_t q = r; q < st.size() && named < 8; ++q)
                if (st[q] & 1u) { runs += (named++ ? ", " : "") + std::to_string(q); }
            return qe_fail(QE_ERR_INDEX, "Cannot choose from an empty sequence (runs %s%s)", runs.c_str(), named == 8 ? ", ..." : "");
        }
    return QE_OK;
}

// Every run's draw counter: step_ctr + its offset.
int get_counters(qe_engine* e, uint64_t* out) {
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    std::vector<unsigned long long> off(m, 0ull);
    if (P.off_any) {
        HIP_TRY(hipMemcpyAsync(off.data(), P.step_off.p, m * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    for (size_t r = 0; r < m; ++r) out[r] = e->step_ctr + off[r];
    return QE_OK;
}

// Run r's counter := in[r]: step_ctr = in[0] and offsets relative to it (uint64 arithmetic wraps both ways); the kernels
// read the offsets only if one of them is non-zero.
int set_counters(qe_engine* e, const uint64_t* in) {
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    std::vector<unsigned long long> off(m);
    bool any = false;
    for (size_t r = 0; r < m; ++r) {
        off[r] = (unsigned long long)(in[r] - in[0]);
        any |= off[r] != 0;
    }
    if (any) {
        HIP_TRY(P.step_off.ensure(m));
        HIP_TRY(hipMemcpyAsync(P.step_off.p, off.data(), m * sizeof(unsigned long long), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    e->step_ctr = in[0];
    P.off_any = any;
    return QE_OK;
}

// SARSA's pending actions: allocated on first use, every run without one.
int pending_reserve(qe_engine* e) {
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    if (P.pending.p) return QE_OK;
    HIP_TRY(P.pending.ensure(m));
    HIP_TRY(hipMemsetAsync(P.pending.p, 0xFF, m * sizeof(int32_t), e->stream));  // -1
    return QE_OK;
}

// The n-step rules' windows, [slot][runs] with n - 1 slots: allocated for the horizon `n`, every window empty.
int window_reserve(qe_engine* e, int n) {
    PopState::Window& W = e->pop.win;
    const size_t m = (size_t)e->pop.runs, cells = m * (size_t)(n - 1);
    HIP_TRY(W.len.ensure(m)); HIP_TRY(W.s.ensure(cells)); HIP_TRY(W.a.ensure(cells)); HIP_TRY(W.r.ensure(cells));
    HIP_TRY(hipMemsetAsync(W.len.p, 0, m * sizeof(int32_t), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

// Tree Backup's windows, [slot][runs] with n - 1 slots: allocated for the horizon `n`, every window empty.
int tree_reserve(qe_engine* e, int n) {
    PopState::TreeWindow& W = e->pop.tree;
    const size_t m = (size_t)e->pop.runs, cells = m * (size_t)(n - 1);
    HIP_TRY(W.len.ensure(m)); HIP_TRY(W.s.ensure(cells)); HIP_TRY(W.a.ensure(cells)); HIP_TRY(W.r.ensure(cells));
    HIP_TRY(hipMemsetAsync(W.len.p, 0, m * sizeof(int32_t), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

// What every other mode setter answers while Tree Backup is on.
int tree_refuse(const qe_engine* e, const char* what) {
    return qe_fail(QE_ERR_UNSUPPORTED, "%s: tree_backup = %d is on, and Tree Backup is built for the plain Q-learning run (qe_population_set_tree_backup)",
                   what, e->pop.tree.n);
}

// T(gamma * lambda), the decay factor of a run's traces, as a double; `f32`: T is float.
double trace_decay_of(double gamma, double lambda, bool f32) {
    const double d = gamma * lambda;
    return f32 ? (double)(float)d : d;
}

// QE_ERR_UNSUPPORTED naming the first run whose decay factor lies outside [0, 1] (a NaN included), else QE_OK.
int check_trace_decay(const qe_engine* e, const double* gamma, const double* lambda) {
    for (size_t r = 0; r < (size_t)e->pop.runs; ++r) {
        const double d = trace_decay_of(gamma[r], lambda[r], e->dtype == QE_F32);
        if (!(d >= 0.0 && d <= 1.0))
            return qe_fail(QE_ERR_UNSUPPORTED, "run %lld: the trace decay factor gamma * lambda = %g * %g is outside [0, 1]",
                           (long long)r, gamma[r], lambda[r]);
    }
    return QE_OK;
}

// Every trace slot of every run free.
int traces_clear(qe_engine* e) {
    PopState::Traces& X = e->pop.trace;
    const size_t cells = (size_t)e->pop.runs * (size_t)X.k;
    HIP_TRY(hipMemsetAsync(X.s.p, 0, cells * sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(X.a.p, 0, cells * sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(X.e.p, 0, cells * sizeof(double), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

// Dyna-Q: every run's model unseen, its list empty.
int model_clear(qe_engine* e) {
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    HIP_TRY(hipMemsetAsync(P.dyna.entry.p, 0xFF, m * (size_t)P.S * (size_t)e->ld * sizeof(uint2), e->stream));  // DYNA_UNSEEN
    HIP_TRY(hipMemsetAsync(P.dyna.count.p, 0, m * sizeof(int32_t), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

// Visit counts: the bonus plane rewritten from the counts and the runs' betas (k_visit_fill), so that B == bonus(beta, N)
// in every cell; synchronises the stream.
int visits_fill(qe_engine* e) {
    PopState& P = e->pop;
    const int64_t per_run = P.S * (int64_t)e->ld, total = P.runs * per_run;
    const dim3 grid(grid_for(total, 256)), block(256);
    if (e->dtype == QE_F32)
        hipLaunchKernelGGL(k_visit_fill<float>, grid, block, 0, e->stream, (const uint32_t*)P.visit.n.p, (float*)P.visit.b.p,
                           (const double*)P.visit.beta.p, per_run, total, (int)e->A, (int)e->ld);
    else
        hipLaunchKernelGGL(k_visit_fill<double>, grid, block, 0, e->stream, (const uint32_t*)P.visit.n.p, (double*)P.visit.b.p,
                           (const double*)P.visit.beta.p, per_run, total, (int)e->A, (int)e->ld);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

// What every other mode setter answers while visit counts are on.
int visits_refuse(const char* what) {
    return qe_fail(QE_ERR_UNSUPPORTED, "%s: visit counts are on, and they are built for the plain one-step Q-learning run (qe_population_set_visits)", what);
}

// The double estimator's table entry points: the qe_table_* call `f` with table B standing in for the engine's table.
template <class F>
int on_table_b(qe_engine* e, F f) {
    if (int rc = need_population(e)) return rc;
    if (!e->pop.table_b) return qe_fail(QE_ERR_INVALID, "the double estimator is off (qe_population_set_double)");
    void* const a = e->q;
    e->q = e->pop.table_b;
    const int rc = f();
    e->q = a;
    return rc;
}

// Slot-major state (windows, trace slots) is [slot][runs] on the device and [runs][slot] at the ABI.  These copy the
// slots `keep(r, i)` names from one order to the other; the others become 0.  A NULL `abi` is not written.
template <typename U, typename V, class Keep>
void slots_to_abi(const U* dev, V* abi, size_t m, size_t w, Keep keep) {
    for (size_t r = 0; abi && r < m; ++r)
        for (size_t i = 0; i < w; ++i) abi[r * w + i] = keep(r, i) ? (V)dev[i * m + r] : V{};
}
template <typename U, typename V, class Keep>
void slots_to_device(const V* abi, U* dev, size_t m, size_t w, Keep keep) {
    for (size_t r = 0; r < m; ++r)
        for (size_t i = 0; i < w; ++i) dev[i * m + r] = keep(r, i) ? (U)abi[r * w + i] : U{};
}

// The training launch of a population: the kernel of the first method that is on, in this order.
template <typename T, class Env>
int64_t launch_training(const qe_engine* e, const RunsLaunch<T>& l) {
    const PopState& P = e->pop;
    if (P.visit.on)
        return launch_visit_runs<T, Env>(l, VisitPlanes{P.visit.n.p, P.visit.b.p, P.visit.beta.p, P.visit.lr ? 1 : 0}, P.visit.any_bonus);
    if (P.table_b) return launch_double_runs<T, Env>(l, (T*)P.table_b);
    if (P.dyna.planning)
        return launch_dyna_runs<T, Env>(l, DynaModel{P.dyna.planning, P.dyna.entry.p, P.dyna.visited.p, P.dyna.count.p, P.S * (int64_t)e->A});
    if (P.trace.k)
        return launch_trace_runs<T, Env>(l, P.rule, P.pending.p,
                                         TraceSlots<T>{P.trace.k, P.trace.kind, P.trace.s.p, P.trace.a.p, (T*)P.trace.e.p, P.trace.lambda.p});
    if (P.tree.n > 1) return launch_tree_runs<T, Env>(l, TreeWin{P.tree.n, P.tree.len.p, P.tree.s.p, P.tree.a.p, P.tree.r.p});
    if (P.win.n > 1) return launch_nstep_runs<T, Env>(l, P.rule, P.pending.p, NStepWin{P.win.n, P.win.len.p, P.win.s.p, P.win.a.p, P.win.r.p});
    if (P.rule != QE_RULE_Q_LEARNING) return launch_runs_td<T, Env>(l, P.rule, P.pending.p);
    return launch_runs<T, Env>(l);
}

// A call of qe_population_rollout / qe_population_evaluate from call_begin to call_end.
struct PopCall {
    qe_engine* e;
    qe_env* env;
    int64_t steps;
    bool log;
    int nan_select;   // the caller's selection rule (rollout_ctx)
    int64_t variant;  // kernel_variant of the latest launch; of a call without one, the caller's
    long long per_launch = 0;
    EnvCtx ev{};
    CallLog L;
    int64_t launches = 0;
    std::vector<uint32_t> st;  // every run's status, once call_end has copied it back
};

// What both calls refuse first.  The log of the previous call is gone once the engine is known to be a population.
int call_check(qe_engine* e, const qe_env* env, int64_t steps, qe_rollout_stats* stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = need_population(e)) return rc;
    e->pop.log.step.clear();
    e->pop.log.ret.clear();
    if (!env || env->e != e) return qe_fail(QE_ERR_INVALID, "engine/env mismatch");
    if (steps < 0) return qe_fail(QE_ERR_INVALID, "steps must be >= 0");
    return QE_OK;
}

// The entry of a call that has passed its checks: sizes the launches (`planning`: see launch_len), reserves the log
// buffers and, through `own_buffers`, what the caller keeps per run, zeroes the accumulators and starts the clock.
template <class F>
int call_begin(PopCall& c, int planning, F own_buffers) {
    qe_engine* e = c.e;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    if (e->ld > 64) return qe_fail(QE_ERR_UNSUPPORTED, "a population holds rows of at most 64 actions");
    HIP_TRY(hipSetDevice(e->device));
    c.per_launch = launch_len(P.runs, c.steps, c.log, planning);
    if (c.log)
        if (int rc = log_reserve(P.log, m, c.per_launch)) return rc;
    if (int rc = own_buffers()) return rc;
    c.env->mirror_obs = nullptr; c.env->mirror_aux = nullptr; c.env->mirror_acc = nullptr;  // the device state moves on
    HIP_TRY(hipMemsetAsync(P.status.p, 0, m * sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync(P.ep_count.p, 0, m * sizeof(long long), e->stream));
    HIP_TRY(hipMemsetAsync(P.ep_sum.p, 0, m * sizeof(float), e->stream));
    c.ev = make_envctx(e, c.env);
    HIP_TRY(hipEventRecord(P.ev0, e->stream));
    return QE_OK;
}

// One launch of `k` steps from step `t` of the call: `own(l, Env{})` completes l.c and launches, the rest is bookkeeping.
template <class F>
int call_launch(PopCall& c, long long t, long long k, F own) {
    qe_engine* e = c.e;
    qe_env* env = c.env;
    PopState& P = e->pop;
    const int64_t v = by_env(env->p.kind, [&](auto tag) -> int64_t {
        auto go = [&](auto tt) -> int64_t {
            using T = decltype(tt);
            RunsLaunch<T> l{e->stream, {}, c.ev, e->ld, env->p.masked != 0, k};
            RunsCtx<T>& x = l.c;
            x.q = (T*)e->q; x.S = P.S; x.M = P.runs;
            x.obs = env->n.p; x.aux = env->aux.p; x.acc = env->acc.p;
            x.status = P.status.p; x.ep_count = P.ep_count.p; x.ep_sum = P.ep_sum.p;
            if (c.log) { x.seg_cnt = P.log.seg_cnt.p; x.seg_step = P.log.seg_step.p; x.seg_ret = P.log.seg_ret.p; x.seg_len = k; }
            x.seed_lo = (uint32_t)e->seed; x.seed_hi = (uint32_t)(e->seed >> 32);
            x.nan_select = c.nan_select;
            x.step0 = e->step_ctr + (unsigned long long)t; x.t_call = t;
            x.step_off = P.off_any ? P.step_off.p : nullptr;
            return own(l, tag);
        };
        return e->dtype == QE_F32 ? go(float{}) : go(double{});
    });
    if (v < 0) return qe_fail(QE_ERR_INVALID, "unknown env kind %d", (int)env->p.kind);
    c.variant = v;
    ++c.launches;
    HIP_TRY(hipGetLastError());
    if (c.log)
        if (int rc = log_launch(e, k, c.L, c.launches)) return rc;
    return QE_OK;
}

// The exit of a call: stops the clock and copies back (`own_copies` enqueues the caller's beside the common ones); then
// `settle(env_steps)` advances the draw counters and does what else the caller derives per run; then the log in
// (run, episode) order, the statistics, and the refusal that names the runs without a selectable action.  Returns the
// episodes ended.
template <class Copies, class Settle>
int64_t call_end(PopCall& c, qe_rollout_stats* stats, int64_t* ep_count, float* ep_sum, uint32_t* status, Copies own_copies,
                 Settle settle) {
    qe_engine* e = c.e;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    HIP_TRY(hipEventRecord(P.ev1, e->stream));
    std::vector<long long> counts(m);
    c.st.resize(m);
    HIP_TRY(hipMemcpyAsync(counts.data(), P.ep_count.p, m * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(c.st.data(), P.status.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    if (ep_sum) HIP_TRY(hipMemcpyAsync(ep_sum, P.ep_sum.p, m * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (int rc = own_copies()) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    long long total = 0, env_steps = 0;
    if (int rc = settle(env_steps)) return rc;
    for (size_t r = 0; r < m; ++r) {
        if (ep_count) ep_count[r] = counts[r];
        total += counts[r];
    }
    if (status) memcpy(status, c.st.data(), m * sizeof(uint32_t));
    if (c.log) log_finish(P.log, m, c.L, counts);
    if (stats) {
        float ms = 0.0f;
        if (c.launches) HIP_TRY(hipEventElapsedTime(&ms, P.ev0, P.ev1));
        stats->kernel_ms = ms; stats->launches = c.launches; stats->episodes = total;
        stats->dominant_ms = ms; stats->dominant_launches = c.launches; stats->dominant_env_steps = env_steps;
        stats->kernel_variant = c.variant;
    }
    if (int rc = fail_empty(c.st)) return rc;
    return total;
}

}  // namespace

extern "C" {

int qe_create_population(qe_engine** out, int64_t runs, int64_t S, int32_t A, uint64_t seed, int32_t dtype, int32_t device) {
    if (!out) return qe_fail(QE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (runs <= 0 || S <= 0 || A <= 0) return qe_fail(QE_ERR_INVALID, "runs, state_size and action_size must be positive");
    if (runs > 0x7FFFFFFF) return qe_fail(QE_ERR_INVALID, "at most 2^31 - 1 runs");
    if (A > 64) return qe_fail(QE_ERR_UNSUPPORTED, "a population holds rows of at most 64 actions (have %d)", (int)A);
    if ((double)runs * (double)S >= 4294967296.0) return qe_fail(QE_ERR_UNSUPPORTED, "runs * state_size must be < 2^32 rows");
    qe_engine* e = nullptr;
    if (int rc = qe_create(&e, runs * S, A, 0.0, seed, dtype, device)) return rc;
    // (the touch counters serve the paths that order agents sharing a row: not this one)
    (void)hipFree(e->stamps);
    e->stamps = nullptr;
    PopState& P = e->pop;
    P.runs = runs;
    P.S = S;
    const size_t m = (size_t)runs;
    hipError_t err = hipSuccess;
    auto ok = [&](hipError_t step) { return (err = step) == hipSuccess; };
    if (ok(P.eps.ensure(m)) && ok(P.lr.ensure(m)) && ok(P.gamma.ensure(m)) && ok(P.status.ensure(m)) && ok(P.ep_count.ensure(m)) &&
        ok(P.ep_sum.ensure(m)) && ok(hipMemsetAsync(P.eps.p, 0, m * sizeof(RunSched), e->stream)) &&  // constant 0
        ok(hipMemsetAsync(P.lr.p, 0, m * sizeof(RunSched), e->stream)) && ok(hipMemsetAsync(P.gamma.p, 0, m * sizeof(double), e->stream)) &&
        ok(hipEventCreate(&P.ev0)) && ok(hipEventCreate(&P.ev1)) && ok(hipStreamSynchronize(e->stream))) {
        *out = e;
        return QE_OK;
    }
    const int code = qe_fail(err == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_NO_DEVICE, "population allocation failed: %s",
                             hipGetErrorString(err));
    qe_destroy(e);
    return code;
}

int64_t qe_population_runs(qe_engine* e) { return e ? e->pop.runs : 0; }

int qe_population_configure(qe_engine* e, const qe_run_schedule* eps, const qe_run_schedule* lr, const double* gamma) {
    if (int rc = need_population(e)) return rc;
    static_assert(sizeof(qe_run_schedule) == sizeof(RunSched), "qe_run_schedule and RunSched differ");
    const size_t m = (size_t)e->pop.runs;
    if (gamma && e->pop.trace.k)  // (the kernel multiplies the traces by T(gamma * lambda))
        if (int rc = check_trace_decay(e, gamma, e->pop.trace.h_lambda.data())) return rc;
    for (const qe_run_schedule* d : {eps, lr})
        for (size_t r = 0; d && r < m; ++r)
            if (d[r].kind < QE_SCHED_CONSTANT || d[r].kind > QE_SCHED_EXPONENTIAL)
                return qe_fail(QE_ERR_INVALID, "schedule of run %lld: unknown kind %d", (long long)r, (int)d[r].kind);
    HIP_TRY(hipSetDevice(e->device));
    if (eps) HIP_TRY(hipMemcpyAsync(e->pop.eps.p, eps, m * sizeof(RunSched), hipMemcpyHostToDevice, e->stream));
    if (lr) HIP_TRY(hipMemcpyAsync(e->pop.lr.p, lr, m * sizeof(RunSched), hipMemcpyHostToDevice, e->stream));
    if (gamma) HIP_TRY(hipMemcpyAsync(e->pop.gamma.p, gamma, m * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_schedules(qe_engine* e, double* eps_values, double* lr_values) {
    if (int rc = need_population(e)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t m = (size_t)e->pop.runs;
    std::vector<RunSched> h(m);
    for (auto [dev, dst] : {std::make_pair(e->pop.eps.p, eps_values), std::make_pair(e->pop.lr.p, lr_values)}) {
        if (!dst) continue;
        HIP_TRY(hipMemcpyAsync(h.data(), dev, m * sizeof(RunSched), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (size_t r = 0; r < m; ++r) dst[r] = h[r].value;
    }
    return QE_OK;
}

int64_t qe_population_rollout(qe_engine* e, qe_env* env, int64_t steps, int32_t mode, int32_t log, qe_rollout_stats* stats,
                              int64_t* ep_count, float* ep_sum, int32_t* obs, uint32_t* aux, float* agent_rewards,
                              uint32_t* status) {
    if (int rc = call_check(e, env, steps, stats)) return rc;
    if (mode != QE_LEARN_ITER && mode != QE_LEARN_VEC) return qe_fail(QE_ERR_INVALID, "bad learn mode");
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    // One agent per run: the reference's dispatcher picks the list variants of the selection (they step over a NaN)
    // except for masked rows of more than 10 actions (q_learning_optimal.py:700, :713; see rollout_ctx)
    const bool masked = env->p.masked != 0 || env->p.kind == QE_ENV_TICTACTOE;
    PopCall c{e, env, steps, log != 0, masked && e->A > 10 ? 1 : 0, P.table_b ? QE_VARIANT_RUNS_DOUBLE : QE_VARIANT_RUNS};
    if (int rc = call_begin(c, P.dyna.planning, [&] { return P.rule == QE_RULE_SARSA ? pending_reserve(e) : QE_OK; })) return rc;
    for (long long t = 0; t < steps; t += c.per_launch)
        if (int rc = call_launch(c, t, std::min<long long>(c.per_launch, steps - t), [&](auto& l, auto tag) {
                l.c.eps = P.eps.p; l.c.lr = P.lr.p; l.c.gamma = P.gamma.p; l.c.mode = mode;
                return launch_training<std::decay_t<decltype(*l.c.q)>, decltype(tag)>(e, l);
            }))
            return rc;
    return call_end(
        c, stats, ep_count, ep_sum, status,
        [&]() -> int {
            if (obs) HIP_TRY(hipMemcpyAsync(obs, env->n.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
            if (aux) HIP_TRY(hipMemcpyAsync(aux, env->aux.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
            if (agent_rewards) HIP_TRY(hipMemcpyAsync(agent_rewards, env->acc.p, m * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            return QE_OK;
        },
        [&](long long& env_steps) {
            e->step_ctr += (uint64_t)steps;
            env_steps = steps * P.runs;
            return QE_OK;
        });
}

int64_t qe_population_evaluate(qe_engine* e, qe_env* env, int64_t steps, int64_t episodes, int32_t log, qe_rollout_stats* stats,
                               int64_t* ep_count, float* ep_sum, int64_t* used, uint32_t* status) {
    if (int rc = call_check(e, env, steps, stats)) return rc;
    if (episodes < 0) return qe_fail(QE_ERR_INVALID, "episodes must be >= 0");
    PopState& P = e->pop;
    PopState::EpisodeMode& G = P.epi;
    const size_t m = (size_t)P.runs;
    // The standalone evaluation's rule (rollout_ctx): deterministic selection takes the list variants, which step over a
    // NaN, for rows of at most 10 actions (q_learning_optimal.py:673), masked or not
    PopCall c{e, env, steps, log != 0, e->A > 10 ? 1 : 0, P.table_b ? QE_VARIANT_RUNS_DOUBLE_EVAL : QE_VARIANT_RUNS_EVAL};
    if (int rc = call_begin(c, 0, [&]() -> int {
            if (!episodes) return QE_OK;
            HIP_TRY(G.used.ensure(m)); HIP_TRY(G.done.ensure(m)); HIP_TRY(G.h_done.ensure(m));
            HIP_TRY(hipMemsetAsync(G.used.p, 0, m * sizeof(long long), e->stream));
            HIP_TRY(hipMemsetAsync(G.done.p, 0, m, e->stream));
            return QE_OK;
        }))
        return rc;
    bool all_done = false;
    for (long long t = 0; t < steps && !all_done; t += c.per_launch) {
        if (int rc = call_launch(c, t, std::min<long long>(c.per_launch, steps - t), [&](auto& l, auto tag) {
                using T = std::decay_t<decltype(*l.c.q)>;
                long long* const took = episodes ? G.used.p : nullptr;
                uint8_t* const done = episodes ? G.done.p : nullptr;
                if (P.table_b) return launch_double_evaluate<T, decltype(tag)>(l, episodes, took, done, (const T*)P.table_b);
                return launch_evaluate_runs<T, decltype(tag)>(l, episodes, took, done);
            }))
            return rc;
        if (episodes) {  // no further launch once every run has its episodes
            HIP_TRY(hipMemcpyAsync(G.h_done.p, G.done.p, m, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            all_done = std::all_of(G.h_done.p, G.h_done.p + m, [](uint8_t d) { return d != 0; });
        }
    }
    std::vector<long long> took(m, steps);
    return call_end(
        c, stats, ep_count, ep_sum, status,
        [&]() -> int {
            if (!episodes) return QE_OK;
            HIP_TRY(hipMemcpyAsync(took.data(), G.used.p, m * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipMemcpyAsync(G.h_done.p, G.done.p, m, hipMemcpyDeviceToHost, e->stream));
            return QE_OK;
        },
        [&](long long& env_steps) -> int {
            // every run's draw counter moves on by the steps it took (the standalone evaluate_episodes: start + used)
            if (episodes) {
                std::vector<uint64_t> ctr(m);
                if (int rc = get_counters(e, ctr.data())) return rc;
                for (size_t r = 0; r < m; ++r) ctr[r] += (uint64_t)took[r];
                if (int rc = set_counters(e, ctr.data())) return rc;
            } else {
                e->step_ctr += (uint64_t)steps;
            }
            for (size_t r = 0; r < m; ++r) {
                if (episodes && !G.h_done.p[r]) c.st[r] |= 2u;  // stopped by the bound `steps`
                if (used) used[r] = took[r];
                env_steps += took[r];
            }
            return QE_OK;
        });
}

int qe_population_step_counters(qe_engine* e, uint64_t* out) {
    if (int rc = need_population(e)) return rc;
    if (!out) return qe_fail(QE_ERR_INVALID, "out is NULL");
    HIP_TRY(hipSetDevice(e->device));
    return get_counters(e, out);
}

int qe_population_set_step_counters(qe_engine* e, const uint64_t* in) {
    if (int rc = need_population(e)) return rc;
    if (!in) return qe_fail(QE_ERR_INVALID, "in is NULL");
    HIP_TRY(hipSetDevice(e->device));
    return set_counters(e, in);
}

int qe_population_set_update_rule(qe_engine* e, int32_t rule) {
    if (int rc = need_population(e)) return rc;
    if (rule != QE_RULE_Q_LEARNING && rule != QE_RULE_SARSA && rule != QE_RULE_EXPECTED_SARSA)
        return qe_fail(QE_ERR_INVALID, "unknown update rule %d (qe_update_rule)", (int)rule);
    if (e->pop.visit.on && rule != QE_RULE_Q_LEARNING) return visits_refuse("an on-policy update rule");
    if (e->pop.tree.n > 1 && rule != QE_RULE_Q_LEARNING) return tree_refuse(e, "an on-policy update rule");
    if (e->pop.table_b && rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED, "the double estimator is built for Q-learning only (qe_population_set_double)");
    if (e->pop.win.n > 1 && rule == QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "n_step = %d: an uncorrected n-step Q-learning is not an off-policy method (its n-step form is Tree Backup, "
                       "qe_population_set_tree_backup); the n-step rules are SARSA and Expected SARSA",
                       e->pop.win.n);
    if (e->pop.dyna.planning && rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "planning is on (%d updates per step): Dyna-Q replays remembered transitions through Q-learning's update; "
                       "planning for the on-policy rules is not built (qe_population_set_planning)",
                       e->pop.dyna.planning);
    if (e->pop.trace.k && rule == QE_RULE_EXPECTED_SARSA)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "eligibility traces are on: the trace form of Expected SARSA needs policy-probability weighting, which "
                       "is not built; the trace rules are SARSA and Q-learning (qe_population_set_traces)");
    e->pop.rule = rule;
    return QE_OK;
}

int qe_population_update_rule(qe_engine* e) {
    if (int rc = need_population(e)) return rc;
    return e->pop.rule;
}

int qe_population_set_double(qe_engine* e, int32_t on) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (on && P.visit.on) return visits_refuse("the double estimator");
    if (on && P.tree.n > 1) return tree_refuse(e, "the double estimator");
    if (on && P.win.n > 1)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: the double estimator is a one-step method (qe_population_set_n_step)", P.win.n);
    if (on && P.trace.k)
        return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces are on: the double estimator has no trace form (qe_population_set_traces)");
    if (on && P.dyna.planning)
        return qe_fail(QE_ERR_UNSUPPORTED, "planning is on: Dyna-Q plans on one table (qe_population_set_planning)");
    if (P.rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED, "the double estimator is built for Q-learning only (update rule %d)", P.rule);
    HIP_TRY(hipSetDevice(e->device));
    if (!on) {
        if (P.table_b) {
            HIP_TRY(hipStreamSynchronize(e->stream));
            (void)hipFree(P.table_b);
            P.table_b = nullptr;
        }
        return QE_OK;
    }
    if (P.table_b) return QE_OK;
    // table B: zeros, and -inf in the padding columns, exactly as qe_create leaves table A
    const size_t bytes = (size_t)e->S * e->ld * e->esize();
    void* b = nullptr;
    hipError_t err = hipMalloc(&b, bytes);
    if (err == hipSuccess) err = hipMemsetAsync(b, 0, bytes, e->stream);
    if (err == hipSuccess && e->ld > e->A) {
        const int64_t cells = e->S * (int64_t)(e->ld - e->A);
        if (e->dtype == QE_F32)
            hipLaunchKernelGGL(k_pad_fill<float>, dim3(grid_for(cells, 256)), dim3(256), 0, e->stream, (float*)b, e->S, e->A, e->ld);
        else
            hipLaunchKernelGGL(k_pad_fill<double>, dim3(grid_for(cells, 256)), dim3(256), 0, e->stream, (double*)b, e->S, e->A, e->ld);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) {
        if (b) (void)hipFree(b);
        return qe_fail(err == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_NO_DEVICE, "allocation of the second table failed: %s",
                       hipGetErrorString(err));
    }
    P.table_b = b;
    return QE_OK;
}

int qe_population_double(qe_engine* e) {
    if (int rc = need_population(e)) return rc;
    if (e->pop.rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED, "the double estimator is built for Q-learning only (update rule %d)", e->pop.rule);
    return e->pop.table_b ? 1 : 0;
}

int qe_population_table_b_upload(qe_engine* e, const void* host, int32_t host_dtype) {
    return on_table_b(e, [&] { return qe_table_upload(e, host, host_dtype); });
}

int qe_population_table_b_download(qe_engine* e, void* host, int32_t host_dtype) {
    return on_table_b(e, [&] { return qe_table_download(e, host, host_dtype); });
}

int qe_population_table_b_download_rows(qe_engine* e, void* host, int64_t first_row, int64_t rows) {
    return on_table_b(e, [&] { return qe_table_download_rows(e, host, first_row, rows); });
}

int qe_population_pending_actions(qe_engine* e, int32_t* out) {
    if (int rc = need_population(e)) return rc;
    if (!out) return qe_fail(QE_ERR_INVALID, "out is NULL");
    const size_t m = (size_t)e->pop.runs;
    if (!e->pop.pending.p) {  // never set, never run under SARSA: none
        std::fill(out, out + m, -1);
        return QE_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(out, e->pop.pending.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_pending_actions(qe_engine* e, const int32_t* in) {
    if (int rc = need_population(e)) return rc;
    const size_t m = (size_t)e->pop.runs;
    for (size_t r = 0; in && r < m; ++r)  // (the kernel indexes the run's row with it)
        if (in[r] < -1 || in[r] >= e->A)
            return qe_fail(QE_ERR_INVALID, "pending action of run %lld: %d is outside [-1, %d)", (long long)r, (int)in[r], (int)e->A);
    if (!in && !e->pop.pending.p) return QE_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = pending_reserve(e)) return rc;
    if (in) HIP_TRY(hipMemcpyAsync(e->pop.pending.p, in, m * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    else HIP_TRY(hipMemsetAsync(e->pop.pending.p, 0xFF, m * sizeof(int32_t), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_n_step(qe_engine* e, int32_t n) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (n < 1 || n > NSTEP_MAX) return qe_fail(QE_ERR_INVALID, "n_step must be in 1 .. %d, got %d", NSTEP_MAX, (int)n);
    if (n > 1 && P.visit.on) return visits_refuse("n_step > 1");
    if (n > 1 && P.tree.n > 1) return tree_refuse(e, "n_step > 1");
    if (n > 1 && P.rule == QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "n_step = %d with Q-learning: an uncorrected n-step Q-learning is not an off-policy method (its n-step form is "
                       "Tree Backup, qe_population_set_tree_backup); the n-step rules are SARSA and Expected SARSA",
                       (int)n);
    if (n > 1 && P.table_b)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: the double estimator is a one-step method (qe_population_set_double)", (int)n);
    if (n > 1 && P.dyna.planning)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: planning is on, and Dyna-Q is a one-step method (qe_population_set_planning)", (int)n);
    if (n > 1 && P.trace.k)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: eligibility traces are on, and they are the multi-step method then (qe_population_set_traces)", (int)n);
    if (n == P.win.n) return QE_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (n > 1) {
        if (int rc = window_reserve(e, n)) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(e->stream));
        P.win.release();
    }
    P.win.n = n;
    return QE_OK;
}

int qe_population_n_step(qe_engine* e) {
    if (int rc = need_population(e)) return rc;
    return e->pop.win.n;
}

int qe_population_window(qe_engine* e, int32_t* len, int32_t* states, int32_t* actions, float* rewards) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs, w = (size_t)(P.win.n - 1);
    if (!w) return QE_OK;  // a one-step rule has no window: nothing to write
    if (!len) return qe_fail(QE_ERR_INVALID, "len is NULL");
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int32_t> hs(m * w), ha(m * w);
    std::vector<float> hr(m * w);
    HIP_TRY(hipMemcpyAsync(len, P.win.len.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hs.data(), P.win.s.p, m * w * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(ha.data(), P.win.a.p, m * w * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hr.data(), P.win.r.p, m * w * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    auto used = [&](size_t r, size_t i) { return (int32_t)i < len[r]; };  // slots past the length hold 0
    slots_to_abi(hs.data(), states, m, w, used);
    slots_to_abi(ha.data(), actions, m, w, used);
    slots_to_abi(hr.data(), rewards, m, w, used);
    return QE_OK;
}

int qe_population_set_window(qe_engine* e, const int32_t* len, const int32_t* states, const int32_t* actions,
                             const float* rewards) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs, w = (size_t)(P.win.n - 1);
    if (!w) {
        for (size_t r = 0; len && r < m; ++r)
            if (len[r] != 0) return qe_fail(QE_ERR_INVALID, "window of run %lld: length %d with n_step = 1", (long long)r, (int)len[r]);
        return QE_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (!len) {  // every window empty
        HIP_TRY(hipMemsetAsync(P.win.len.p, 0, m * sizeof(int32_t), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return QE_OK;
    }
    if (!states || !actions || !rewards) return qe_fail(QE_ERR_INVALID, "states, actions or rewards is NULL");
    for (size_t r = 0; r < m; ++r) {  // (the kernel indexes LDS with the length and the run's table with the entries)
        if (len[r] < 0 || len[r] > (int32_t)w)
            return qe_fail(QE_ERR_INVALID, "window of run %lld: length %d is outside [0, %d]", (long long)r, (int)len[r], (int)w);
        for (size_t i = 0; i < (size_t)len[r]; ++i) {
            const int32_t s = states[r * w + i], a = actions[r * w + i];
            if (s < 0 || s >= P.S)
                return qe_fail(QE_ERR_INVALID, "window of run %lld: state %d is outside [0, %lld)", (long long)r, (int)s, (long long)P.S);
            if (a < 0 || a >= e->A)
                return qe_fail(QE_ERR_INVALID, "window of run %lld: action %d is outside [0, %d)", (long long)r, (int)a, (int)e->A);
        }
    }
    std::vector<int32_t> hs(m * w), ha(m * w);
    std::vector<float> hr(m * w);
    auto used = [&](size_t r, size_t i) { return i < (size_t)len[r]; };
    slots_to_device(states, hs.data(), m, w, used);
    slots_to_device(actions, ha.data(), m, w, used);
    slots_to_device(rewards, hr.data(), m, w, used);
    HIP_TRY(hipMemcpyAsync(P.win.len.p, len, m * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.win.s.p, hs.data(), m * w * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.win.a.p, ha.data(), m * w * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.win.r.p, hr.data(), m * w * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_tree_backup(qe_engine* e, int32_t n) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (n < 1 || n > TREE_MAX) return qe_fail(QE_ERR_INVALID, "tree_backup must be in 1 .. %d, got %d", TREE_MAX, (int)n);
    if (n > 1 && P.visit.on) return visits_refuse("tree_backup > 1");
    if (n > 1 && P.rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "tree_backup = %d with update rule %d: Tree Backup under a greedy target policy is Q-learning's n-step form; "
                       "the on-policy rules have n_step (qe_population_set_n_step)",
                       (int)n, P.rule);
    if (n > 1 && P.table_b)
        return qe_fail(QE_ERR_UNSUPPORTED, "tree_backup = %d: the double estimator is a one-step method (qe_population_set_double)", (int)n);
    if (n > 1 && P.win.n > 1)
        return qe_fail(QE_ERR_UNSUPPORTED, "tree_backup = %d with n_step = %d: one multi-step method at a time (qe_population_set_n_step)", (int)n, P.win.n);
    if (n > 1 && P.trace.k)
        return qe_fail(QE_ERR_UNSUPPORTED, "tree_backup = %d: eligibility traces are on, and they are the multi-step method then (qe_population_set_traces)", (int)n);
    if (n > 1 && P.dyna.planning)
        return qe_fail(QE_ERR_UNSUPPORTED, "tree_backup = %d: planning is on, and Dyna-Q is a one-step method (qe_population_set_planning)", (int)n);
    if (n == P.tree.n) return QE_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (n > 1) {
        if (int rc = tree_reserve(e, n)) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(e->stream));
        P.tree.release();
    }
    P.tree.n = n;
    return QE_OK;
}

int qe_population_tree_backup(qe_engine* e) {
    if (int rc = need_population(e)) return rc;
    return e->pop.tree.n;
}

int qe_population_tree_window(qe_engine* e, int32_t* len, int32_t* states, int32_t* actions, float* rewards, uint8_t* greedy) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs, w = (size_t)(P.tree.n - 1);
    if (!w) return QE_OK;  // the one-step rule has no window: nothing to write
    if (!len) return qe_fail(QE_ERR_INVALID, "len is NULL");
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int32_t> hs(m * w), ha(m * w), hf(m * w);
    std::vector<float> hr(m * w);
    HIP_TRY(hipMemcpyAsync(len, P.tree.len.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hs.data(), P.tree.s.p, m * w * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(ha.data(), P.tree.a.p, m * w * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hr.data(), P.tree.r.p, m * w * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < m * w; ++k) {  // the action word: the action, and the flag in its top bit
        hf[k] = ha[k] < 0 ? 1 : 0;
        ha[k] &= ~TREE_GREEDY;
    }
    auto used = [&](size_t r, size_t i) { return (int32_t)i < len[r]; };  // slots past the length hold 0
    slots_to_abi(hs.data(), states, m, w, used);
    slots_to_abi(ha.data(), actions, m, w, used);
    slots_to_abi(hr.data(), rewards, m, w, used);
    slots_to_abi(hf.data(), greedy, m, w, used);
    return QE_OK;
}

int qe_population_set_tree_window(qe_engine* e, const int32_t* len, const int32_t* states, const int32_t* actions,
                                  const float* rewards, const uint8_t* greedy) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs, w = (size_t)(P.tree.n - 1);
    if (!w) {
        for (size_t r = 0; len && r < m; ++r)
            if (len[r] != 0) return qe_fail(QE_ERR_INVALID, "window of run %lld: length %d with tree_backup = 1", (long long)r, (int)len[r]);
        return QE_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (!len) {  // every window empty
        HIP_TRY(hipMemsetAsync(P.tree.len.p, 0, m * sizeof(int32_t), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return QE_OK;
    }
    if (!states || !actions || !rewards || !greedy) return qe_fail(QE_ERR_INVALID, "states, actions, rewards or greedy is NULL");
    for (size_t r = 0; r < m; ++r) {  // (the kernel indexes LDS with the length and the run's table with the entries)
        if (len[r] < 0 || len[r] > (int32_t)w)
            return qe_fail(QE_ERR_INVALID, "window of run %lld: length %d is outside [0, %d]", (long long)r, (int)len[r], (int)w);
        for (size_t i = 0; i < (size_t)len[r]; ++i) {
            const int32_t s = states[r * w + i], a = actions[r * w + i];
            if (s < 0 || s >= P.S)
                return qe_fail(QE_ERR_INVALID, "window of run %lld: state %d is outside [0, %lld)", (long long)r, (int)s, (long long)P.S);
            if (a < 0 || a >= e->A)
                return qe_fail(QE_ERR_INVALID, "window of run %lld: action %d is outside [0, %d)", (long long)r, (int)a, (int)e->A);
            if (greedy[r * w + i] > 1)
                return qe_fail(QE_ERR_INVALID, "window of run %lld: greedy flag %d is neither 0 nor 1", (long long)r, (int)greedy[r * w + i]);
        }
    }
    std::vector<int32_t> hs(m * w), ha(m * w), packed(m * w);
    std::vector<float> hr(m * w);
    for (size_t k = 0; k < m * w; ++k) packed[k] = actions[k] | (greedy[k] ? TREE_GREEDY : 0);
    auto used = [&](size_t r, size_t i) { return i < (size_t)len[r]; };
    slots_to_device(states, hs.data(), m, w, used);
    slots_to_device(packed.data(), ha.data(), m, w, used);
    slots_to_device(rewards, hr.data(), m, w, used);
    HIP_TRY(hipMemcpyAsync(P.tree.len.p, len, m * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.tree.s.p, hs.data(), m * w * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.tree.a.p, ha.data(), m * w * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.tree.r.p, hr.data(), m * w * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_traces(qe_engine* e, int32_t K, int32_t kind, const double* lambda) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    if (!lambda) {  // off
        if (!P.trace.k) return QE_OK;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipStreamSynchronize(e->stream));
        P.trace.release();
        return QE_OK;
    }
    if (K < 1 || K > TRACE_MAX) return qe_fail(QE_ERR_INVALID, "trace_length must be in 1 .. %d, got %d", TRACE_MAX, (int)K);
    if (kind != QE_TRACE_REPLACING && kind != QE_TRACE_ACCUMULATING)
        return qe_fail(QE_ERR_INVALID, "unknown trace kind %d (qe_trace_kind)", (int)kind);
    if (P.visit.on) return visits_refuse("eligibility traces");
    if (P.tree.n > 1) return tree_refuse(e, "eligibility traces");
    for (size_t r = 0; r < m; ++r)
        if (!(lambda[r] >= 0.0 && lambda[r] <= 1.0))
            return qe_fail(QE_ERR_UNSUPPORTED, "trace decay of run %lld: lambda = %g is outside [0, 1]", (long long)r, lambda[r]);
    if (P.rule == QE_RULE_EXPECTED_SARSA)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "eligibility traces with Expected SARSA: its trace form needs policy-probability weighting, which is not "
                       "built; the trace rules are SARSA and Q-learning");
    if (P.table_b) return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces: the double estimator has no trace form (qe_population_set_double)");
    if (P.dyna.planning)
        return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces: planning is on, and Dyna-Q is a one-step method (qe_population_set_planning)");
    if (P.win.n > 1)
        return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces with n_step = %d: one multi-step method at a time (qe_population_set_n_step)", P.win.n);
    HIP_TRY(hipSetDevice(e->device));
    std::vector<double> gamma(m);
    HIP_TRY(hipMemcpyAsync(gamma.data(), P.gamma.p, m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rc = check_trace_decay(e, gamma.data(), lambda)) return rc;
    const size_t cells = m * (size_t)K;
    PopState::Traces& X = P.trace;
    HIP_TRY(X.s.ensure(cells)); HIP_TRY(X.a.ensure(cells)); HIP_TRY(X.e.ensure(cells)); HIP_TRY(X.lambda.ensure(m));
    HIP_TRY(hipMemcpyAsync(X.lambda.p, lambda, m * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    X.h_lambda.assign(lambda, lambda + m);
    X.k = K;
    X.kind = kind;
    return traces_clear(e);
}

int qe_population_trace_config(qe_engine* e, int32_t* K, int32_t* kind, double* lambda) {
    if (int rc = need_population(e)) return rc;
    const PopState::Traces& X = e->pop.trace;
    if (K) *K = X.k;
    if (kind) *kind = X.k ? X.kind : 0;
    if (lambda && X.k) std::copy(X.h_lambda.begin(), X.h_lambda.end(), lambda);
    return X.k ? 1 : 0;
}

int qe_population_traces(qe_engine* e, int32_t* states, int32_t* actions, double* values) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.trace.k) return qe_fail(QE_ERR_INVALID, "eligibility traces are off (qe_population_set_traces)");
    const size_t m = (size_t)P.runs, k = (size_t)P.trace.k;
    const bool f32 = e->dtype == QE_F32;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int32_t> hs(m * k), ha(m * k);
    std::vector<double> he(m * k);
    HIP_TRY(hipMemcpyAsync(hs.data(), P.trace.s.p, m * k * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(ha.data(), P.trace.a.p, m * k * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(he.data(), P.trace.e.p, m * k * e->esize(), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const float* const he32 = reinterpret_cast<const float*>(he.data());
    auto live = [&](size_t r, size_t i) { return (f32 ? (double)he32[i * m + r] : he[i * m + r]) != 0.0; };  // free slots read (0, 0, 0.0)
    slots_to_abi(hs.data(), states, m, k, live);
    slots_to_abi(ha.data(), actions, m, k, live);
    if (f32) slots_to_abi(he32, values, m, k, live);
    else slots_to_abi(he.data(), values, m, k, live);
    return QE_OK;
}

int qe_population_set_trace_state(qe_engine* e, const int32_t* states, const int32_t* actions, const double* values) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.trace.k) return qe_fail(QE_ERR_INVALID, "eligibility traces are off (qe_population_set_traces)");
    HIP_TRY(hipSetDevice(e->device));
    if (!states && !actions && !values) return traces_clear(e);
    if (!states || !actions || !values) return qe_fail(QE_ERR_INVALID, "states, actions or values is NULL");
    const size_t m = (size_t)P.runs, k = (size_t)P.trace.k;
    const bool f32 = e->dtype == QE_F32;
    for (size_t r = 0; r < m; ++r)  // (the kernel indexes the run's table with the live slots)
        for (size_t i = 0; i < k; ++i) {
            const double v = values[r * k + i];
            if (!(v >= 0.0) || std::isinf(v) || (f32 && (double)(float)v != v))
                return qe_fail(QE_ERR_INVALID, "trace slot %d of run %lld: the value %g is negative, not finite or not a %s",
                               (int)i, (long long)r, v, f32 ? "float32" : "float64");
            if (v == 0.0) continue;  // free
            const int32_t s = states[r * k + i], a = actions[r * k + i];
            if (s < 0 || s >= P.S)
                return qe_fail(QE_ERR_INVALID, "trace slot %d of run %lld: state %d is outside [0, %lld)", (int)i, (long long)r, (int)s,
                               (long long)P.S);
            if (a < 0 || a >= e->A)
                return qe_fail(QE_ERR_INVALID, "trace slot %d of run %lld: action %d is outside [0, %d)", (int)i, (long long)r, (int)a,
                               (int)e->A);
            for (size_t j = 0; j < i; ++j)
                if (values[r * k + j] != 0.0 && states[r * k + j] == s && actions[r * k + j] == a)
                    return qe_fail(QE_ERR_INVALID, "trace slots %d and %d of run %lld name the same cell (%d, %d)", (int)j, (int)i,
                                   (long long)r, (int)s, (int)a);
        }
    std::vector<int32_t> hs(m * k), ha(m * k);
    std::vector<double> he(m * k);
    auto live = [&](size_t r, size_t i) { return values[r * k + i] != 0.0; };
    slots_to_device(states, hs.data(), m, k, live);
    slots_to_device(actions, ha.data(), m, k, live);
    if (f32) slots_to_device(values, reinterpret_cast<float*>(he.data()), m, k, live);
    else slots_to_device(values, he.data(), m, k, live);
    HIP_TRY(hipMemcpyAsync(P.trace.s.p, hs.data(), m * k * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.trace.a.p, ha.data(), m * k * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.trace.e.p, he.data(), m * k * e->esize(), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_planning(qe_engine* e, int32_t n) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (n < 0 || n > DYNA_MAX) return qe_fail(QE_ERR_INVALID, "planning_steps must be in 0 .. %d, got %d", DYNA_MAX, (int)n);
    if (n == 0) {  // off: the model is forgotten
        if (!P.dyna.planning) return QE_OK;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipStreamSynchronize(e->stream));
        P.dyna.release();
        return QE_OK;
    }
    if (P.visit.on) return visits_refuse("planning");
    if (P.tree.n > 1) return tree_refuse(e, "planning");
    if (P.rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "planning with update rule %d: Dyna-Q replays remembered transitions through Q-learning's update; planning "
                       "for the on-policy rules is not built",
                       P.rule);
    if (P.table_b) return qe_fail(QE_ERR_UNSUPPORTED, "planning: Dyna-Q plans on one table, the double estimator has two (qe_population_set_double)");
    if (P.win.n > 1)
        return qe_fail(QE_ERR_UNSUPPORTED, "planning with n_step = %d: Dyna-Q is a one-step method (qe_population_set_n_step)", P.win.n);
    if (P.trace.k) return qe_fail(QE_ERR_UNSUPPORTED, "planning with eligibility traces: Dyna-Q is a one-step method (qe_population_set_traces)");
    // (the list and the kernel name a cell by its offset in the run's table, an int32; ld >= A)
    if ((double)P.S * (double)e->ld >= 2147483648.0)
        return qe_fail(QE_ERR_UNSUPPORTED, "planning: a run's table must hold fewer than 2^31 cells (state_size * row stride = %lld * %d)",
                       (long long)P.S, (int)e->ld);
    if (P.dyna.planning) {  // already on: the model is knowledge and stays
        P.dyna.planning = n;
        return QE_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    const size_t m = (size_t)P.runs;
    hipError_t err = P.dyna.entry.ensure(m * (size_t)P.S * (size_t)e->ld);
    if (err == hipSuccess) err = P.dyna.visited.ensure(m * (size_t)P.S * (size_t)e->A);
    if (err == hipSuccess) err = P.dyna.count.ensure(m);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        P.dyna.release();
        return qe_fail(err == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_NO_DEVICE, "planning: the model could not be allocated: %s",
                       hipGetErrorString(err));
    }
    if (int rc = model_clear(e)) return rc;
    P.dyna.planning = n;
    return QE_OK;
}

int qe_population_planning(qe_engine* e) {
    if (int rc = need_population(e)) return rc;
    return e->pop.dyna.planning;
}

int qe_population_model(qe_engine* e, int32_t* next_states, float* rewards, uint8_t* terminated, int32_t* visited, int32_t* count) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.dyna.planning) return qe_fail(QE_ERR_INVALID, "planning is off (qe_population_set_planning)");
    const size_t m = (size_t)P.runs, S = (size_t)P.S, A = (size_t)e->A, ld = (size_t)e->ld;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int32_t> hc(m);
    HIP_TRY(hipMemcpyAsync(hc.data(), P.dyna.count.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (next_states || rewards || terminated) {
        std::vector<uint2> he(m * S * ld);
        HIP_TRY(hipMemcpyAsync(he.data(), P.dyna.entry.p, he.size() * sizeof(uint2), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (size_t r = 0; r < m; ++r)
            for (size_t s = 0; s < S; ++s)
                for (size_t a = 0; a < A; ++a) {
                    const uint2 x = he[(r * S + s) * ld + a];
                    const bool seen = x.x != DYNA_UNSEEN;
                    const size_t at = (r * S + s) * A + a;
                    if (next_states) next_states[at] = seen ? (int32_t)(x.x & 0x7FFFFFFFu) : -1;
                    if (rewards) {
                        const uint32_t bits = seen ? x.y : 0u;
                        memcpy(&rewards[at], &bits, sizeof bits);
                    }
                    if (terminated) terminated[at] = seen && (x.x >> 31) ? 1 : 0;
                }
    }
    if (visited) {
        std::vector<int32_t> hv(m * S * A);
        HIP_TRY(hipMemcpyAsync(hv.data(), P.dyna.visited.p, hv.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (size_t r = 0; r < m; ++r)  // table offsets s * ld + a -> cells s * A + a; -1 past the count
            for (size_t j = 0; j < S * A; ++j) {
                const int32_t o = hv[r * S * A + j];
                visited[r * S * A + j] = j < (size_t)hc[r] ? (int32_t)((size_t)o / ld * A + (size_t)o % ld) : -1;
            }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (count) std::copy(hc.begin(), hc.end(), count);
    return QE_OK;
}

int qe_population_set_model(qe_engine* e, const int32_t* next_states, const float* rewards, const uint8_t* terminated,
                            const int32_t* visited, const int32_t* count) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.dyna.planning) return qe_fail(QE_ERR_INVALID, "planning is off (qe_population_set_planning)");
    HIP_TRY(hipSetDevice(e->device));
    if (!next_states && !rewards && !terminated && !visited && !count) return model_clear(e);
    if (!next_states || !rewards || !terminated || !visited || !count)
        return qe_fail(QE_ERR_INVALID, "next_states, rewards, terminated, visited or count is NULL");
    const size_t m = (size_t)P.runs, S = (size_t)P.S, A = (size_t)e->A, ld = (size_t)e->ld;
    std::vector<uint2> he(m * S * ld, make_uint2(DYNA_UNSEEN, DYNA_UNSEEN));
    std::vector<int32_t> hv(m * S * A, 0);
    std::vector<uint8_t> listed(S * A);
    for (size_t r = 0; r < m; ++r) {  // (the kernel indexes the run's table with the entries and the list)
        size_t seen = 0;
        for (size_t c = 0; c < S * A; ++c) {
            const int32_t p = next_states[r * S * A + c];
            if (p == -1) continue;
            if (p < 0 || (size_t)p >= S)
                return qe_fail(QE_ERR_INVALID, "model of run %lld, cell %lld: next state %d is outside [0, %lld) and is not -1",
                               (long long)r, (long long)c, (int)p, (long long)S);
            uint32_t bits;
            memcpy(&bits, &rewards[r * S * A + c], sizeof bits);
            he[(r * S + c / A) * ld + c % A] = make_uint2((uint32_t)p | (terminated[r * S * A + c] ? 0x80000000u : 0u), bits);
            ++seen;
        }
        if (count[r] < 0 || (size_t)count[r] != seen)
            return qe_fail(QE_ERR_INVALID, "model of run %lld: count is %d, the model holds %lld seen cells", (long long)r, (int)count[r],
                           (long long)seen);
        std::fill(listed.begin(), listed.end(), 0);
        for (size_t j = 0; j < seen; ++j) {
            const int32_t c = visited[r * S * A + j];
            if (c < 0 || (size_t)c >= S * A)
                return qe_fail(QE_ERR_INVALID, "visited list of run %lld, entry %lld: cell %d is outside [0, %lld)", (long long)r,
                               (long long)j, (int)c, (long long)(S * A));
            if (next_states[r * S * A + (size_t)c] == -1)
                return qe_fail(QE_ERR_INVALID, "visited list of run %lld, entry %lld: cell %d is unseen in the model", (long long)r,
                               (long long)j, (int)c);
            if (listed[(size_t)c])
                return qe_fail(QE_ERR_INVALID, "visited list of run %lld, entry %lld: cell %d is listed twice", (long long)r, (long long)j,
                               (int)c);
            listed[(size_t)c] = 1;
            hv[r * S * A + j] = (int32_t)((size_t)c / A * ld + (size_t)c % A);
        }
    }
    HIP_TRY(hipMemcpyAsync(P.dyna.entry.p, he.data(), he.size() * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.dyna.visited.p, hv.data(), hv.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.dyna.count.p, count, m * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_visits(qe_engine* e, const double* bonus, int32_t visit_lr) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    PopState::Visits& V = P.visit;
    const size_t m = (size_t)P.runs;
    if (!bonus && !visit_lr) {  // off: the counts are forgotten
        if (!V.on) return QE_OK;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipStreamSynchronize(e->stream));
        V.release();
        return QE_OK;
    }
    if (P.rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "visit counts with update rule %d: the bonus changes the behaviour policy only, and the on-policy rules "
                       "under a bonus policy are not built",
                       P.rule);
    if (P.tree.n > 1) return tree_refuse(e, "visit counts");
    if (P.table_b) return qe_fail(QE_ERR_UNSUPPORTED, "visit counts: the double estimator is on (qe_population_set_double)");
    if (P.win.n > 1) return qe_fail(QE_ERR_UNSUPPORTED, "visit counts with n_step = %d: they are built for the one-step rule (qe_population_set_n_step)", P.win.n);
    if (P.trace.k) return qe_fail(QE_ERR_UNSUPPORTED, "visit counts: eligibility traces are on (qe_population_set_traces)");
    if (P.dyna.planning) return qe_fail(QE_ERR_UNSUPPORTED, "visit counts: planning is on (qe_population_set_planning)");
    bool any = false;
    for (size_t r = 0; bonus && r < m; ++r) {
        if (!(bonus[r] >= 0.0) || std::isinf(bonus[r]))
            return qe_fail(QE_ERR_UNSUPPORTED, "exploration bonus of run %lld: beta = %g is negative or not finite", (long long)r, bonus[r]);
        any |= bonus[r] > 0.0;
    }
    if (e->ld > 64 || !visit_supported(e->dtype == QE_F32, e->ld / 4))
        return qe_fail(QE_ERR_UNSUPPORTED, "visit counts: the kernel for %s rows of %d actions is not built (it does not fit the register file)",
                       e->dtype == QE_F32 ? "float32" : "float64", (int)e->A);
    HIP_TRY(hipSetDevice(e->device));
    const size_t cells = m * (size_t)P.S * (size_t)e->ld;
    if (!V.on) {  // (already on: the counts are knowledge and stay)
        hipError_t err = V.n.ensure(cells);
        if (err == hipSuccess) err = V.b.ensure(cells * e->esize());
        if (err == hipSuccess) err = V.beta.ensure(m);
        if (err == hipSuccess) err = hipMemsetAsync(V.n.p, 0, cells * sizeof(uint32_t), e->stream);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            V.release();
            return qe_fail(err == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_NO_DEVICE, "visit counts: the planes could not be allocated: %s",
                           hipGetErrorString(err));
        }
    }
    V.h_beta.assign(m, 0.0);
    if (bonus) std::copy(bonus, bonus + m, V.h_beta.begin());
    HIP_TRY(hipMemcpyAsync(V.beta.p, V.h_beta.data(), m * sizeof(double), hipMemcpyHostToDevice, e->stream));
    V.on = true;
    V.lr = visit_lr != 0;
    V.any_bonus = any;
    return visits_fill(e);
}

int qe_population_visits(qe_engine* e, int32_t* on, int32_t* visit_lr, double* bonus) {
    if (int rc = need_population(e)) return rc;
    const PopState::Visits& V = e->pop.visit;
    if (on) *on = V.on ? 1 : 0;
    if (visit_lr) *visit_lr = V.on && V.lr ? 1 : 0;
    if (bonus && V.on) std::copy(V.h_beta.begin(), V.h_beta.end(), bonus);
    return QE_OK;
}

int qe_population_visit_counts(qe_engine* e, uint32_t* out) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.visit.on) return qe_fail(QE_ERR_INVALID, "visit counts are off (qe_population_set_visits)");
    if (!out) return qe_fail(QE_ERR_INVALID, "out is NULL");
    const size_t rows = (size_t)P.runs * (size_t)P.S, A = (size_t)e->A, ld = (size_t)e->ld;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint32_t> h(rows * ld);
    HIP_TRY(hipMemcpyAsync(h.data(), P.visit.n.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < rows; ++i) std::copy(h.begin() + i * ld, h.begin() + i * ld + A, out + i * A);
    return QE_OK;
}

int qe_population_set_visit_counts(qe_engine* e, const uint32_t* in) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.visit.on) return qe_fail(QE_ERR_INVALID, "visit counts are off (qe_population_set_visits)");
    const size_t rows = (size_t)P.runs * (size_t)P.S, A = (size_t)e->A, ld = (size_t)e->ld;
    HIP_TRY(hipSetDevice(e->device));
    if (!in) {
        HIP_TRY(hipMemsetAsync(P.visit.n.p, 0, rows * ld * sizeof(uint32_t), e->stream));
        return visits_fill(e);
    }
    std::vector<uint32_t> h(rows * ld, 0u);  // (the padding columns hold 0)
    for (size_t i = 0; i < rows; ++i) std::copy(in + i * A, in + i * A + A, h.begin() + i * ld);
    HIP_TRY(hipMemcpyAsync(P.visit.n.p, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return visits_fill(e);
}

int qe_population_visit_bonus(qe_engine* e, void* out, int32_t dtype) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.visit.on) return qe_fail(QE_ERR_INVALID, "visit counts are off (qe_population_set_visits)");
    if (!out) return qe_fail(QE_ERR_INVALID, "out is NULL");
    if (dtype != QE_F32 && dtype != QE_F64) return qe_fail(QE_ERR_INVALID, "bad dtype %d", (int)dtype);
    const size_t rows = (size_t)P.runs * (size_t)P.S, A = (size_t)e->A, ld = (size_t)e->ld;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<uint8_t> h(rows * ld * e->esize());
    HIP_TRY(hipMemcpyAsync(h.data(), P.visit.b.p, h.size(), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const float* const h32 = reinterpret_cast<const float*>(h.data());
    const double* const h64 = reinterpret_cast<const double*>(h.data());
    for (size_t i = 0; i < rows; ++i)
        for (size_t a = 0; a < A; ++a) {
            const double v = e->dtype == QE_F32 ? (double)h32[i * ld + a] : h64[i * ld + a];
            if (dtype == QE_F32) ((float*)out)[i * A + a] = (float)v;
            else ((double*)out)[i * A + a] = v;
        }
    return QE_OK;
}

int64_t qe_population_log(qe_engine* e, int64_t cap, int32_t* step, float* ret) {
    if (int rc = need_population(e)) return rc;
    const int64_t n = (int64_t)e->pop.log.step.size();
    for (int64_t k = 0; k < n && k < cap; ++k) {
        if (step) step[k] = e->pop.log.step[(size_t)k];
        if (ret) ret[k] = e->pop.log.ret[(size_t)k];
    }
    return n;
}

}  // extern "C"
