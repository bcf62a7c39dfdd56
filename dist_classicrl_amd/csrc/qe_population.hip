// qe_population.hip -- host side of the population path (include/qlearn_engine.h, "population"): M independent
// single-agent runs in one [M * S, ld] table, trained by k_rollout_runs (Q-learning) or k_rollout_runs_td (SARSA, Expected
// SARSA: qe_rollout_runs_td.h, instantiated in qe_inst_runs_td.hip) and evaluated greedily by k_evaluate_runs
// (qe_rollout_runs.h, instantiated in qe_inst_runs.hip), plus the compaction of the per-run episode-log segments and
// the per-run draw counters.  With the double estimator on (qe_population_set_double) a second table B of the same
// shape stands beside the engine's table A: k_double_rollout trains both and k_double_evaluate acts on their sum
// (qe_rollout_double.h, instantiated in qe_inst_runs_double.hip).  With a horizon n > 1 (qe_population_set_n_step) the
// on-policy rules train through k_nstep_rollout (qe_rollout_nstep.h, instantiated in qe_inst_runs_nstep.hip), which
// carries every run's window of transitions from launch to launch in the win_* arrays.  With eligibility traces on
// (qe_population_set_traces) SARSA and Q-learning train through k_trace_rollout (qe_rollout_trace.h, instantiated in
// qe_inst_runs_trace.hip), which carries every run's trace slots from launch to launch in the trace_* arrays.  With
// planning on (qe_population_set_planning) Q-learning trains through k_dyna_rollout (qe_rollout_dyna.h, instantiated in
// qe_inst_runs_dyna.hip), which keeps every run's learned model and visited list in the dyna_* arrays.
#include "qe_host.h"
#include "qe_rollout_dyna.h"
#include "qe_rollout_nstep.h"
#include "qe_rollout_trace.h"

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

int log_reserve(PopState& P, size_t m, long long per_launch) {
    const size_t seg = m * (size_t)per_launch;
    HIP_TRY(P.seg_cnt.ensure(m)); HIP_TRY(P.off.ensure(m + 1)); HIP_TRY(P.seg_step.ensure(seg)); HIP_TRY(P.seg_ret.ensure(seg));
    HIP_TRY(P.out_step.ensure(seg)); HIP_TRY(P.out_ret.ensure(seg)); HIP_TRY(P.h_cnt.ensure(m + 1));
    return QE_OK;
}

// Episode log of a call, launch-major: per launch, each run's entries in order.
struct CallLog {
    std::vector<int32_t> cnt, step;
    std::vector<float> ret;
};

// Compacts the segments the launch of `k` steps has just written and appends them to `L` (synchronises the stream).
int log_launch(qe_engine* e, long long k, CallLog& L, int64_t& launches) {
    PopState& P = e->pop;
    const int64_t M = P.runs;
    const size_t m = (size_t)M;
    hipLaunchKernelGGL(k_runs_log_scan, dim3(1), dim3(1024), 0, e->stream, (const int32_t*)P.seg_cnt.p, M, P.off.p);
    hipLaunchKernelGGL(k_runs_log_pack, dim3(grid_for(M, 256)), dim3(256), 0, e->stream, (const int32_t*)P.seg_cnt.p,
                       (const int32_t*)P.off.p, (const int32_t*)P.seg_step.p, (const float*)P.seg_ret.p, k, M,
                       P.out_step.p, P.out_ret.p);
    launches += 2;
    HIP_TRY(hipMemcpyAsync(P.h_cnt.p, P.seg_cnt.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(P.h_cnt.p + m, P.off.p + m, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t total = (size_t)P.h_cnt.p[m];
    L.cnt.insert(L.cnt.end(), P.h_cnt.p, P.h_cnt.p + m);
    if (total) {
        HIP_TRY(P.h_step.ensure(total)); HIP_TRY(P.h_ret.ensure(total));
        HIP_TRY(hipMemcpyAsync(P.h_step.p, P.out_step.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(P.h_ret.p, P.out_ret.p, total * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        L.step.insert(L.step.end(), P.h_step.p, P.h_step.p + total);
        L.ret.insert(L.ret.end(), P.h_ret.p, P.h_ret.p + total);
    }
    return QE_OK;
}

// Launch-major -> (run, episode) order, into P.log_step / P.log_ret (qe_population_log).
void log_finish(PopState& P, const CallLog& L, const std::vector<long long>& counts) {
    const size_t m = (size_t)P.runs;
    std::vector<size_t> at(m + 1, 0);
    for (size_t r = 0; r < m; ++r) at[r + 1] = at[r] + (size_t)counts[r];
    P.log_step.resize(L.step.size());
    P.log_ret.resize(L.ret.size());
    size_t src = 0;
    for (size_t l = 0; l < L.cnt.size() / std::max<size_t>(m, 1); ++l)
        for (size_t r = 0; r < m; ++r)
            for (int32_t j = 0; j < L.cnt[l * m + r]; ++j, ++src) {
                P.log_step[at[r]] = L.step[src];
                P.log_ret[at[r]] = L.ret[src];
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
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs, cells = m * (size_t)(n - 1);
    HIP_TRY(P.win_len.ensure(m)); HIP_TRY(P.win_s.ensure(cells)); HIP_TRY(P.win_a.ensure(cells)); HIP_TRY(P.win_r.ensure(cells));
    HIP_TRY(hipMemsetAsync(P.win_len.p, 0, m * sizeof(int32_t), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
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
    PopState& P = e->pop;
    const size_t cells = (size_t)P.runs * (size_t)P.trace_k;
    HIP_TRY(hipMemsetAsync(P.trace_s.p, 0, cells * sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(P.trace_a.p, 0, cells * sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(P.trace_e.p, 0, cells * sizeof(double), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

// Dyna-Q: every run's model unseen, its list empty.
int model_clear(qe_engine* e) {
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    HIP_TRY(hipMemsetAsync(P.dyna_entry.p, 0xFF, m * (size_t)P.S * (size_t)e->ld * sizeof(uint2), e->stream));  // DYNA_UNSEEN
    HIP_TRY(hipMemsetAsync(P.dyna_count.p, 0, m * sizeof(int32_t), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
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
    e->pop.runs = runs;
    e->pop.S = S;
    const size_t m = (size_t)runs;
    hipError_t err = e->pop.eps.ensure(m);
    if (err == hipSuccess) err = e->pop.lr.ensure(m);
    if (err == hipSuccess) err = e->pop.gamma.ensure(m);
    if (err == hipSuccess) err = e->pop.status.ensure(m);
    if (err == hipSuccess) err = e->pop.ep_count.ensure(m);
    if (err == hipSuccess) err = e->pop.ep_sum.ensure(m);
    if (err == hipSuccess) err = hipMemsetAsync(e->pop.eps.p, 0, m * sizeof(RunSched), e->stream);  // constant 0
    if (err == hipSuccess) err = hipMemsetAsync(e->pop.lr.p, 0, m * sizeof(RunSched), e->stream);
    if (err == hipSuccess) err = hipMemsetAsync(e->pop.gamma.p, 0, m * sizeof(double), e->stream);
    if (err == hipSuccess) err = hipEventCreate(&e->pop.ev0);
    if (err == hipSuccess) err = hipEventCreate(&e->pop.ev1);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) {
        const int code = qe_fail(err == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_NO_DEVICE, "population allocation failed: %s",
                                 hipGetErrorString(err));
        qe_destroy(e);
        return code;
    }
    *out = e;
    return QE_OK;
}

int64_t qe_population_runs(qe_engine* e) { return e ? e->pop.runs : 0; }

int qe_population_configure(qe_engine* e, const qe_run_schedule* eps, const qe_run_schedule* lr, const double* gamma) {
    if (int rc = need_population(e)) return rc;
    static_assert(sizeof(qe_run_schedule) == sizeof(RunSched), "qe_run_schedule and RunSched differ");
    const size_t m = (size_t)e->pop.runs;
    if (gamma && e->pop.trace_k)  // (the kernel multiplies the traces by T(gamma * lambda))
        if (int rc = check_trace_decay(e, gamma, e->pop.h_lambda.data())) return rc;
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
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    P.log_step.clear();
    P.log_ret.clear();
    if (!env || env->e != e) return qe_fail(QE_ERR_INVALID, "engine/env mismatch");
    if (steps < 0) return qe_fail(QE_ERR_INVALID, "steps must be >= 0");
    if (mode != QE_LEARN_ITER && mode != QE_LEARN_VEC) return qe_fail(QE_ERR_INVALID, "bad learn mode");
    if (e->ld > 64) return qe_fail(QE_ERR_UNSUPPORTED, "a population holds rows of at most 64 actions");
    HIP_TRY(hipSetDevice(e->device));
    const int64_t M = P.runs;
    const size_t m = (size_t)M;
    const long long per_launch = launch_len(M, steps, log != 0, P.planning);
    if (log)
        if (int rc = log_reserve(P, m, per_launch)) return rc;
    env->mirror_obs = nullptr; env->mirror_aux = nullptr; env->mirror_acc = nullptr;  // the device state moves on
    HIP_TRY(hipMemsetAsync(P.status.p, 0, m * sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync(P.ep_count.p, 0, m * sizeof(long long), e->stream));
    HIP_TRY(hipMemsetAsync(P.ep_sum.p, 0, m * sizeof(float), e->stream));
    // One agent per run: the reference's dispatcher picks the list variants of the selection (they step over a NaN)
    // except for masked rows of more than 10 actions (q_learning_optimal.py:700, :713; see rollout_ctx)
    const bool masked = env->p.masked != 0 || env->p.kind == QE_ENV_TICTACTOE;
    const int nan_select = masked && e->A > 10 ? 1 : 0;
    const EnvCtx ev = make_envctx(e, env);
    if (P.rule == QE_RULE_SARSA)
        if (int rc = pending_reserve(e)) return rc;
    CallLog L;
    int64_t launches = 0, variant = P.table_b ? QE_VARIANT_RUNS_DOUBLE : QE_VARIANT_RUNS;
    HIP_TRY(hipEventRecord(P.ev0, e->stream));
    for (long long t = 0; t < steps; t += per_launch) {
        const long long k = std::min<long long>(per_launch, steps - t);
        const int64_t v = by_env(env->p.kind, [&](auto tag) -> int64_t {
            using Env = decltype(tag);
            auto go = [&](auto tt) -> int64_t {
                using T = decltype(tt);
                RunsCtx<T> c{};
                c.q = (T*)e->q; c.S = P.S; c.M = M;
                c.obs = env->n.p; c.aux = env->aux.p; c.acc = env->acc.p;
                c.eps = P.eps.p; c.lr = P.lr.p; c.gamma = P.gamma.p; c.status = P.status.p;
                c.ep_count = P.ep_count.p; c.ep_sum = P.ep_sum.p;
                if (log) { c.seg_cnt = P.seg_cnt.p; c.seg_step = P.seg_step.p; c.seg_ret = P.seg_ret.p; c.seg_len = k; }
                c.seed_lo = (uint32_t)e->seed; c.seed_hi = (uint32_t)(e->seed >> 32);
                c.mode = mode; c.nan_select = nan_select;
                c.step0 = e->step_ctr + (unsigned long long)t; c.t_call = t;
                c.step_off = P.off_any ? P.step_off.p : nullptr;
                if (P.table_b) return launch_double_runs<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k, (T*)P.table_b);
                if (P.planning) {
                    const DynaModel w{P.planning, P.dyna_entry.p, P.dyna_visited.p, P.dyna_count.p, P.S * (int64_t)e->A};
                    return launch_dyna_runs<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k, w);
                }
                if (P.trace_k) {
                    const TraceSlots<T> w{P.trace_k, P.trace_kind, P.trace_s.p, P.trace_a.p, (T*)P.trace_e.p, P.trace_lambda.p};
                    return launch_trace_runs<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k, P.rule, P.pending.p, w);
                }
                if (P.n_step > 1) {
                    const NStepWin w{P.n_step, P.win_len.p, P.win_s.p, P.win_a.p, P.win_r.p};
                    return launch_nstep_runs<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k, P.rule, P.pending.p, w);
                }
                if (P.rule != QE_RULE_Q_LEARNING)
                    return launch_runs_td<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k, P.rule, P.pending.p);
                return launch_runs<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k);
            };
            return e->dtype == QE_F32 ? go(float{}) : go(double{});
        });
        if (v < 0) return qe_fail(QE_ERR_INVALID, "unknown env kind %d", (int)env->p.kind);
        variant = v;
        ++launches;
        HIP_TRY(hipGetLastError());
        if (log)
            if (int rc = log_launch(e, k, L, launches)) return rc;
    }
    HIP_TRY(hipEventRecord(P.ev1, e->stream));
    e->step_ctr += (uint64_t)steps;
    std::vector<long long> counts(m);
    std::vector<uint32_t> st(m);
    HIP_TRY(hipMemcpyAsync(counts.data(), P.ep_count.p, m * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(st.data(), P.status.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    if (ep_sum) HIP_TRY(hipMemcpyAsync(ep_sum, P.ep_sum.p, m * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (obs) HIP_TRY(hipMemcpyAsync(obs, env->n.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (aux) HIP_TRY(hipMemcpyAsync(aux, env->aux.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    if (agent_rewards) HIP_TRY(hipMemcpyAsync(agent_rewards, env->acc.p, m * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    long long total = 0;
    for (size_t r = 0; r < m; ++r) {
        if (ep_count) ep_count[r] = counts[r];
        total += counts[r];
    }
    if (status) memcpy(status, st.data(), m * sizeof(uint32_t));
    if (log) log_finish(P, L, counts);
    if (stats) {
        float ms = 0.0f;
        if (steps > 0) HIP_TRY(hipEventElapsedTime(&ms, P.ev0, P.ev1));
        stats->kernel_ms = ms; stats->launches = launches; stats->episodes = total;
        stats->dominant_ms = ms; stats->dominant_launches = launches; stats->dominant_env_steps = steps * M;
        stats->kernel_variant = variant;
    }
    if (int rc = fail_empty(st)) return rc;
    return total;
}

int64_t qe_population_evaluate(qe_engine* e, qe_env* env, int64_t steps, int64_t episodes, int32_t log, qe_rollout_stats* stats,
                               int64_t* ep_count, float* ep_sum, int64_t* used, uint32_t* status) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    P.log_step.clear();
    P.log_ret.clear();
    if (!env || env->e != e) return qe_fail(QE_ERR_INVALID, "engine/env mismatch");
    if (steps < 0) return qe_fail(QE_ERR_INVALID, "steps must be >= 0");
    if (episodes < 0) return qe_fail(QE_ERR_INVALID, "episodes must be >= 0");
    if (e->ld > 64) return qe_fail(QE_ERR_UNSUPPORTED, "a population holds rows of at most 64 actions");
    HIP_TRY(hipSetDevice(e->device));
    const int64_t M = P.runs;
    const size_t m = (size_t)M;
    const long long per_launch = launch_len(M, steps, log != 0);
    if (log)
        if (int rc = log_reserve(P, m, per_launch)) return rc;
    if (episodes) {
        HIP_TRY(P.used.ensure(m)); HIP_TRY(P.done.ensure(m)); HIP_TRY(P.h_done.ensure(m));
        HIP_TRY(hipMemsetAsync(P.used.p, 0, m * sizeof(long long), e->stream));
        HIP_TRY(hipMemsetAsync(P.done.p, 0, m, e->stream));
    }
    env->mirror_obs = nullptr; env->mirror_aux = nullptr; env->mirror_acc = nullptr;  // the device state moves on
    HIP_TRY(hipMemsetAsync(P.status.p, 0, m * sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync(P.ep_count.p, 0, m * sizeof(long long), e->stream));
    HIP_TRY(hipMemsetAsync(P.ep_sum.p, 0, m * sizeof(float), e->stream));
    // The standalone evaluation's rule (rollout_ctx): deterministic selection takes the list variants, which step over a
    // NaN, for rows of at most 10 actions (q_learning_optimal.py:673), masked or not
    const int nan_select = e->A > 10 ? 1 : 0;
    const EnvCtx ev = make_envctx(e, env);
    CallLog L;
    int64_t launches = 0, variant = P.table_b ? QE_VARIANT_RUNS_DOUBLE_EVAL : QE_VARIANT_RUNS_EVAL;
    bool all_done = false;
    HIP_TRY(hipEventRecord(P.ev0, e->stream));
    for (long long t = 0; t < steps && !all_done; t += per_launch) {
        const long long k = std::min<long long>(per_launch, steps - t);
        const int64_t v = by_env(env->p.kind, [&](auto tag) -> int64_t {
            using Env = decltype(tag);
            auto go = [&](auto tt) -> int64_t {
                using T = decltype(tt);
                RunsCtx<T> c{};
                c.q = (T*)e->q; c.S = P.S; c.M = M;
                c.obs = env->n.p; c.aux = env->aux.p; c.acc = env->acc.p;
                c.status = P.status.p; c.ep_count = P.ep_count.p; c.ep_sum = P.ep_sum.p;
                if (log) { c.seg_cnt = P.seg_cnt.p; c.seg_step = P.seg_step.p; c.seg_ret = P.seg_ret.p; c.seg_len = k; }
                c.seed_lo = (uint32_t)e->seed; c.seed_hi = (uint32_t)(e->seed >> 32);
                c.nan_select = nan_select;
                c.step0 = e->step_ctr + (unsigned long long)t; c.t_call = t;
                c.step_off = P.off_any ? P.step_off.p : nullptr;
                if (P.table_b)
                    return launch_double_evaluate<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k, episodes,
                                                          episodes ? P.used.p : nullptr, episodes ? P.done.p : nullptr,
                                                          (const T*)P.table_b);
                return launch_evaluate_runs<T, Env>(e->stream, c, ev, e->ld, env->p.masked != 0, k, episodes,
                                                    episodes ? P.used.p : nullptr, episodes ? P.done.p : nullptr);
            };
            return e->dtype == QE_F32 ? go(float{}) : go(double{});
        });
        if (v < 0) return qe_fail(QE_ERR_INVALID, "unknown env kind %d", (int)env->p.kind);
        variant = v;
        ++launches;
        HIP_TRY(hipGetLastError());
        if (log)
            if (int rc = log_launch(e, k, L, launches)) return rc;
        if (episodes) {  // no further launch once every run has its episodes
            HIP_TRY(hipMemcpyAsync(P.h_done.p, P.done.p, m, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            all_done = std::all_of(P.h_done.p, P.h_done.p + m, [](uint8_t d) { return d != 0; });
        }
    }
    HIP_TRY(hipEventRecord(P.ev1, e->stream));
    std::vector<long long> counts(m), took(m, steps);
    std::vector<uint32_t> st(m);
    HIP_TRY(hipMemcpyAsync(counts.data(), P.ep_count.p, m * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(st.data(), P.status.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    if (ep_sum) HIP_TRY(hipMemcpyAsync(ep_sum, P.ep_sum.p, m * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (episodes) {
        HIP_TRY(hipMemcpyAsync(took.data(), P.used.p, m * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(P.h_done.p, P.done.p, m, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    // every run's draw counter moves on by the steps it took (the standalone evaluate_episodes: start + used)
    if (episodes) {
        std::vector<uint64_t> ctr(m);
        if (int rc = get_counters(e, ctr.data())) return rc;
        for (size_t r = 0; r < m; ++r) ctr[r] += (uint64_t)took[r];
        if (int rc = set_counters(e, ctr.data())) return rc;
    } else {
        e->step_ctr += (uint64_t)steps;
    }
    long long total = 0, env_steps = 0;
    for (size_t r = 0; r < m; ++r) {
        if (episodes && !P.h_done.p[r]) st[r] |= 2u;  // stopped by the bound `steps`
        if (ep_count) ep_count[r] = counts[r];
        if (used) used[r] = took[r];
        total += counts[r];
        env_steps += took[r];
    }
    if (status) memcpy(status, st.data(), m * sizeof(uint32_t));
    if (log) log_finish(P, L, counts);
    if (stats) {
        float ms = 0.0f;
        if (launches) HIP_TRY(hipEventElapsedTime(&ms, P.ev0, P.ev1));
        stats->kernel_ms = ms; stats->launches = launches; stats->episodes = total;
        stats->dominant_ms = ms; stats->dominant_launches = launches; stats->dominant_env_steps = env_steps;
        stats->kernel_variant = variant;
    }
    if (int rc = fail_empty(st)) return rc;
    return total;
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
    if (e->pop.table_b && rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED, "the double estimator is built for Q-learning only (qe_population_set_double)");
    if (e->pop.n_step > 1 && rule == QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "n_step = %d: an uncorrected n-step Q-learning is not an off-policy method (importance sampling and "
                       "tree backup are not built); the n-step rules are SARSA and Expected SARSA",
                       e->pop.n_step);
    if (e->pop.planning && rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "planning is on (%d updates per step): Dyna-Q replays remembered transitions through Q-learning's update; "
                       "planning for the on-policy rules is not built (qe_population_set_planning)",
                       e->pop.planning);
    if (e->pop.trace_k && rule == QE_RULE_EXPECTED_SARSA)
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
    if (on && P.n_step > 1)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: the double estimator is a one-step method (qe_population_set_n_step)", P.n_step);
    if (on && P.trace_k)
        return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces are on: the double estimator has no trace form (qe_population_set_traces)");
    if (on && P.planning)
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
    if (n > 1 && P.rule == QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "n_step = %d with Q-learning: an uncorrected n-step Q-learning is not an off-policy method (importance "
                       "sampling and tree backup are not built); the n-step rules are SARSA and Expected SARSA",
                       (int)n);
    if (n > 1 && P.table_b)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: the double estimator is a one-step method (qe_population_set_double)", (int)n);
    if (n > 1 && P.planning)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: planning is on, and Dyna-Q is a one-step method (qe_population_set_planning)", (int)n);
    if (n > 1 && P.trace_k)
        return qe_fail(QE_ERR_UNSUPPORTED, "n_step = %d: eligibility traces are on, and they are the multi-step method then (qe_population_set_traces)", (int)n);
    if (n == P.n_step) return QE_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (n > 1) {
        if (int rc = window_reserve(e, n)) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(e->stream));
        P.win_len.release(); P.win_s.release(); P.win_a.release(); P.win_r.release();
    }
    P.n_step = n;
    return QE_OK;
}

int qe_population_n_step(qe_engine* e) {
    if (int rc = need_population(e)) return rc;
    return e->pop.n_step;
}

int qe_population_window(qe_engine* e, int32_t* len, int32_t* states, int32_t* actions, float* rewards) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs, w = (size_t)(P.n_step - 1);
    if (!w) return QE_OK;  // a one-step rule has no window: nothing to write
    if (!len) return qe_fail(QE_ERR_INVALID, "len is NULL");
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int32_t> hs(m * w), ha(m * w);
    std::vector<float> hr(m * w);
    HIP_TRY(hipMemcpyAsync(len, P.win_len.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hs.data(), P.win_s.p, m * w * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(ha.data(), P.win_a.p, m * w * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(hr.data(), P.win_r.p, m * w * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t r = 0; r < m; ++r)  // [slot][run] -> [run][slot]; slots past the length hold 0
        for (size_t i = 0; i < w; ++i) {
            const bool used = (int32_t)i < len[r];
            if (states) states[r * w + i] = used ? hs[i * m + r] : 0;
            if (actions) actions[r * w + i] = used ? ha[i * m + r] : 0;
            if (rewards) rewards[r * w + i] = used ? hr[i * m + r] : 0.0f;
        }
    return QE_OK;
}

int qe_population_set_window(qe_engine* e, const int32_t* len, const int32_t* states, const int32_t* actions,
                             const float* rewards) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs, w = (size_t)(P.n_step - 1);
    if (!w) {
        for (size_t r = 0; len && r < m; ++r)
            if (len[r] != 0) return qe_fail(QE_ERR_INVALID, "window of run %lld: length %d with n_step = 1", (long long)r, (int)len[r]);
        return QE_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (!len) {  // every window empty
        HIP_TRY(hipMemsetAsync(P.win_len.p, 0, m * sizeof(int32_t), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return QE_OK;
    }
    if (!states || !actions || !rewards) return qe_fail(QE_ERR_INVALID, "states, actions or rewards is NULL");
    std::vector<int32_t> hs(m * w, 0), ha(m * w, 0);
    std::vector<float> hr(m * w, 0.0f);
    for (size_t r = 0; r < m; ++r) {  // (the kernel indexes LDS with the length and the run's table with the entries)
        if (len[r] < 0 || len[r] > (int32_t)w)
            return qe_fail(QE_ERR_INVALID, "window of run %lld: length %d is outside [0, %d]", (long long)r, (int)len[r], (int)w);
        for (size_t i = 0; i < (size_t)len[r]; ++i) {
            const int32_t s = states[r * w + i], a = actions[r * w + i];
            if (s < 0 || s >= P.S)
                return qe_fail(QE_ERR_INVALID, "window of run %lld: state %d is outside [0, %lld)", (long long)r, (int)s, (long long)P.S);
            if (a < 0 || a >= e->A)
                return qe_fail(QE_ERR_INVALID, "window of run %lld: action %d is outside [0, %d)", (long long)r, (int)a, (int)e->A);
            hs[i * m + r] = s; ha[i * m + r] = a; hr[i * m + r] = rewards[r * w + i];
        }
    }
    HIP_TRY(hipMemcpyAsync(P.win_len.p, len, m * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.win_s.p, hs.data(), m * w * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.win_a.p, ha.data(), m * w * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.win_r.p, hr.data(), m * w * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_traces(qe_engine* e, int32_t K, int32_t kind, const double* lambda) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    const size_t m = (size_t)P.runs;
    if (!lambda) {  // off
        if (!P.trace_k) return QE_OK;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipStreamSynchronize(e->stream));
        P.trace_s.release(); P.trace_a.release(); P.trace_e.release(); P.trace_lambda.release();
        P.h_lambda.clear();
        P.trace_k = 0;
        return QE_OK;
    }
    if (K < 1 || K > TRACE_MAX) return qe_fail(QE_ERR_INVALID, "trace_length must be in 1 .. %d, got %d", TRACE_MAX, (int)K);
    if (kind != QE_TRACE_REPLACING && kind != QE_TRACE_ACCUMULATING)
        return qe_fail(QE_ERR_INVALID, "unknown trace kind %d (qe_trace_kind)", (int)kind);
    for (size_t r = 0; r < m; ++r)
        if (!(lambda[r] >= 0.0 && lambda[r] <= 1.0))
            return qe_fail(QE_ERR_UNSUPPORTED, "trace decay of run %lld: lambda = %g is outside [0, 1]", (long long)r, lambda[r]);
    if (P.rule == QE_RULE_EXPECTED_SARSA)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "eligibility traces with Expected SARSA: its trace form needs policy-probability weighting, which is not "
                       "built; the trace rules are SARSA and Q-learning");
    if (P.table_b) return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces: the double estimator has no trace form (qe_population_set_double)");
    if (P.planning)
        return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces: planning is on, and Dyna-Q is a one-step method (qe_population_set_planning)");
    if (P.n_step > 1)
        return qe_fail(QE_ERR_UNSUPPORTED, "eligibility traces with n_step = %d: one multi-step method at a time (qe_population_set_n_step)", P.n_step);
    HIP_TRY(hipSetDevice(e->device));
    std::vector<double> gamma(m);
    HIP_TRY(hipMemcpyAsync(gamma.data(), P.gamma.p, m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rc = check_trace_decay(e, gamma.data(), lambda)) return rc;
    const size_t cells = m * (size_t)K;
    HIP_TRY(P.trace_s.ensure(cells)); HIP_TRY(P.trace_a.ensure(cells)); HIP_TRY(P.trace_e.ensure(cells)); HIP_TRY(P.trace_lambda.ensure(m));
    HIP_TRY(hipMemcpyAsync(P.trace_lambda.p, lambda, m * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    P.h_lambda.assign(lambda, lambda + m);
    P.trace_k = K;
    P.trace_kind = kind;
    return traces_clear(e);
}

int qe_population_trace_config(qe_engine* e, int32_t* K, int32_t* kind, double* lambda) {
    if (int rc = need_population(e)) return rc;
    const PopState& P = e->pop;
    if (K) *K = P.trace_k;
    if (kind) *kind = P.trace_k ? P.trace_kind : 0;
    if (lambda && P.trace_k) std::copy(P.h_lambda.begin(), P.h_lambda.end(), lambda);
    return P.trace_k ? 1 : 0;
}

int qe_population_traces(qe_engine* e, int32_t* states, int32_t* actions, double* values) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.trace_k) return qe_fail(QE_ERR_INVALID, "eligibility traces are off (qe_population_set_traces)");
    const size_t m = (size_t)P.runs, k = (size_t)P.trace_k;
    const bool f32 = e->dtype == QE_F32;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int32_t> hs(m * k), ha(m * k);
    std::vector<double> he(m * k);
    HIP_TRY(hipMemcpyAsync(hs.data(), P.trace_s.p, m * k * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(ha.data(), P.trace_a.p, m * k * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(he.data(), P.trace_e.p, m * k * e->esize(), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const float* const he32 = reinterpret_cast<const float*>(he.data());
    for (size_t r = 0; r < m; ++r)  // [slot][run] -> [run][slot]; free slots read (0, 0, 0.0)
        for (size_t i = 0; i < k; ++i) {
            const double v = f32 ? (double)he32[i * m + r] : he[i * m + r];
            const bool live = v != 0.0;
            if (states) states[r * k + i] = live ? hs[i * m + r] : 0;
            if (actions) actions[r * k + i] = live ? ha[i * m + r] : 0;
            if (values) values[r * k + i] = live ? v : 0.0;
        }
    return QE_OK;
}

int qe_population_set_trace_state(qe_engine* e, const int32_t* states, const int32_t* actions, const double* values) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.trace_k) return qe_fail(QE_ERR_INVALID, "eligibility traces are off (qe_population_set_traces)");
    HIP_TRY(hipSetDevice(e->device));
    if (!states && !actions && !values) return traces_clear(e);
    if (!states || !actions || !values) return qe_fail(QE_ERR_INVALID, "states, actions or values is NULL");
    const size_t m = (size_t)P.runs, k = (size_t)P.trace_k;
    const bool f32 = e->dtype == QE_F32;
    std::vector<int32_t> hs(m * k, 0), ha(m * k, 0);
    std::vector<double> he(m * k, 0.0);
    float* const he32 = reinterpret_cast<float*>(he.data());
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
            hs[i * m + r] = s; ha[i * m + r] = a;
            if (f32) he32[i * m + r] = (float)v;
            else he[i * m + r] = v;
        }
    HIP_TRY(hipMemcpyAsync(P.trace_s.p, hs.data(), m * k * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.trace_a.p, ha.data(), m * k * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.trace_e.p, he.data(), m * k * e->esize(), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int qe_population_set_planning(qe_engine* e, int32_t n) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (n < 0 || n > DYNA_MAX) return qe_fail(QE_ERR_INVALID, "planning_steps must be in 0 .. %d, got %d", DYNA_MAX, (int)n);
    if (n == 0) {  // off: the model is forgotten
        if (!P.planning) return QE_OK;
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipStreamSynchronize(e->stream));
        P.dyna_entry.release(); P.dyna_visited.release(); P.dyna_count.release();
        P.planning = 0;
        return QE_OK;
    }
    if (P.rule != QE_RULE_Q_LEARNING)
        return qe_fail(QE_ERR_UNSUPPORTED,
                       "planning with update rule %d: Dyna-Q replays remembered transitions through Q-learning's update; planning "
                       "for the on-policy rules is not built",
                       P.rule);
    if (P.table_b) return qe_fail(QE_ERR_UNSUPPORTED, "planning: Dyna-Q plans on one table, the double estimator has two (qe_population_set_double)");
    if (P.n_step > 1)
        return qe_fail(QE_ERR_UNSUPPORTED, "planning with n_step = %d: Dyna-Q is a one-step method (qe_population_set_n_step)", P.n_step);
    if (P.trace_k) return qe_fail(QE_ERR_UNSUPPORTED, "planning with eligibility traces: Dyna-Q is a one-step method (qe_population_set_traces)");
    // (the list and the kernel name a cell by its offset in the run's table, an int32; ld >= A)
    if ((double)P.S * (double)e->ld >= 2147483648.0)
        return qe_fail(QE_ERR_UNSUPPORTED, "planning: a run's table must hold fewer than 2^31 cells (state_size * row stride = %lld * %d)",
                       (long long)P.S, (int)e->ld);
    if (P.planning) {  // already on: the model is knowledge and stays
        P.planning = n;
        return QE_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    const size_t m = (size_t)P.runs;
    hipError_t err = P.dyna_entry.ensure(m * (size_t)P.S * (size_t)e->ld);
    if (err == hipSuccess) err = P.dyna_visited.ensure(m * (size_t)P.S * (size_t)e->A);
    if (err == hipSuccess) err = P.dyna_count.ensure(m);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        P.dyna_entry.release(); P.dyna_visited.release(); P.dyna_count.release();
        return qe_fail(err == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_NO_DEVICE, "planning: the model could not be allocated: %s",
                       hipGetErrorString(err));
    }
    if (int rc = model_clear(e)) return rc;
    P.planning = n;
    return QE_OK;
}

int qe_population_planning(qe_engine* e) {
    if (int rc = need_population(e)) return rc;
    return e->pop.planning;
}

int qe_population_model(qe_engine* e, int32_t* next_states, float* rewards, uint8_t* terminated, int32_t* visited, int32_t* count) {
    if (int rc = need_population(e)) return rc;
    PopState& P = e->pop;
    if (!P.planning) return qe_fail(QE_ERR_INVALID, "planning is off (qe_population_set_planning)");
    const size_t m = (size_t)P.runs, S = (size_t)P.S, A = (size_t)e->A, ld = (size_t)e->ld;
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int32_t> hc(m);
    HIP_TRY(hipMemcpyAsync(hc.data(), P.dyna_count.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (next_states || rewards || terminated) {
        std::vector<uint2> he(m * S * ld);
        HIP_TRY(hipMemcpyAsync(he.data(), P.dyna_entry.p, he.size() * sizeof(uint2), hipMemcpyDeviceToHost, e->stream));
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
        HIP_TRY(hipMemcpyAsync(hv.data(), P.dyna_visited.p, hv.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
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
    if (!P.planning) return qe_fail(QE_ERR_INVALID, "planning is off (qe_population_set_planning)");
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
    HIP_TRY(hipMemcpyAsync(P.dyna_entry.p, he.data(), he.size() * sizeof(uint2), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.dyna_visited.p, hv.data(), hv.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(P.dyna_count.p, count, m * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QE_OK;
}

int64_t qe_population_log(qe_engine* e, int64_t cap, int32_t* step, float* ret) {
    if (int rc = need_population(e)) return rc;
    const int64_t n = (int64_t)e->pop.log_step.size();
    for (int64_t k = 0; k < n && k < cap; ++k) {
        if (step) step[k] = e->pop.log_step[(size_t)k];
        if (ret) ret[k] = e->pop.log_ret[(size_t)k];
    }
    return n;
}

}  // extern "C"
