// qe_mdp_solve.hip -- exact solution of a QE_ENV_TABLE environment's MDP and exact values of a population's greedy
// policies (include/qlearn_engine.h, "dynamic programming"): the instantiations of the kernels of qe_mdp_solve.h, one per
// record count K = 1 .. 8 (and per table dtype for the tie sets), and the two entry points that drive them.  Sweeps are
// enqueued MDP_BATCH at a time on the engine's stream; the host reads the residual words (value iteration) or the done
// flags (policy values) once per batch.  Every buffer lives for one call.
#include "qe_host.h"
#include "qe_mdp_solve.h"

namespace {

// a call's device buffers: released however the call ends
template <typename U>
struct CallBuf : DevBuf<U> {
    ~CallBuf() { this->release(); }
};

template <class F>
int by_records(int k, F f) {
    switch (k) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
    }
    return qe_fail(QE_ERR_INVALID, "k = %d outcome slots: must be 1 .. 8", k);
}

int check_sweep_args(double tol, int32_t max_sweeps) {
    if (!(tol >= 0.0) || !std::isfinite(tol)) return qe_fail(QE_ERR_INVALID, "tol must be finite and >= 0 (have %g)", tol);
    if (max_sweeps < 1) return qe_fail(QE_ERR_INVALID, "max_sweeps must be in 1 .. 2^31 - 1 (have %d)", (int)max_sweeps);
    return QE_OK;
}

int check_gamma(double gamma, long long run) {
    if (gamma >= 0.0 && gamma <= 1.0) return QE_OK;
    if (run < 0) return qe_fail(QE_ERR_INVALID, "gamma must be a finite number in [0, 1] (have %g)", gamma);
    return qe_fail(QE_ERR_INVALID, "run %lld: gamma must be a finite number in [0, 1] (have %g)", run, gamma);
}

// the table environment of a live engine, else the status to return
int need_table_env(const qe_env* env) {
    if (!env) return qe_fail(QE_ERR_INVALID, "env is NULL");
    if (!env->e) return qe_fail(QE_ERR_INVALID, "the environment's engine has been destroyed");
    if (env->p.kind != QE_ENV_TABLE)
        return qe_fail(QE_ERR_UNSUPPORTED, "dynamic programming needs a QE_ENV_TABLE environment (have kind %d)", (int)env->p.kind);
    // (not a narrower limit than the environment's: qe_env_create_table already refuses rows wider than 256, so this
    // cannot fire today -- it only keeps "a workgroup holds a whole row" next to the code that relies on it)
    if (env->e->A > MDP_BLOCK)
        return qe_fail(QE_ERR_UNSUPPORTED, "dynamic programming supports action_size <= %d (have %d)", MDP_BLOCK, (int)env->e->A);
    return QE_OK;
}

}  // namespace

extern "C" {

int qe_env_table_solve(qe_env* env, double gamma, double tol, int32_t max_sweeps, double* q_out, double* v_out,
                       int32_t* sweeps_out, double* residual_out) {
    if (int rc = need_table_env(env)) return rc;
    if (int rc = check_gamma(gamma, -1)) return rc;
    if (int rc = check_sweep_args(tol, max_sweeps)) return rc;
    qe_engine* e = env->e;
    HIP_TRY(hipSetDevice(e->device));
    const int64_t S = env_states(e);
    const int A = e->A, K = env->tbl_k;
    const size_t s = (size_t)S, cells = s * (size_t)A;
    const int rpb = MDP_BLOCK / A;
    const unsigned grid = (unsigned)((S + rpb - 1) / rpb);
    const uint4* rec = (const uint4*)env->tbl_rec.p;
    const uint32_t* mask = env->p.masked ? env->tbl_mask.p : nullptr;
    const int n_words = (A + 31) / 32;
    CallBuf<double> v[2], q;
    CallBuf<unsigned long long> res;
    HIP_TRY(v[0].ensure(s)); HIP_TRY(v[1].ensure(s)); HIP_TRY(res.ensure(MDP_BATCH));
    if (q_out) HIP_TRY(q.ensure(cells));
    HIP_TRY(hipMemsetAsync(v[0].p, 0, s * sizeof(double), e->stream));  // V_0 = 0
    unsigned long long h_res[MDP_BATCH];
    int32_t t = 0;  // sweeps made
    double residual = 0.0;
    bool stopped = false;
    while (!stopped && t < max_sweeps) {
        const int n = (int)std::min<int64_t>(MDP_BATCH, (int64_t)max_sweeps - t);
        HIP_TRY(hipMemsetAsync(res.p, 0, MDP_BATCH * sizeof(unsigned long long), e->stream));
        const int rc = by_records(K, [&](auto kk) -> int {
            constexpr int KK = decltype(kk)::value;
            for (int i = 0; i < n; ++i) {
                const int32_t sweep = t + i + 1;  // reads V_{sweep - 1}, writes V_sweep into the buffer of its parity
                hipLaunchKernelGGL((k_mdp_value_sweep<KK>), dim3(grid), dim3(MDP_BLOCK), 0, e->stream, rec, mask, n_words, S, A,
                                   rpb, (const double*)v[(sweep - 1) & 1].p, v[sweep & 1].p, gamma, tol,
                                   i ? (const unsigned long long*)(res.p + i - 1) : nullptr, res.p + i);
            }
            return QE_OK;
        });
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_res, res.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        int made = n;
        for (int i = 0; i < n; ++i) {
            double x;
            memcpy(&x, &h_res[i], sizeof x);
            if (x <= tol) { made = i + 1; stopped = true; break; }
        }
        memcpy(&residual, &h_res[made - 1], sizeof residual);
        t += made;
    }
    if (q_out) {  // Q_t from V_{t-1}, which the sweeps behind t have left alone
        const int rc = by_records(K, [&](auto kk) -> int {
            constexpr int KK = decltype(kk)::value;
            hipLaunchKernelGGL((k_mdp_q_values<KK>), dim3(grid_for((int64_t)cells, MDP_BLOCK)), dim3(MDP_BLOCK), 0, e->stream, rec,
                               (int64_t)cells, (const double*)v[(t - 1) & 1].p, gamma, q.p);
            return QE_OK;
        });
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(q_out, q.p, cells * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    }
    if (v_out) HIP_TRY(hipMemcpyAsync(v_out, v[t & 1].p, s * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (sweeps_out) *sweeps_out = t;
    if (residual_out) *residual_out = residual;
    return stopped ? 1 : 0;
}

int qe_population_policy_values(qe_engine* e, qe_env* env, const double* gammas, double tol, int32_t max_sweeps, double* v_out,
                                int32_t* sweeps_out, double* residual_out, uint32_t* status_out) {
    if (!e) return qe_fail(QE_ERR_INVALID, "engine is NULL");
    if (!e->pop.runs) return qe_fail(QE_ERR_INVALID, "not a population engine (qe_create_population)");
    if (int rc = need_table_env(env)) return rc;
    if (env->e != e) return qe_fail(QE_ERR_INVALID, "engine/env mismatch");
    if (e->A > 64 || e->ld > 64) return qe_fail(QE_ERR_UNSUPPORTED, "a population holds rows of at most 64 actions");
    if (int rc = check_sweep_args(tol, max_sweeps)) return rc;
    PopState& P = e->pop;
    const int64_t M = P.runs, S = P.S, rows = M * S;
    const size_t m = (size_t)M, cells = (size_t)rows;
    for (size_t r = 0; gammas && r < m; ++r)
        if (int rc = check_gamma(gammas[r], (long long)r)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const int A = e->A, K = env->tbl_k;
    const int rpb = MDP_BLOCK / A;
    const unsigned grid = (unsigned)((rows + rpb - 1) / rpb), grid_runs = grid_for(M, MDP_BLOCK), grid_rows = grid_for(rows, MDP_BLOCK);
    const uint4* rec = (const uint4*)env->tbl_rec.p;
    const uint32_t* mask = env->p.masked ? env->tbl_mask.p : nullptr;
    const int n_words = (A + 31) / 32;
    CallBuf<double> v[2], out, gam, residual;
    CallBuf<unsigned long long> gmask, res;
    CallBuf<uint32_t> status;
    CallBuf<int32_t> sweeps;
    CallBuf<uint8_t> done;
    HIP_TRY(v[0].ensure(cells)); HIP_TRY(v[1].ensure(cells)); HIP_TRY(out.ensure(cells)); HIP_TRY(gmask.ensure(cells));
    HIP_TRY(res.ensure((size_t)MDP_BATCH * m)); HIP_TRY(status.ensure(m)); HIP_TRY(sweeps.ensure(m)); HIP_TRY(done.ensure(m));
    HIP_TRY(residual.ensure(m));
    const double* d_gamma = P.gamma.p;  // the runs' own discounts
    if (gammas) {
        HIP_TRY(gam.ensure(m));
        HIP_TRY(hipMemcpyAsync(gam.p, gammas, m * sizeof(double), hipMemcpyHostToDevice, e->stream));
        d_gamma = gam.p;
    }
    HIP_TRY(hipMemsetAsync(v[0].p, 0, cells * sizeof(double), e->stream));  // V_0 = 0
    HIP_TRY(hipMemsetAsync(status.p, 0, m * sizeof(uint32_t), e->stream));
    if (e->dtype == QE_F32)
        hipLaunchKernelGGL((k_mdp_tie_sets<float>), dim3(grid_rows), dim3(MDP_BLOCK), 0, e->stream, (const float*)e->q,
                           (const float*)P.table_b, (int)e->ld, mask, n_words, rows, S, A, gmask.p, status.p);
    else
        hipLaunchKernelGGL((k_mdp_tie_sets<double>), dim3(grid_rows), dim3(MDP_BLOCK), 0, e->stream, (const double*)e->q,
                           (const double*)P.table_b, (int)e->ld, mask, n_words, rows, S, A, gmask.p, status.p);
    hipLaunchKernelGGL(k_mdp_policy_begin, dim3(grid_runs), dim3(MDP_BLOCK), 0, e->stream, (const uint32_t*)status.p, M, done.p,
                       sweeps.p, residual.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> h_done(m);
    bool all_done = false;
    for (int32_t t = 0; !all_done && t < max_sweeps;) {
        const int n = (int)std::min<int64_t>(MDP_BATCH, (int64_t)max_sweeps - t);
        HIP_TRY(hipMemsetAsync(res.p, 0, (size_t)MDP_BATCH * m * sizeof(unsigned long long), e->stream));
        const int rc = by_records(K, [&](auto kk) -> int {
            constexpr int KK = decltype(kk)::value;
            for (int i = 0; i < n; ++i) {
                const int32_t sweep = t + i + 1;
                hipLaunchKernelGGL((k_mdp_policy_sweep<KK>), dim3(grid), dim3(MDP_BLOCK), 0, e->stream, rec,
                                   (const unsigned long long*)gmask.p, rows, S, A, rpb, (const double*)v[(sweep - 1) & 1].p,
                                   v[sweep & 1].p, d_gamma, tol, (const uint8_t*)done.p,
                                   i ? (const unsigned long long*)(res.p + (size_t)(i - 1) * m) : nullptr, res.p + (size_t)i * m);
            }
            return QE_OK;
        });
        if (rc) return rc;
        hipLaunchKernelGGL(k_mdp_policy_batch_end, dim3(grid_runs), dim3(MDP_BLOCK), 0, e->stream, (const unsigned long long*)res.p,
                           n, M, tol, t, done.p, sweeps.p, residual.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_done.data(), done.p, m, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        all_done = std::all_of(h_done.begin(), h_done.end(), [](uint8_t d) { return d != 0; });
        t += n;
    }
    hipLaunchKernelGGL(k_mdp_policy_collect, dim3(grid_rows), dim3(MDP_BLOCK), 0, e->stream, (const double*)v[0].p,
                       (const double*)v[1].p, (const int32_t*)sweeps.p, (const uint32_t*)status.p, rows, S, out.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> h_status(m);
    if (v_out) HIP_TRY(hipMemcpyAsync(v_out, out.p, cells * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (sweeps_out) HIP_TRY(hipMemcpyAsync(sweeps_out, sweeps.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (residual_out) HIP_TRY(hipMemcpyAsync(residual_out, residual.p, m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(h_status.data(), status.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(h_done.data(), done.p, m, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (status_out) memcpy(status_out, h_status.data(), m * sizeof(uint32_t));
    int converged = 0;
    for (size_t r = 0; r < m; ++r) converged += h_done[r] && !(h_status[r] & MDP_STATUS_NAN);
    return converged;
}

}  // extern "C"
