// qe_inst_runs_trace.hip -- population path, eligibility traces: the k_trace_rollout instantiations (SARSA(lambda) and
// Watkins's Q(lambda)) of ONE (table dtype, environment) pair.  Compiled once per pair (-DQE_INST_T=...
// -DQE_INST_ENV=...), see Makefile; qe_population.hip calls launch_trace_runs.
#include "qe_host.h"
#include "qe_rollout_trace.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

static_assert((int)QE_RULE_Q_LEARNING == (int)TD_Q_LEARNING && (int)QE_RULE_SARSA == (int)TD_SARSA, "qe_update_rule and TdRule differ");
static_assert((int)QE_TRACE_REPLACING == (int)TRACE_REPLACING && (int)QE_TRACE_ACCUMULATING == (int)TRACE_ACCUMULATING,
              "qe_trace_kind and TraceKind differ");
static_assert(TRACE_MAX < 64, "kernel_variant carries K in six bits");

// One launch of `steps` steps of every run under `rule` with the trace slots `w`; the slots of a workgroup are dynamic
// LDS.  Returns QE_VARIANT_RUNS_TRACE | rule | NV | masked | K | kind.
template <typename T, class Env>
int64_t launch_trace_runs(hipStream_t stream, const RunsCtx<T>& c, const EnvCtx& ev, int ld, bool masked, long long steps, int rule,
                          int32_t* pending, const TraceSlots<T>& w) {
    const dim3 grid(grid_for(c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    const size_t lds = trace_lds_bytes(w.K, sizeof(T));
    return runs_by_build<Env>(ld, masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        if (rule == QE_RULE_SARSA)
            hipLaunchKernelGGL((k_trace_rollout<T, Env, NV, MK, TD_SARSA>), grid, block, lds, stream, c, ev, steps, pending, w);
        else
            hipLaunchKernelGGL((k_trace_rollout<T, Env, NV, MK, TD_Q_LEARNING>), grid, block, lds, stream, c, ev, steps, pending,
                               w);
        return QE_VARIANT_RUNS_TRACE | ((int64_t)rule << 4) | ((int64_t)NV << 12) | ((int64_t)MK << 20) | ((int64_t)w.K << 24) |
               ((int64_t)w.kind << 30);
    });
}

template int64_t launch_trace_runs<QE_INST_T, QE_INST_ENV>(hipStream_t, const RunsCtx<QE_INST_T>&, const EnvCtx&, int, bool,
                                                           long long, int, int32_t*, const TraceSlots<QE_INST_T>&);
