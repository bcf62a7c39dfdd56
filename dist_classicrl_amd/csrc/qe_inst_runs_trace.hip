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

// One launch of l.steps steps of every run under `rule` with the trace slots `w`; the slots of a workgroup are dynamic
// LDS.  Returns QE_VARIANT_RUNS_TRACE | rule | NV | masked | K | kind.
template <typename T, class Env>
int64_t launch_trace_runs(const RunsLaunch<T>& l, int rule, int32_t* pending, const TraceSlots<T>& w) {
    const size_t lds = trace_lds_bytes(w.K, sizeof(T));
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_TRACE, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        if (rule == QE_RULE_SARSA)
            hipLaunchKernelGGL((k_trace_rollout<T, Env, decltype(nv)::value, decltype(mk)::value, TD_SARSA>), grid, block, lds, l.stream, l.c, l.ev, l.steps, pending, w);
        else
            hipLaunchKernelGGL((k_trace_rollout<T, Env, decltype(nv)::value, decltype(mk)::value, TD_Q_LEARNING>), grid, block, lds, l.stream, l.c, l.ev, l.steps, pending,
                               w);
        return ((int64_t)rule << 4) | ((int64_t)w.K << 24) | ((int64_t)w.kind << 30);
    });
}

template int64_t launch_trace_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, int, int32_t*, const TraceSlots<QE_INST_T>&);
