// qe_inst_runs_nstep.hip -- population path, n-step on-policy rules: the k_nstep_rollout instantiations (n-step SARSA and
// n-step Expected SARSA) of ONE (table dtype, environment) pair.  Compiled once per pair (-DQE_INST_T=...
// -DQE_INST_ENV=...), see Makefile; qe_population.hip calls launch_nstep_runs.
#include "qe_host.h"
#include "qe_rollout_nstep.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

static_assert((int)QE_RULE_SARSA == (int)TD_SARSA && (int)QE_RULE_EXPECTED_SARSA == (int)TD_EXPECTED_SARSA,
              "qe_update_rule and TdRule differ");
static_assert(NSTEP_MAX < 32, "kernel_variant carries n in five bits");

// One launch of l.steps steps of every run under `rule` with the windows `w`; the window of a workgroup is dynamic LDS.
// Returns QE_VARIANT_RUNS_NSTEP | rule | NV | masked | n.
template <typename T, class Env>
int64_t launch_nstep_runs(const RunsLaunch<T>& l, int rule, int32_t* pending, const RunWindows& w) {
    const size_t lds = window_lds_bytes(w.n);
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_NSTEP, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        if (rule == QE_RULE_SARSA)
            hipLaunchKernelGGL((k_nstep_rollout<T, Env, decltype(nv)::value, decltype(mk)::value, TD_SARSA>), grid, block, lds, l.stream, l.c, l.ev, l.steps, pending, w);
        else
            hipLaunchKernelGGL((k_nstep_rollout<T, Env, decltype(nv)::value, decltype(mk)::value, TD_EXPECTED_SARSA>), grid, block, lds, l.stream, l.c, l.ev, l.steps,
                               pending, w);
        return ((int64_t)rule << 4) | ((int64_t)w.n << 24);
    });
}

template int64_t launch_nstep_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, int, int32_t*, const RunWindows&);
