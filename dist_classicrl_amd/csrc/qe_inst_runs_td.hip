// qe_inst_runs_td.hip -- population path, on-policy update rules: the k_rollout_runs_td instantiations (SARSA and
// Expected SARSA) of ONE (table dtype, environment) pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see
// Makefile; qe_population.hip calls launch_runs_td.
#include "qe_host.h"
#include "qe_rollout_runs_td.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

static_assert((int)QE_RULE_SARSA == (int)TD_SARSA && (int)QE_RULE_EXPECTED_SARSA == (int)TD_EXPECTED_SARSA,
              "qe_update_rule and TdRule differ");

// One launch of l.steps steps of every run under `rule`; returns QE_VARIANT_RUNS_TD | rule | NV | masked.
template <typename T, class Env>
int64_t launch_runs_td(const RunsLaunch<T>& l, int rule, int32_t* pending) {
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_TD, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        if (rule == QE_RULE_SARSA)
            hipLaunchKernelGGL((k_rollout_runs_td<T, Env, decltype(nv)::value, decltype(mk)::value, TD_SARSA>), grid, block, 0, l.stream, l.c, l.ev, l.steps, pending);
        else
            hipLaunchKernelGGL((k_rollout_runs_td<T, Env, decltype(nv)::value, decltype(mk)::value, TD_EXPECTED_SARSA>), grid, block, 0, l.stream, l.c, l.ev, l.steps,
                               pending);
        return (int64_t)rule << 4;
    });
}

template int64_t launch_runs_td<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, int, int32_t*);
