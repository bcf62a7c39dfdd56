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

// One launch of `steps` steps of every run under `rule`; returns QE_VARIANT_RUNS_TD | rule | NV | masked.
template <typename T, class Env>
int64_t launch_runs_td(hipStream_t stream, const RunsCtx<T>& c, const EnvCtx& ev, int ld, bool masked, long long steps, int rule,
                       int32_t* pending) {
    const dim3 grid(grid_for(c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(ld, masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        if (rule == QE_RULE_SARSA)
            hipLaunchKernelGGL((k_rollout_runs_td<T, Env, NV, MK, TD_SARSA>), grid, block, 0, stream, c, ev, steps, pending);
        else
            hipLaunchKernelGGL((k_rollout_runs_td<T, Env, NV, MK, TD_EXPECTED_SARSA>), grid, block, 0, stream, c, ev, steps,
                               pending);
        return QE_VARIANT_RUNS_TD | ((int64_t)rule << 4) | ((int64_t)NV << 12) | ((int64_t)MK << 20);
    });
}

template int64_t launch_runs_td<QE_INST_T, QE_INST_ENV>(hipStream_t, const RunsCtx<QE_INST_T>&, const EnvCtx&, int, bool, long long,
                                                        int, int32_t*);
