// qe_inst_runs.hip -- population path: the k_rollout_runs and k_evaluate_runs instantiations of ONE (table dtype,
// environment) pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see Makefile; qe_population.hip calls
// launch_runs and launch_evaluate_runs.
#include "qe_host.h"
#include "qe_rollout_runs.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

// One launch of l.steps steps of every run; returns the kernel_variant of the build (QE_VARIANT_RUNS | NV | masked).
template <typename T, class Env>
int64_t launch_runs(const RunsLaunch<T>& l) {
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        hipLaunchKernelGGL((k_rollout_runs<T, Env, decltype(nv)::value, decltype(mk)::value>), grid, block, 0, l.stream, l.c, l.ev, l.steps);
        return 0;
    });
}

// One launch of greedy evaluation (k_evaluate_runs); returns QE_VARIANT_RUNS_EVAL | NV | masked.
template <typename T, class Env>
int64_t launch_evaluate_runs(const RunsLaunch<T>& l, long long episodes, long long* used, uint8_t* done) {
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_EVAL, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        hipLaunchKernelGGL((k_evaluate_runs<T, Env, decltype(nv)::value, decltype(mk)::value>), grid, block, 0, l.stream, l.c, l.ev, l.steps, episodes, used, done);
        return 0;
    });
}

template int64_t launch_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&);
template int64_t launch_evaluate_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, long long, long long*, uint8_t*);
