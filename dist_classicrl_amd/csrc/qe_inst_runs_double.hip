// qe_inst_runs_double.hip -- population path, double estimator (Double Q-learning): the k_double_rollout and
// k_double_evaluate instantiations of ONE (table dtype, environment) pair.  Compiled once per pair (-DQE_INST_T=...
// -DQE_INST_ENV=...), see Makefile; qe_population.hip calls launch_double_runs and launch_double_evaluate.
#include "qe_host.h"
#include "qe_rollout_double.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

// One launch of l.steps steps of every run, second table `table_b`; returns QE_VARIANT_RUNS_DOUBLE | NV | masked.
template <typename T, class Env>
int64_t launch_double_runs(const RunsLaunch<T>& l, T* table_b) {
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_DOUBLE, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        hipLaunchKernelGGL((k_double_rollout<T, Env, decltype(nv)::value, decltype(mk)::value>), grid, block, 0, l.stream, l.c, l.ev, l.steps, table_b);
        return 0;
    });
}

// One launch of its greedy evaluation (k_double_evaluate); returns QE_VARIANT_RUNS_DOUBLE_EVAL | NV | masked.
template <typename T, class Env>
int64_t launch_double_evaluate(const RunsLaunch<T>& l, long long episodes, long long* used, uint8_t* done, const T* table_b) {
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_DOUBLE_EVAL, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        hipLaunchKernelGGL((k_double_evaluate<T, Env, decltype(nv)::value, decltype(mk)::value>), grid, block, 0, l.stream, l.c, l.ev, l.steps, episodes, used, done,
                           table_b);
        return 0;
    });
}

template int64_t launch_double_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, QE_INST_T*);
template int64_t launch_double_evaluate<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, long long, long long*, uint8_t*,
                                                                const QE_INST_T*);
