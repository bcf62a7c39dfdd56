// qe_inst_runs_double.hip -- population path, double estimator (Double Q-learning): the k_double_rollout and
// k_double_evaluate instantiations of ONE (table dtype, environment) pair.  Compiled once per pair (-DQE_INST_T=...
// -DQE_INST_ENV=...), see Makefile; qe_population.hip calls launch_double_runs and launch_double_evaluate.
#include "qe_host.h"
#include "qe_rollout_double.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

// One launch of `steps` steps of every run, second table `table_b`; returns QE_VARIANT_RUNS_DOUBLE | NV | masked.
template <typename T, class Env>
int64_t launch_double_runs(hipStream_t stream, const RunsCtx<T>& c, const EnvCtx& ev, int ld, bool masked, long long steps,
                           T* table_b) {
    const dim3 grid(grid_for(c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(ld, masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        hipLaunchKernelGGL((k_double_rollout<T, Env, NV, MK>), grid, block, 0, stream, c, ev, steps, table_b);
        return QE_VARIANT_RUNS_DOUBLE | ((int64_t)NV << 12) | ((int64_t)MK << 20);
    });
}

// One launch of its greedy evaluation (k_double_evaluate); returns QE_VARIANT_RUNS_DOUBLE_EVAL | NV | masked.
template <typename T, class Env>
int64_t launch_double_evaluate(hipStream_t stream, const RunsCtx<T>& c, const EnvCtx& ev, int ld, bool masked, long long steps,
                               long long episodes, long long* used, uint8_t* done, const T* table_b) {
    const dim3 grid(grid_for(c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(ld, masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        hipLaunchKernelGGL((k_double_evaluate<T, Env, NV, MK>), grid, block, 0, stream, c, ev, steps, episodes, used, done,
                           table_b);
        return QE_VARIANT_RUNS_DOUBLE_EVAL | ((int64_t)NV << 12) | ((int64_t)MK << 20);
    });
}

template int64_t launch_double_runs<QE_INST_T, QE_INST_ENV>(hipStream_t, const RunsCtx<QE_INST_T>&, const EnvCtx&, int, bool,
                                                            long long, QE_INST_T*);
template int64_t launch_double_evaluate<QE_INST_T, QE_INST_ENV>(hipStream_t, const RunsCtx<QE_INST_T>&, const EnvCtx&, int, bool,
                                                                long long, long long, long long*, uint8_t*, const QE_INST_T*);
