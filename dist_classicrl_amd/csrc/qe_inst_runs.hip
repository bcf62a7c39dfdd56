// qe_inst_runs.hip -- population path: the k_rollout_runs and k_evaluate_runs instantiations of ONE (table dtype,
// environment) pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see Makefile; qe_population.hip calls
// launch_runs and launch_evaluate_runs.
#include "qe_host.h"
#include "qe_rollout_runs.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

// One launch of `steps` steps of every run; returns the kernel_variant of the build (QE_VARIANT_RUNS | NV | masked).
template <typename T, class Env>
int64_t launch_runs(hipStream_t stream, const RunsCtx<T>& c, const EnvCtx& ev, int ld, bool masked, long long steps) {
    const dim3 grid(grid_for(c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(ld, masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        hipLaunchKernelGGL((k_rollout_runs<T, Env, NV, MK>), grid, block, 0, stream, c, ev, steps);
        return QE_VARIANT_RUNS | ((int64_t)NV << 12) | ((int64_t)MK << 20);
    });
}

// One launch of greedy evaluation (k_evaluate_runs); returns QE_VARIANT_RUNS_EVAL | NV | masked.
template <typename T, class Env>
int64_t launch_evaluate_runs(hipStream_t stream, const RunsCtx<T>& c, const EnvCtx& ev, int ld, bool masked, long long steps,
                             long long episodes, long long* used, uint8_t* done) {
    const dim3 grid(grid_for(c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(ld, masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        hipLaunchKernelGGL((k_evaluate_runs<T, Env, NV, MK>), grid, block, 0, stream, c, ev, steps, episodes, used, done);
        return QE_VARIANT_RUNS_EVAL | ((int64_t)NV << 12) | ((int64_t)MK << 20);
    });
}

template int64_t launch_runs<QE_INST_T, QE_INST_ENV>(hipStream_t, const RunsCtx<QE_INST_T>&, const EnvCtx&, int, bool, long long);
template int64_t launch_evaluate_runs<QE_INST_T, QE_INST_ENV>(hipStream_t, const RunsCtx<QE_INST_T>&, const EnvCtx&, int, bool,
                                                              long long, long long, long long*, uint8_t*);
