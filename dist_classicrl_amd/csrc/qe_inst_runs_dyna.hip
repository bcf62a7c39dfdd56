// qe_inst_runs_dyna.hip -- population path, Dyna-Q: the k_dyna_rollout instantiations of ONE (table dtype, environment)
// pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see Makefile; qe_population.hip calls
// launch_dyna_runs.
#include "qe_host.h"
#include "qe_rollout_dyna.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

static_assert(DYNA_MAX < 128, "kernel_variant carries n in seven bits");
static_assert(DYNA_BATCH == 4, "a group of planning updates is one Philox block");

// One launch of `steps` steps of every run, each followed by w.n planning updates.  Returns QE_VARIANT_RUNS_DYNA | NV |
// masked | n.
template <typename T, class Env>
int64_t launch_dyna_runs(hipStream_t stream, const RunsCtx<T>& c, const EnvCtx& ev, int ld, bool masked, long long steps,
                         const DynaModel& w) {
    const dim3 grid(grid_for(c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(ld, masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        hipLaunchKernelGGL((k_dyna_rollout<T, Env, NV, MK>), grid, block, 0, stream, c, ev, steps, w);
        return QE_VARIANT_RUNS_DYNA | ((int64_t)NV << 12) | ((int64_t)MK << 20) | ((int64_t)w.n << 24);
    });
}

template int64_t launch_dyna_runs<QE_INST_T, QE_INST_ENV>(hipStream_t, const RunsCtx<QE_INST_T>&, const EnvCtx&, int, bool,
                                                          long long, const DynaModel&);
