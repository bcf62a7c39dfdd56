// qe_inst_runs_dyna_sample.hip -- population path, Dyna-Q over a sample model: the k_dyna_sample_rollout instantiations
// of ONE (table dtype, environment) pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see Makefile;
// qe_population.hip calls launch_dyna_sample_runs.
#include "qe_host.h"
#include "qe_rollout_dyna_sample.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

static_assert(DYNA_OUTCOMES_MAX == 8, "kernel_variant carries K - 1 in three bits");
static_assert((QE_VARIANT_OUTCOMES_SHIFT == 21), "bits 21-23 of path 13 hold K - 1");

// One launch of l.steps steps of every run, each followed by w.n planning updates over the sample model.  Returns
// QE_VARIANT_RUNS_DYNA | (K - 1) << 21 | NV | masked | n, or QE_ERR_UNSUPPORTED for a build that is not compiled
// (dyna_sample_supported, qe_host.h: the setter has refused the shape before a launch can ask for it).
template <typename T, class Env>
int64_t launch_dyna_sample_runs(const RunsLaunch<T>& l, const SampleModel& w) {
    const dim3 grid(grid_for(l.c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(l.ld, l.masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        if constexpr (dyna_sample_supported(sizeof(T) == 4, NV)) {
            hipLaunchKernelGGL((k_dyna_sample_rollout<T, Env, NV, MK>), grid, block, 0, l.stream, l.c, l.ev, l.steps, w);
            return QE_VARIANT_RUNS_DYNA | ((int64_t)(w.K - 1) << QE_VARIANT_OUTCOMES_SHIFT) | ((int64_t)NV << 12) | ((int64_t)MK << 20) |
                   ((int64_t)w.n << 24);
        } else {
            return QE_ERR_UNSUPPORTED;
        }
    });
}

template int64_t launch_dyna_sample_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, const SampleModel&);
