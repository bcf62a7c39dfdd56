// qe_inst_runs_sweep.hip -- population path, prioritized sweeping: the k_sweep_rollout instantiations of ONE (table
// dtype, environment) pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see Makefile;
// qe_population.hip calls launch_sweep_runs.
#include "qe_host.h"
#include "qe_rollout_sweep.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

static_assert(SWEEP_MAX == 32, "kernel_variant carries K - 1 in five bits");
static_assert(QE_VARIANT_SWEEP == 1 << 4, "bit 4 of path 13 is the prioritized order");

// One launch of l.steps steps of every run, each followed by at most w.n planning updates taken from the run's queue.
// Returns QE_VARIANT_RUNS_DYNA | QE_VARIANT_SWEEP | (K - 1) << 5 | NV | masked | n, or QE_ERR_UNSUPPORTED for a build
// that is not compiled (sweep_supported, qe_host.h: the setter has refused the shape before a launch can ask for it).
template <typename T, class Env>
int64_t launch_sweep_runs(const RunsLaunch<T>& l, const DynaModel& w, const SweepState& z) {
    const dim3 grid(grid_for(l.c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    const size_t lds = sweep_lds_bytes(z.K);
    return runs_by_build<Env>(l.ld, l.masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        if constexpr (sweep_supported(sizeof(T) == 4, NV)) {
            hipLaunchKernelGGL((k_sweep_rollout<T, Env, NV, MK>), grid, block, lds, l.stream, l.c, l.ev, l.steps, w, z);
            return QE_VARIANT_RUNS_DYNA | QE_VARIANT_SWEEP | ((int64_t)(z.K - 1) << 5) | ((int64_t)NV << 12) | ((int64_t)MK << 20) |
                   ((int64_t)w.n << 24);
        } else {
            return QE_ERR_UNSUPPORTED;
        }
    });
}

template int64_t launch_sweep_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, const DynaModel&, const SweepState&);
