// qe_inst_runs_visit.hip -- population path, visit counts: the k_visit_rollout instantiations of ONE (table dtype,
// environment) pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see Makefile; qe_population.hip calls
// launch_visit_runs (and launches the fill kernel of the bonus plane itself).
#include "qe_host.h"
#include "qe_rollout_visit.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

// One launch of l.steps steps of every run.  Returns QE_VARIANT_RUNS_VISIT | NV | masked | visit_lr << 4 | (some beta
// > 0) << 5, or QE_ERR_UNSUPPORTED for a build that is not compiled (visit_supported, qe_host.h: the setter has refused
// the shape before a launch can ask for it).
template <typename T, class Env>
int64_t launch_visit_runs(const RunsLaunch<T>& l, const VisitPlanes& w, bool any_bonus) {
    const dim3 grid(grid_for(l.c.M, RUNS_BLOCK)), block(RUNS_BLOCK);
    return runs_by_build<Env>(l.ld, l.masked, [&](auto nv, auto mk) -> int64_t {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MK = decltype(mk)::value;
        if constexpr (visit_supported(sizeof(T) == 4, NV)) {
            hipLaunchKernelGGL((k_visit_rollout<T, Env, NV, MK>), grid, block, 0, l.stream, l.c, l.ev, l.steps, w);
            return QE_VARIANT_RUNS_VISIT | (w.visit_lr ? 1 << 4 : 0) | (any_bonus ? 1 << 5 : 0) | ((int64_t)NV << 12) | ((int64_t)MK << 20);
        } else {
            return QE_ERR_UNSUPPORTED;
        }
    });
}

template int64_t launch_visit_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, const VisitPlanes&, bool);
