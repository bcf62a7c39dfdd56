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

// One launch of l.steps steps of every run, each followed by w.n planning updates.  Returns QE_VARIANT_RUNS_DYNA | NV |
// masked | n.
template <typename T, class Env>
int64_t launch_dyna_runs(const RunsLaunch<T>& l, const DynaModel& w) {
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_DYNA, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        hipLaunchKernelGGL((k_dyna_rollout<T, Env, decltype(nv)::value, decltype(mk)::value>), grid, block, 0, l.stream, l.c, l.ev, l.steps, w);
        return (int64_t)w.n << 24;
    });
}

template int64_t launch_dyna_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, const DynaModel&);
