// qe_inst_runs_tree.hip -- population path, n-step Tree Backup: the k_tree_rollout instantiations of ONE (table dtype,
// environment) pair.  Compiled once per pair (-DQE_INST_T=... -DQE_INST_ENV=...), see Makefile; qe_population.hip calls
// launch_tree_runs.
#include "qe_host.h"
#include "qe_rollout_tree.h"

#if !defined(QE_INST_T) || !defined(QE_INST_ENV)
#error "compile with -DQE_INST_T=<float|double> -DQE_INST_ENV=<HashEnv|GridEnv|BanditEnv|TttEnv|TableEnv>"
#endif

static_assert(TREE_MAX < 32, "kernel_variant carries n in five bits");

// One launch of l.steps steps of every run with the windows `w`; the window of a workgroup is dynamic LDS.
// Returns QE_VARIANT_RUNS_TREE | NV | masked | n.
template <typename T, class Env>
int64_t launch_tree_runs(const RunsLaunch<T>& l, const RunWindows& w) {
    const size_t lds = window_lds_bytes(w.n);
    return launch_runs_build<Env>(l, QE_VARIANT_RUNS_TREE, [&](auto nv, auto mk, dim3 grid, dim3 block) -> int64_t {
        hipLaunchKernelGGL((k_tree_rollout<T, Env, decltype(nv)::value, decltype(mk)::value>), grid, block, lds, l.stream, l.c, l.ev, l.steps, w);
        return (int64_t)w.n << 24;
    });
}

template int64_t launch_tree_runs<QE_INST_T, QE_INST_ENV>(const RunsLaunch<QE_INST_T>&, const RunWindows&);
