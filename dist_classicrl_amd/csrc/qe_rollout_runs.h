// qe_rollout_runs.h -- population rollout: M independent single-agent Q-learning runs, ONE RUN PER LANE (gfx950).
//
// Run r owns rows r*S .. r*S+S-1 of one [M*S, ld] table, its own environment state (agent r of the environment), its
// own schedules and discount, and its draws, keyed like every rollout's by the agent's global id (the environment's
// agent_offset + r).
// Nothing is shared between runs, so nothing is ordered: no LDS, no barrier, no atomic -- a lane never waits for another
// lane or workgroup, and occupancy is the only thing that hides the two dependent loads of a step.
//
// Run r after K steps is bit for bit the standalone one-agent rollout (k_rollout_lane with N = 1) on a one-agent
// environment with agent offset agent_offset + r: one step is
//   1. draws of (agent_offset + r, step), step = the launch's step0 + the run's own offset (step_off) + t;
//   2. epsilon-greedy pick (select_lane) from the row of the current state, held in registers;
//   3. Env::step;
//   4. gather of the next state's row: the TD maximum (np.max over its valid columns) and the next pick;
//   5. store of the update of Q[r*S + s, a];
//   6. an own write into that row (s' == s) is patched into the registers: the target above used the old value, the
//      next pick sees the new one -- single_learn's read-then-write order.
// Only the row of the current state is live.  Schedules advance in the lane with the float64 operations of
// schedules/__init__.py; the epsilon threshold is eps_threshold (qe_device.h).
//
// A launch covers `steps` consecutive steps of a call (the host chops calls, see qe_population.hip); per-run state
// (observation, env-internal word, running return, schedule values, episode count and float32 sum of returns) is loaded
// at its start and stored at its end.  Ended episodes go, optionally, into the run's own log segment of `seg_len`
// entries (at most one episode per step, so seg_len >= steps cannot overflow).
#pragma once
#include "qe_rollout_lane.h"

namespace qe {

constexpr int RUNS_BLOCK = 64;  // one wavefront per workgroup: the runs of a small population spread over many CUs

enum RunSchedKind : int32_t { RUN_SCHED_CONSTANT = 0, RUN_SCHED_LINEAR = 1, RUN_SCHED_EXPONENTIAL = 2 };

// One schedule of one run (schedules/__init__.py): constant; linear v <- v + factor; exponential v <- max(v * factor, lo).
struct RunSched {
    double value, min_value, factor;
    int32_t kind, pad;
};

__host__ __device__ __forceinline__ double run_sched_next(double v, double lo, double f, int32_t kind) {
    if (kind == RUN_SCHED_LINEAR) return v + f;
    if (kind == RUN_SCHED_EXPONENTIAL) {
        const double x = v * f;
        return lo > x ? lo : x;  // Python's max(x, lo): the first argument unless the second is larger
    }
    return v;
}

template <typename T>
struct RunsCtx {
    T* q;                 // [M * S, 4 * NV]
    int64_t S, M;
    int32_t* obs;         // environment state of the runs (the environment's agent arrays)
    uint32_t* aux;
    float* acc;
    RunSched* eps;        // [M] descriptors; value advanced in place
    RunSched* lr;
    const double* gamma;  // [M]
    uint32_t* status;     // [M] 1: some step found no selectable action
    long long* ep_count;  // [M] episodes ended in this call
    float* ep_sum;        // [M] their float32 sequential sum
    int32_t* seg_cnt;     // [M] entries of this launch's segment (log only)
    int32_t* seg_step;    // [M * seg_len] step within the call
    float* seg_ret;       // [M * seg_len]
    long long seg_len;    // 0: no log
    uint32_t seed_lo, seed_hi;
    int mode, nan_select;
    unsigned long long step0;  // draw-protocol step of this launch's first step
    long long t_call;          // its index within the call (log entries)
    const unsigned long long* step_off;  // [M] per-run offsets added to step0 (NULL: every run draws at step0 + t)
};

// The windows of all runs between launches (PopState, qe_host.h) and the horizon: what the two multi-step kernels,
// k_nstep_rollout (qe_rollout_nstep.h) and k_tree_rollout (qe_rollout_tree.h), load at launch start and store at its end.
struct RunWindows {
    int32_t n;     // 2 .. NSTEP_MAX, TREE_MAX
    int32_t* len;  // [M] entries of the run's window, <= n - 1
    int32_t* s;    // [(n - 1) * M]: entry i of run r at [i * M + r], oldest first
    int32_t* a;    // Tree Backup: the action | TREE_GREEDY if it was greedy
    float* r;
};

// The dynamic LDS of a workgroup of either kernel: three planes [slot][lane] of n slots.
inline size_t window_lds_bytes(int n) { return (size_t)RUNS_BLOCK * (size_t)n * 12; }

// ---- what every population kernel shares ---------------------------------------------------------------------------
// RunLane is the state one lane carries for its run through a launch, and the ONE copy of the protocol around a
// kernel's own step.  k_rollout_runs and its siblings (qe_rollout_runs_td.h, _double.h, _nstep.h, _trace.h, _dyna.h,
// _visit.h) build their steps from it; what it guarantees:
//   construction   loads the per-run state of run r (the lane is inside the population: r < c.M).  SCHED = false (the
//                  evaluation kernels) leaves c.eps / c.lr / c.gamma unread.
//   draws          the Philox block of (agent_offset + r, step) of a stream; step counts from step0 = the launch's
//                  step0 + the run's own offset (step_off), so a kernel's step t draws at step0 + t.
//   settle         the empty-pick rule: a pick without a selectable action becomes action 0, which keeps the run inside
//                  its table, and the run is flagged -- c.status[r] = 1 at the end of the launch, reported after the call.
//   select, pick, pick_on_policy   the dispatcher's rule for one agent: explore when word 0 of the draws is below
//                  eps_threshold(eps), words 1 and 2 choose the column (select_lane), the NaN rule on when the
//                  population selects NumPy-style; then settle.
//   episode_end    the running return takes the step's reward; a terminated step adds it to the float32 sequential
//                  sum, counts the episode and clears it.  Its log entry is (c.t_call + t, return): the step within the
//                  CALL.  A full segment skips the entry, the episode still counts.
//   next_eps, advance_schedules   the schedules' own float64 operations, once per step.
//   store          writes the state back.  c.seg_cnt[r] only with a log, c.status[r] only when flagged (the host
//                  cleared it before the call).
// The loads of the construction and the stores of store() keep the order they have here: the generated code is
// sensitive to it.  Three kernels keep a line of their own where the shared form costs a build a wave per SIMD: the
// evaluation kernels hold the flag of settle in a local (below), k_visit_rollout patches its two held rows in one
// loop (qe_rollout_visit.h), and k_trace_rollout has its own copy of episode_end (qe_rollout_trace.h).
template <typename T, int NV, bool MASKED, bool SCHED = true>
struct RunLane {
    const RunsCtx<T>& c;
    const int64_t r;
    int32_t n;     // observation
    uint32_t aux;  // environment-internal word
    float acc;     // running return
    RunSched es, ls;
    double eps_v, lr_v;
    Hyper h;  // gamma here; the step sets its rate with learning_rate()
    long long count;
    float sum;
    int32_t logged = 0;
    bool empty = false;
    bool nan_sel;
    uint32_t id;  // the draw key of every rollout: the environment's agent id
    unsigned long long step0;
    long long seg0;  // the run's log segment starts here

    __device__ __forceinline__ RunLane(const RunsCtx<T>& ctx, const EnvCtx& ev, int64_t run) : c(ctx), r(run) {
        n = c.obs[r];
        aux = c.aux[r];
        acc = c.acc[r];
        if constexpr (SCHED) {
            es = c.eps[r]; ls = c.lr[r];
            eps_v = es.value; lr_v = ls.value;
            h.gamma = c.gamma[r]; h.gamma32 = (float)h.gamma;
        }
        count = c.ep_count[r];
        sum = c.ep_sum[r];
        nan_sel = c.nan_select != 0;
        id = ev.agent_offset + (uint32_t)r;
        step0 = c.step0 + (c.step_off ? c.step_off[r] : 0ull);
        seg0 = r * c.seg_len;
    }

    __device__ __forceinline__ U4 draws(unsigned long long step, uint32_t stream = STREAM_POLICY) const {
        return philox4x32_10(id, (uint32_t)step, (uint32_t)(step >> 32), stream, c.seed_lo, c.seed_hi);
    }

    // the empty-pick rule: no selectable action (act < 0) becomes action 0, which keeps the run inside its table; true
    // when it applied -- the run is then reported after the call
    static __device__ __forceinline__ bool settle(int& act) {
        if (act < 0) {
            act = 0;
            return true;
        }
        return false;
    }

    // the pick from a masked row with the draws x in hand; *value = the row's value of the returned action
    template <typename M>
    __device__ __forceinline__ int select(const RowV<T, NV>& rowm, M valid, bool explore, const U4& x, bool row_nan, T* value) {
        int act = select_lane<T, NV, M>(rowm, valid, explore, x.y, x.z, value, nan_sel && row_nan);
        empty |= settle(act);
        return act;
    }

    // the epsilon-greedy pick from the row as loaded, with the draws of `step`
    template <typename M>
    __device__ __forceinline__ int pick(const RowV<T, NV>& row, M valid, bool row_nan, unsigned long long step, double eps, T* value) {
        const U4 x = draws(step);
        const bool explore = (unsigned long long)x.x < eps_threshold(eps);
        return select(masked_row<MASKED>(row, valid), valid, explore, x, row_nan, value);
    }

    // ... of the on-policy kernels, whose *value is the next prediction: a flagged pick hands on row.v[0], the cell of
    // action 0 itself, not its masked value
    template <typename M>
    __device__ __forceinline__ int pick_on_policy(const RowV<T, NV>& row, M valid, bool row_nan, unsigned long long step,
                                                  double eps, T* value) {
        const U4 x = draws(step);
        const bool explore = (unsigned long long)x.x < eps_threshold(eps);
        int act = select_lane<T, NV, M>(masked_row<MASKED>(row, valid), valid, explore, x.y, x.z, value, nan_sel && row_nan);
        if (settle(act)) {
            empty = true;
            *value = row.v[0];
        }
        return act;
    }

    // the episode ends with step t of the launch
    __device__ __forceinline__ void episode_done(long long t) {
        if (logged < c.seg_len) {
            const long long at = seg0 + logged;
            c.seg_step[at] = (int32_t)(c.t_call + t);
            c.seg_ret[at] = acc;
            ++logged;
        }
        sum += acc;
        ++count;
        acc = 0.0f;
    }
    __device__ __forceinline__ void episode_end(const Transition& tr, long long t) {
        acc += tr.reward;
        if (tr.terminated) episode_done(t);
    }

    __device__ __forceinline__ void learning_rate(double lr) { h.lr = lr; h.lr32 = (float)lr; }
    __device__ __forceinline__ double next_eps() const { return run_sched_next(eps_v, es.min_value, es.factor, es.kind); }
    __device__ __forceinline__ void advance_schedules(double eps_next) {
        eps_v = eps_next;
        lr_v = run_sched_next(lr_v, ls.min_value, ls.factor, ls.kind);
    }
    __device__ __forceinline__ void advance_schedules() { advance_schedules(next_eps()); }

    __device__ __forceinline__ void store() const {
        c.obs[r] = n;
        c.aux[r] = aux;
        c.acc[r] = acc;
        if constexpr (SCHED) {
            c.eps[r].value = eps_v;
            c.lr[r].value = lr_v;
        }
        c.ep_count[r] = count;
        c.ep_sum[r] = sum;
        if (c.seg_len) c.seg_cnt[r] = logged;
        if (empty) c.status[r] = 1u;
    }
};

// a store of q1 into column `act` of the row held in registers
template <int NV, typename T>
__device__ __forceinline__ void patch_own_write(RowV<T, NV>& row, int act, T q1) {
#pragma unroll
    for (int j = 0; j < 4 * NV; ++j) row.v[j] = j == act ? q1 : row.v[j];
}

template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_rollout_runs(RunsCtx<T> c, EnvCtx ev, long long steps) {
    using M = typename LaneMask<NV>::type;
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    T* const q = c.q + r * c.S * (4 * NV);
    RunLane<T, NV, MASKED> lane(c, ev, r);

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    bool row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
    for (long long t = 0; t < steps; ++t) {
        const unsigned long long step = lane.step0 + (unsigned long long)t;
        T picked;
        const int act = lane.pick(row, valid, row_nan, step, lane.eps_v, &picked);
        const int32_t s = lane.n;
        const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
        lane.n = tr.next_obs;
        load_row_lane<NV>(row, q, lane.n);
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
        const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
        row_nan = row_nan_lane<NV>(rowm);
        const T m = row_nan ? quiet_nan<T>() : row_max_lane(rowm);
        lane.learning_rate(lane.lr_v);
        T u;
        const T q1 = Td<T>::apply(picked, tr.reward, m, tr.terminated, lane.h, c.mode, &u);
        q[(int64_t)s * (4 * NV) + act] = q1;
        if (lane.n == s) {  // own write lands in the row held in registers
            row_nan |= q1 != q1;
            patch_own_write<NV>(row, act, q1);
        }
        lane.episode_end(tr, t);
        lane.advance_schedules();
    }
    lane.store();
}

// Greedy evaluation of every run (qe_population_evaluate): run r is the standalone one-agent evaluate_steps /
// evaluate_episodes (k_eval with N = 1).  One step is the draws of (agent_offset + r, step), the pick at epsilon 0
// (select_lane with explore = false: the reference's deterministic=True, ties still broken by the draws), Env::step and
// the gather of the next row -- no table store, no TD target, no schedule.  Same launch shape, per-run state and log
// segments as k_rollout_runs; c.eps / c.lr / c.gamma are not read.
//   episodes == 0  step mode: every run takes `steps` steps.
//   episodes > 0   a run stops at the end of the step in which its episode count of the call reaches `episodes`:
//                  done[r] is set and later launches skip the run.  used[r] accumulates the steps it took.
template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_evaluate_runs(RunsCtx<T> c, EnvCtx ev, long long steps, long long episodes,
                                                              long long* used, uint8_t* done) {
    using M = typename LaneMask<NV>::type;
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    if (episodes && done[r]) {  // finished in an earlier launch: an empty log segment, nothing else
        if (c.seg_len) c.seg_cnt[r] = 0;
        return;
    }
    const T* const q = c.q + r * c.S * (4 * NV);
    RunLane<T, NV, MASKED, false> lane(c, ev, r);
    // (the flag of a pick without a selectable action stays a local here and goes to the lane before the store: as a
    // member, written in a loop that a run can leave early, it costs the loop its scalar step counter and registers)
    bool empty = false, finished = false;

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    long long t = 0;
    while (t < steps) {
        const unsigned long long step = lane.step0 + (unsigned long long)t;
        const U4 x = lane.draws(step);
        const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
        T picked;
        int act = select_lane<T, NV, M>(rowm, valid, false, x.y, x.z, &picked, lane.nan_sel && row_nan_lane<NV>(rowm));
        empty |= lane.settle(act);
        const Transition tr = Env::step(ev, r, lane.n, lane.aux, act, step);
        lane.n = tr.next_obs;
        lane.acc += tr.reward;
        ++t;
        if (tr.terminated) {
            lane.episode_done(t - 1);
            if (episodes && lane.count >= episodes) {
                finished = true;
                break;
            }
        }
        load_row_lane<NV>(row, q, lane.n);
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    }
    lane.empty = empty;
    lane.store();
    if (episodes) {
        used[r] += t;
        if (finished) done[r] = 1;
    }
}

}  // namespace qe
