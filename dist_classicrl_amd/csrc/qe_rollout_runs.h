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

template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_rollout_runs(RunsCtx<T> c, EnvCtx ev, long long steps) {
    using M = typename LaneMask<NV>::type;
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    T* const q = c.q + r * c.S * (4 * NV);
    int32_t n = c.obs[r];
    uint32_t aux = c.aux[r];
    float acc = c.acc[r];
    const RunSched es = c.eps[r], ls = c.lr[r];
    double eps_v = es.value, lr_v = ls.value;
    Hyper h;
    h.gamma = c.gamma[r]; h.gamma32 = (float)h.gamma;
    long long count = c.ep_count[r];
    float sum = c.ep_sum[r];
    int32_t logged = 0;
    bool empty = false;
    const bool nan_sel = c.nan_select != 0;
    const uint32_t id = ev.agent_offset + (uint32_t)r;  // the draw key of every rollout: the environment's agent id
    const unsigned long long step0 = c.step0 + (c.step_off ? c.step_off[r] : 0ull);

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, n);
    bool row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
    for (long long t = 0; t < steps; ++t) {
        const unsigned long long step = step0 + (unsigned long long)t;
        const U4 x = philox4x32_10(id, (uint32_t)step, (uint32_t)(step >> 32), STREAM_POLICY, c.seed_lo, c.seed_hi);
        const bool explore = (unsigned long long)x.x < eps_threshold(eps_v);
        T picked;
        int act = select_lane<T, NV, M>(masked_row<MASKED>(row, valid), valid, explore, x.y, x.z, &picked, nan_sel && row_nan);
        if (act < 0) {  // no selectable action: reported after the call, action 0 keeps the run inside its table
            empty = true;
            act = 0;
        }
        const int32_t s = n;
        const Transition tr = Env::step(ev, r, s, aux, act, step);
        n = tr.next_obs;
        load_row_lane<NV>(row, q, n);
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, n);
        const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
        row_nan = row_nan_lane<NV>(rowm);
        const T m = row_nan ? quiet_nan<T>() : row_max_lane(rowm);
        h.lr = lr_v; h.lr32 = (float)lr_v;
        T u;
        const T q1 = Td<T>::apply(picked, tr.reward, m, tr.terminated, h, c.mode, &u);
        q[(int64_t)s * (4 * NV) + act] = q1;
        if (n == s) {  // own write lands in the row held in registers
            row_nan |= q1 != q1;
#pragma unroll
            for (int j = 0; j < 4 * NV; ++j) row.v[j] = j == act ? q1 : row.v[j];
        }
        acc += tr.reward;
        if (tr.terminated) {
            if (logged < c.seg_len) {
                c.seg_step[r * c.seg_len + logged] = (int32_t)(c.t_call + t);
                c.seg_ret[r * c.seg_len + logged] = acc;
                ++logged;
            }
            sum += acc;
            ++count;
            acc = 0.0f;
        }
        eps_v = run_sched_next(eps_v, es.min_value, es.factor, es.kind);
        lr_v = run_sched_next(lr_v, ls.min_value, ls.factor, ls.kind);
    }
    c.obs[r] = n;
    c.aux[r] = aux;
    c.acc[r] = acc;
    c.eps[r].value = eps_v;
    c.lr[r].value = lr_v;
    c.ep_count[r] = count;
    c.ep_sum[r] = sum;
    if (c.seg_len) c.seg_cnt[r] = logged;
    if (empty) c.status[r] = 1u;
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
    int32_t n = c.obs[r];
    uint32_t aux = c.aux[r];
    float acc = c.acc[r];
    long long count = c.ep_count[r];
    float sum = c.ep_sum[r];
    int32_t logged = 0;
    bool empty = false, finished = false;
    const bool nan_sel = c.nan_select != 0;
    const uint32_t id = ev.agent_offset + (uint32_t)r;
    const unsigned long long step0 = c.step0 + (c.step_off ? c.step_off[r] : 0ull);

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, n);
    long long t = 0;
    while (t < steps) {
        const unsigned long long step = step0 + (unsigned long long)t;
        const U4 x = philox4x32_10(id, (uint32_t)step, (uint32_t)(step >> 32), STREAM_POLICY, c.seed_lo, c.seed_hi);
        const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
        T picked;
        int act = select_lane<T, NV, M>(rowm, valid, false, x.y, x.z, &picked, nan_sel && row_nan_lane<NV>(rowm));
        if (act < 0) {  // no selectable action: reported after the call, action 0 keeps the run inside its table
            empty = true;
            act = 0;
        }
        const Transition tr = Env::step(ev, r, n, aux, act, step);
        n = tr.next_obs;
        acc += tr.reward;
        ++t;
        if (tr.terminated) {
            if (logged < c.seg_len) {
                c.seg_step[r * c.seg_len + logged] = (int32_t)(c.t_call + t - 1);
                c.seg_ret[r * c.seg_len + logged] = acc;
                ++logged;
            }
            sum += acc;
            ++count;
            acc = 0.0f;
            if (episodes && count >= episodes) {
                finished = true;
                break;
            }
        }
        load_row_lane<NV>(row, q, n);
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, n);
    }
    c.obs[r] = n;
    c.aux[r] = aux;
    c.acc[r] = acc;
    c.ep_count[r] = count;
    c.ep_sum[r] = sum;
    if (c.seg_len) c.seg_cnt[r] = logged;
    if (empty) c.status[r] = 1u;
    if (episodes) {
        used[r] += t;
        if (finished) done[r] = 1;
    }
}

}  // namespace qe
