// qe_rollout_runs_td.h -- population rollout with an on-policy update rule: SARSA and Expected SARSA (gfx950).
//
// The sibling of k_rollout_runs (qe_rollout_runs.h): one run per lane, the same launch shape, per-run state, draws, log
// segments and schedules, no LDS, no barrier, no atomic.  The update arithmetic is Td<T>::apply with ONE scalar replaced:
// where Q-learning bootstraps from m = np.max(Q[s', valid]), these rules pass v.
//
// Expected SARSA -- the step order of k_rollout_runs (pick from the post-update row); v is the expectation of Q[s', .]
// under the epsilon-greedy policy that will act in s' (row_expected_lane), with the epsilon of the NEXT step.
//
// SARSA -- the next action is chosen BEFORE the update, from the row of s' as it stands then, with the draws and the
// epsilon of the next step, and the update bootstraps from its value:
//   step with counter k:
//     a       = the run's pending action if it has one, else the pick from row(s) with draws(id, k), eps_k
//     s', r, terminated = Env::step(s, a)
//     a'      = pick from row(s') with draws(id, k + 1), eps_{k+1}
//     Q[s, a] = Td::apply(Q[s, a], r, Q[s', a'], terminated, lr_k, gamma)
//     pending = a'
// Only (a, Q[s, a]) is carried from step to step; the row of s' is dead after the pick.  When s' == s and a' == a the
// carried prediction is the UPDATED cell.  After a terminated step s' is the reset observation: a' is the first action of
// the new episode.  The pending action is run state: loaded at launch start (-1: none), stored at launch end.
#pragma once
#include "qe_rollout_runs.h"

namespace qe {

enum TdRule : int { TD_Q_LEARNING = 0, TD_SARSA = 1, TD_EXPECTED_SARSA = 2 };  // qe_update_rule

// Expected SARSA's bootstrap value of a row: (1 - e) * max + e * mean over the valid columns, in float64, rounded once
// to the table dtype.  The sum runs left to right over the valid columns; e is eps clamped as eps_threshold clamps it.
// `row` is the row as loaded (invalid and padding columns are skipped by `valid`), `m` its np.max.
template <typename T, int NV, typename M>
__device__ __forceinline__ T row_expected_lane(const RowV<T, NV>& row, M valid, T m, double eps) {
#pragma clang fp contract(off)
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * NV; ++j) tot = ((valid >> j) & 1) ? tot + (double)row.v[j] : tot;
    const double mean = tot / (double)popc_mask(valid);
    const double e = !(eps > 0.0) ? 0.0 : (eps >= 1.0 ? 1.0 : eps);
    const double keep = (1.0 - e) * (double)m, spread = e * mean;
    return (T)(keep + spread);
}

template <typename T, class Env, int NV, bool MASKED, int RULE>
__global__ __launch_bounds__(RUNS_BLOCK) void k_rollout_runs_td(RunsCtx<T> c, EnvCtx ev, long long steps, int32_t* pending) {
    static_assert(RULE == TD_SARSA || RULE == TD_EXPECTED_SARSA, "Q-learning runs k_rollout_runs");
    using M = typename LaneMask<NV>::type;
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    T* const q = c.q + r * c.S * (4 * NV);
    RunLane<T, NV, MASKED> lane(c, ev, r);

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    bool row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
    if constexpr (RULE == TD_SARSA) {
        int act = pending[r];
        T picked;
        if (act < 0) act = lane.pick_on_policy(row, valid, row_nan, lane.step0, lane.eps_v, &picked);
        else picked = row_pick_lane(row, act);
        for (long long t = 0; t < steps; ++t) {
            const unsigned long long step = lane.step0 + (unsigned long long)t;
            const int32_t s = lane.n;
            const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
            lane.n = tr.next_obs;
            load_row_lane<NV>(row, q, lane.n);
            valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
            row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
            const double eps_n = lane.next_eps();
            T v;
            const int next = lane.pick_on_policy(row, valid, row_nan, step + 1ull, eps_n, &v);
            lane.learning_rate(lane.lr_v);
            T u;
            const T q1 = Td<T>::apply(picked, tr.reward, v, tr.terminated, lane.h, c.mode, &u);
            q[(int64_t)s * (4 * NV) + act] = q1;
            picked = (lane.n == s && next == act) ? q1 : v;  // the next prediction is the cell as this step leaves it
            act = next;
            lane.episode_end(tr, t);
            lane.advance_schedules(eps_n);
        }
        pending[r] = act;
    } else {
        for (long long t = 0; t < steps; ++t) {
            const unsigned long long step = lane.step0 + (unsigned long long)t;
            T picked;
            const int act = lane.pick_on_policy(row, valid, row_nan, step, lane.eps_v, &picked);
            const int32_t s = lane.n;
            const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
            lane.n = tr.next_obs;
            load_row_lane<NV>(row, q, lane.n);
            valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
            const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
            row_nan = row_nan_lane<NV>(rowm);
            const T m = row_nan ? quiet_nan<T>() : row_max_lane(rowm);
            const double eps_n = lane.next_eps();
            const T v = row_expected_lane<T, NV, M>(row, valid, m, eps_n);
            lane.learning_rate(lane.lr_v);
            T u;
            const T q1 = Td<T>::apply(picked, tr.reward, v, tr.terminated, lane.h, c.mode, &u);
            q[(int64_t)s * (4 * NV) + act] = q1;
            if (lane.n == s) {  // own write lands in the row held in registers
                row_nan |= q1 != q1;
                patch_own_write<NV>(row, act, q1);
            }
            lane.episode_end(tr, t);
            lane.advance_schedules(eps_n);
        }
    }
    lane.store();
}

}  // namespace qe
