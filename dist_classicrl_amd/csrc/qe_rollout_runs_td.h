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
    const uint32_t id = ev.agent_offset + (uint32_t)r;
    const unsigned long long step0 = c.step0 + (c.step_off ? c.step_off[r] : 0ull);

    // the epsilon-greedy pick of the dispatcher's rule for one agent, with the draws of `step`; no selectable action:
    // reported after the call, action 0 keeps the run inside its table
    auto pick = [&](const RowV<T, NV>& row, M valid, bool row_nan, unsigned long long step, double eps, T* value) -> int {
        const U4 x = philox4x32_10(id, (uint32_t)step, (uint32_t)(step >> 32), STREAM_POLICY, c.seed_lo, c.seed_hi);
        const bool explore = (unsigned long long)x.x < eps_threshold(eps);
        int act = select_lane<T, NV, M>(masked_row<MASKED>(row, valid), valid, explore, x.y, x.z, value, nan_sel && row_nan);
        if (act < 0) {
            empty = true;
            act = 0;
            *value = row.v[0];
        }
        return act;
    };
    auto episode_end = [&](const Transition& tr, long long t) {
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
    };

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, n);
    bool row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
    if constexpr (RULE == TD_SARSA) {
        int act = pending[r];
        T picked;
        if (act < 0) act = pick(row, valid, row_nan, step0, eps_v, &picked);
        else picked = row_pick_lane(row, act);
        for (long long t = 0; t < steps; ++t) {
            const unsigned long long step = step0 + (unsigned long long)t;
            const int32_t s = n;
            const Transition tr = Env::step(ev, r, s, aux, act, step);
            n = tr.next_obs;
            load_row_lane<NV>(row, q, n);
            valid = valid_mask_lane<Env, NV, MASKED>(ev, r, n);
            row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
            const double eps_n = run_sched_next(eps_v, es.min_value, es.factor, es.kind);
            T v;
            const int next = pick(row, valid, row_nan, step + 1ull, eps_n, &v);
            h.lr = lr_v; h.lr32 = (float)lr_v;
            T u;
            const T q1 = Td<T>::apply(picked, tr.reward, v, tr.terminated, h, c.mode, &u);
            q[(int64_t)s * (4 * NV) + act] = q1;
            picked = (n == s && next == act) ? q1 : v;  // the next prediction is the cell as this step leaves it
            act = next;
            episode_end(tr, t);
            eps_v = eps_n;
            lr_v = run_sched_next(lr_v, ls.min_value, ls.factor, ls.kind);
        }
        pending[r] = act;
    } else {
        for (long long t = 0; t < steps; ++t) {
            const unsigned long long step = step0 + (unsigned long long)t;
            T picked;
            const int act = pick(row, valid, row_nan, step, eps_v, &picked);
            const int32_t s = n;
            const Transition tr = Env::step(ev, r, s, aux, act, step);
            n = tr.next_obs;
            load_row_lane<NV>(row, q, n);
            valid = valid_mask_lane<Env, NV, MASKED>(ev, r, n);
            const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
            row_nan = row_nan_lane<NV>(rowm);
            const T m = row_nan ? quiet_nan<T>() : row_max_lane(rowm);
            const double eps_n = run_sched_next(eps_v, es.min_value, es.factor, es.kind);
            const T v = row_expected_lane<T, NV, M>(row, valid, m, eps_n);
            h.lr = lr_v; h.lr32 = (float)lr_v;
            T u;
            const T q1 = Td<T>::apply(picked, tr.reward, v, tr.terminated, h, c.mode, &u);
            q[(int64_t)s * (4 * NV) + act] = q1;
            if (n == s) {  // own write lands in the row held in registers
                row_nan |= q1 != q1;
#pragma unroll
                for (int j = 0; j < 4 * NV; ++j) row.v[j] = j == act ? q1 : row.v[j];
            }
            episode_end(tr, t);
            eps_v = eps_n;
            lr_v = run_sched_next(lr_v, ls.min_value, ls.factor, ls.kind);
        }
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

}  // namespace qe
