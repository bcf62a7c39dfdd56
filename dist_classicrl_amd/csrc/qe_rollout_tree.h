// qe_rollout_tree.h -- population rollout with n-step Tree Backup under a greedy target policy: the off-policy n-step
// Q-learning (Sutton & Barto 7.5; gfx950).
//
// The sibling of k_rollout_runs (qe_rollout_runs.h) and k_nstep_rollout (qe_rollout_nstep.h): one run per lane, the same
// launch shape, per-run state, draws, log segments and schedules, no barrier, no atomic, no cross-lane work.  Everything
// not named here is k_rollout_runs's: Q-learning's order, the pick reads the row as the previous step's stores left it.
// The run's WINDOW holds entries (s_i, a_i, r_i, f_i), oldest first, at most n - 1 of them between steps; f_i says
// whether a_i was greedy.  One step with draw counter k:
//   1. a = pick(row(s), draws(id, k), eps_k); f = (Q[s, a] == np.max(Q[s, valid])) on the row the pick saw -- the
//      expression of Watkins's cut in k_trace_rollout; a NaN maximum is never equal; no new draws;
//   2. s', r, terminated = Env::step(s, a); (s, a, r, f) is appended: the window now holds L <= n entries;
//   3. v = np.max(Q[s', valid]) from the row of s' BEFORE any store of this step (the one-step kernel's bootstrap);
//   4. terminated: every entry j = 0 .. L-1 is updated, oldest first, and the window emptied; else, L == n: entry 0 is
//      updated and popped; else nothing.  The update of entry j is
//          Q[s_j, a_j] = Td<T>::apply(Q[s_j, a_j], r_j, g_{j+1}, term_j, lr_k, gamma, mode)
//      with the prediction read from the table at that moment and g_i the value the greedy target policy sees at s_i:
//          g_L = v;   f_i:  g_i = td_target(r_i, g_{i+1}, term_i);   !f_i:  g_i = np.max(Q[s_i, valid(s_i)])
//      for j < i < L, the row maximum read from the table at the moment of this update (it sees the earlier updates of
//      the same flush); term_i only for i = L-1 of a terminated step.  Only the nearest non-greedy entry c after j
//      matters: the fold runs from c - 1 (from L - 1 if there is none) down to j + 1.  The flag of entry j itself is not
//      read.  With every flag true this is the fold of k_nstep_rollout with v = the maximum;
//   5. the next pick reads the row of s' as it stands after these stores: stores with s_j == s' are patched into the
//      registers, as n-step Expected SARSA does.
// With n = 1 this is the step of k_rollout_runs; the host never launches this kernel for n = 1.
//
// The window lives in dynamic LDS as k_nstep_rollout has it: three planes [slot][lane] of n * 64 words (states, actions,
// rewards), 64 * n * 12 bytes per workgroup, a ring per lane.  The flag rides in the action word's top bit (set: greedy).
// The row of a cut state s_c is never held beside the row of s': row_np_max_at reduces it to its np.max as it arrives.
// In a steady step (n - 1 entries at its top) entry 0 is updated whatever happens and nothing is stored before that
// update, so its prediction AND the row of its nearest cut among the old entries are gathered at the top of the step,
// off the chain pick -> step -> gather; a cut at the step's own entry needs no gather at all (its row is the held row,
// whose maximum the flag has just used).  The later entries of a flush read per entry.
// The window is run state: loaded from the per-run arrays [slot][M] at launch start, stored there at launch end.
#pragma once
#include "qe_rollout_runs.h"

namespace qe {

constexpr int TREE_MAX = 16;
constexpr int32_t TREE_GREEDY = (int32_t)0x80000000u;  // the flag in an action word (RunWindows::a)

// np.max over the valid columns of row `row` of the run's table, 16 bytes (fp64: 2 x 16) at a time: the maximum and the
// NaN flag are folded as the columns arrive, so the row never occupies registers of its own.  -inf if no column is valid.
template <int NV, bool MASKED, typename M>
__device__ __forceinline__ float row_np_max_at(const float* q, int64_t row, M valid) {
    const float4* p = reinterpret_cast<const float4*>(q + row * (4 * NV));
    float m = neg_inf<float>();
    bool nan = false;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const float4 f = p[k];
        const float x[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = (!MASKED || ((valid >> (4 * k + j)) & 1)) ? x[j] : neg_inf<float>();
            m = lane_fmax(m, y);
            nan |= y != y;
        }
    }
    return nan ? quiet_nan<float>() : m;
}
template <int NV, bool MASKED, typename M>
__device__ __forceinline__ double row_np_max_at(const double* q, int64_t row, M valid) {
    const double2* p = reinterpret_cast<const double2*>(q + row * (4 * NV));
    double m = neg_inf<double>();
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 2 * NV; ++k) {
        const double2 f = p[k];
        const double x[2] = {f.x, f.y};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double y = (!MASKED || ((valid >> (2 * k + j)) & 1)) ? x[j] : neg_inf<double>();
            m = lane_fmax(m, y);
            nan |= y != y;
        }
    }
    return nan ? quiet_nan<double>() : m;
}

template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_tree_rollout(RunsCtx<T> c, EnvCtx ev, long long steps, RunWindows w) {
    using M = typename LaneMask<NV>::type;
    extern __shared__ int32_t tree_lds[];
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    const int N = w.n;
    int32_t* const ws = tree_lds + threadIdx.x;  // this lane's column of the three planes: slot k at [k * RUNS_BLOCK]
    int32_t* const wa = ws + N * RUNS_BLOCK;
    float* const wr = reinterpret_cast<float*>(wa + N * RUNS_BLOCK);
    T* const q = c.q + r * c.S * (4 * NV);
    RunLane<T, NV, MASKED> lane(c, ev, r);

    // the window: entry i (0 = oldest) sits in slot at(i) of the ring that starts at slot `base`
    int base = 0, L = w.len[r];
    for (int i = 0; i < L; ++i) {
        ws[i * RUNS_BLOCK] = w.s[(int64_t)i * c.M + r];
        wa[i * RUNS_BLOCK] = w.a[(int64_t)i * c.M + r];
        wr[i * RUNS_BLOCK] = w.r[(int64_t)i * c.M + r];
    }
    auto at = [&](int i) -> int {
        const int k = base + i;
        return (k >= N ? k - N : k) * RUNS_BLOCK;
    };
    // np.max(Q[s_c, valid(s_c)]) as the table holds it now
    auto cut_value = [&](int32_t sc) -> T {
        return row_np_max_at<NV, MASKED>(q, (int64_t)sc, valid_mask_lane<Env, NV, MASKED>(ev, r, sc));
    };

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    bool row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
    for (long long t = 0; t < steps; ++t) {
        const unsigned long long step = lane.step0 + (unsigned long long)t;
        // A window of n - 1 entries: this step updates entry 0 whatever happens (it pops, or the episode ends), and
        // nothing is stored before that update -- its prediction and the row of its nearest cut among the entries in
        // hand are loaded now, off the chain pick -> step -> gather
        const bool early = L == N - 1;
        T p0 = T(0), g0 = T(0);
        int c0 = 0;  // the nearest non-greedy entry after entry 0 among the old ones; 0: none
        if (early) {
            p0 = q[(int64_t)ws[at(0)] * (4 * NV) + (wa[at(0)] & ~TREE_GREEDY)];
            for (int i = 1; i < L; ++i)
                if (wa[at(i)] >= 0) {
                    c0 = i;
                    break;
                }
            if (c0) g0 = cut_value(ws[at(c0)]);
        }
        T picked;
        const int act = lane.pick(row, valid, row_nan, step, lane.eps_v, &picked);
        // the flag: Watkins's cut (k_trace_rollout), on the row the pick saw
        const T top = row_nan ? quiet_nan<T>() : row_max_lane(masked_row<MASKED>(row, valid));
        const bool greedy = picked == top;
        const int32_t s = lane.n;
        const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
        lane.n = tr.next_obs;
        {
            const int k = at(L);
            ws[k] = s; wa[k] = act | (greedy ? TREE_GREEDY : 0); wr[k] = tr.reward;
            ++L;
        }
        load_row_lane<NV>(row, q, lane.n);
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
        const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
        row_nan = row_nan_lane<NV>(rowm);
        const T v = row_nan ? quiet_nan<T>() : row_max_lane(rowm);
        lane.learning_rate(lane.lr_v);
        const int updates = tr.terminated ? L : (L == N ? 1 : 0);
        for (int j = 0; j < updates; ++j) {
            // g_{c}: the row maximum at the nearest cut c after j, folded from c - 1; without a cut v, folded from L - 1
            T g = v;
            int from = L - 1;
            if (j == 0 && early) {
                if (c0) {
                    g = g0;
                    from = c0 - 1;
                } else if (!greedy) {  // the cut is this step's own entry: its row was the held row, nothing stored since
                    g = top;
                    from = L - 2;
                }
            } else {
                for (int i = j + 1; i < L; ++i)
                    if (wa[at(i)] >= 0) {
                        g = cut_value(ws[at(i)]);
                        from = i - 1;
                        break;
                    }
            }
            for (int i = from; i > j; --i) g = td_target(wr[at(i)], g, tr.terminated && i == L - 1, lane.h, c.mode);
            const int k = at(j);
            const int32_t sj = ws[k], aj = wa[k] & ~TREE_GREEDY;
            T* const cell = q + (int64_t)sj * (4 * NV) + aj;
            const T pred = (j == 0 && early) ? p0 : *cell;
            T u;
            const T q1 = Td<T>::apply(pred, wr[k], g, tr.terminated && j == L - 1, lane.h, c.mode, &u);
            *cell = q1;
            if (sj == lane.n) {  // own write lands in the row held in registers
                row_nan |= q1 != q1;
                patch_own_write<NV>(row, aj, q1);
            }
        }
        if (tr.terminated) {
            L = 0;
            base = 0;
        } else if (updates) {
            base = base + 1 == N ? 0 : base + 1;
            --L;
        }
        lane.episode_end(tr, t);
        lane.advance_schedules();
    }
    for (int i = 0; i < L; ++i) {
        const int k = at(i);
        w.s[(int64_t)i * c.M + r] = ws[k];
        w.a[(int64_t)i * c.M + r] = wa[k];
        w.r[(int64_t)i * c.M + r] = wr[k];
    }
    w.len[r] = L;
    lane.store();
}

}  // namespace qe
