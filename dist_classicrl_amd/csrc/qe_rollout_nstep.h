// qe_rollout_nstep.h -- population rollout with an n-step on-policy target: n-step SARSA and n-step Expected SARSA (gfx950).
//
// The sibling of k_rollout_runs_td (qe_rollout_runs_td.h): one run per lane, the same launch shape, per-run state, draws,
// log segments and schedules, no barrier, no atomic.  What is new is the WINDOW of a run: its last transitions
// (s_i, a_i, r_i), oldest first, at most n - 1 of them between steps.  One step with draw counter k:
//   1. a = the action of the 1-step rule (SARSA: the pending action, else the pick from row(s) with draws(id, k), eps_k;
//      Expected SARSA: the pick from the row as the previous step's stores left it);
//   2. s', r, terminated = Env::step(s, a); (s, a, r) is appended: the window now holds L <= n entries;
//   3. v = the bootstrap scalar of the 1-step rule, from the row of s' BEFORE any store of this step (SARSA: Q[s', a'],
//      a' picked with draws(id, k + 1), eps_{k+1} and kept as the pending action; Expected SARSA: row_expected_lane);
//   4. terminated: every entry j = 0 .. L-1 is updated, oldest first, and the window emptied; else, L == n: entry 0 is
//      updated and popped; else nothing.  The update of entry j is
//          Q[s_j, a_j] = Td<T>::apply(Q[s_j, a_j], r_j, g_{j+1}, term_j, lr_k, gamma, mode)
//      with the prediction read from the table at that moment (a cell that occurs twice sees its earlier update) and
//          g_L = v,  g_i = td_target(r_i, g_{i+1}, term_i)   for i = L-1 down to j+1
//      (td_target, qe_device.h: the target of Td<T>::apply rounded to the table dtype; term_i only for i = L-1 of a
//      terminated step);
//   5. the next pick reads the row of s' as it stands after these stores (Expected SARSA: stores into the held row are
//      patched into the registers).
// With n = 1 this is the step of k_rollout_runs_td; the host never launches this kernel for n = 1.
//
// The window lives in dynamic LDS: three planes [slot][lane] of n * 64 words (states, actions, rewards), 64 * n * 12
// bytes per workgroup.  A lane touches only its own column -- whatever slot each lane is at, the 64 addresses of an access
// fall into 64 different banks -- and reads only what it wrote itself: the workgroup is one wavefront, there is no
// barrier.  Each lane keeps the slot of its oldest entry (a ring) and the length in registers.  Registers could not
// hold the window: 3 * 16 words more would push the wide fp64 builds, which fill the register file, into scratch.  The
// size is dynamic because a static 12 KB would cap the NV = 1 builds at 13 waves per CU for n = 2 as well.
// The window is run state: loaded from the per-run arrays [slot][M] at launch start, stored there at launch end.
#pragma once
#include "qe_rollout_runs_td.h"

namespace qe {

constexpr int NSTEP_MAX = 16;

template <typename T, class Env, int NV, bool MASKED, int RULE>
__global__ __launch_bounds__(RUNS_BLOCK) void k_nstep_rollout(RunsCtx<T> c, EnvCtx ev, long long steps, int32_t* pending,
                                                             RunWindows w) {
    static_assert(RULE == TD_SARSA || RULE == TD_EXPECTED_SARSA, "an uncorrected n-step Q-learning is no off-policy method");
    using M = typename LaneMask<NV>::type;
    extern __shared__ int32_t nstep_lds[];
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    const int N = w.n;
    int32_t* const ws = nstep_lds + threadIdx.x;  // this lane's column of the three planes: slot k at [k * RUNS_BLOCK]
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

    RowV<T, NV> row;
    load_row_lane<NV>(row, q, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    bool row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
    int act = 0;
    if constexpr (RULE == TD_SARSA) {
        act = pending[r];
        T unused;
        if (act < 0) act = lane.pick_on_policy(row, valid, row_nan, lane.step0, lane.eps_v, &unused);
    }
    for (long long t = 0; t < steps; ++t) {
        const unsigned long long step = lane.step0 + (unsigned long long)t;
        // A window of n - 1 entries: this step updates entry 0 whatever happens (it pops, or the episode ends), and
        // nothing is stored before that update -- its prediction is loaded now, off the chain pick -> step -> gather
        const bool early = L == N - 1;
        T p0 = T(0);
        if (early) p0 = q[(int64_t)ws[at(0)] * (4 * NV) + wa[at(0)]];
        if constexpr (RULE == TD_EXPECTED_SARSA) {
            T unused;
            act = lane.pick_on_policy(row, valid, row_nan, step, lane.eps_v, &unused);
        }
        const int32_t s = lane.n;
        const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
        lane.n = tr.next_obs;
        {
            const int k = at(L);
            ws[k] = s; wa[k] = act; wr[k] = tr.reward;
            ++L;
        }
        load_row_lane<NV>(row, q, lane.n);
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
        const double eps_n = lane.next_eps();
        T v;
        if constexpr (RULE == TD_SARSA) {
            row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
            act = lane.pick_on_policy(row, valid, row_nan, step + 1ull, eps_n, &v);
        } else {
            const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
            row_nan = row_nan_lane<NV>(rowm);
            const T m = row_nan ? quiet_nan<T>() : row_max_lane(rowm);
            v = row_expected_lane<T, NV, M>(row, valid, m, eps_n);
        }
        lane.learning_rate(lane.lr_v);
        const int updates = tr.terminated ? L : (L == N ? 1 : 0);
        for (int j = 0; j < updates; ++j) {
            T g = v;
            for (int i = L - 1; i > j; --i) g = td_target(wr[at(i)], g, tr.terminated && i == L - 1, lane.h, c.mode);
            const int k = at(j);
            const int32_t sj = ws[k], aj = wa[k];
            T* const cell = q + (int64_t)sj * (4 * NV) + aj;
            const T pred = (j == 0 && early) ? p0 : *cell;
            T u;
            const T q1 = Td<T>::apply(pred, wr[k], g, tr.terminated && j == L - 1, lane.h, c.mode, &u);
            *cell = q1;
            if constexpr (RULE == TD_EXPECTED_SARSA) {
                if (sj == lane.n) {  // own write lands in the row held in registers
                    row_nan |= q1 != q1;
                    patch_own_write<NV>(row, aj, q1);
                }
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
        lane.advance_schedules(eps_n);
    }
    if constexpr (RULE == TD_SARSA) pending[r] = act;
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
