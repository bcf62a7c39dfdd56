// qe_rollout_dyna.h -- population rollout with Dyna-Q: a learned model and planning updates (gfx950).
//
// The sibling of k_rollout_runs (qe_rollout_runs.h): one run per lane, the same launch shape, per-run state, draws, log
// segments and schedules, no LDS, no barrier, no atomic, no cross-lane work.  What is new is the run's MODEL and its
// VISITED LIST, both in global memory, both the run's own:
//   model    one 8-byte entry per table cell, indexed like the table (o = s * ld + a, ld = 4 * NV the row stride):
//            word 0 = next_obs | terminated << 31, or DYNA_UNSEEN; word 1 = the bits of the float32 reward;
//   visited  the table offsets o of the seen cells in order of first observation, count entries.
// One training step with draw counter k:
//   1. the step of k_rollout_runs, steps 1-6, symbol for symbol: pick, Env::step, m = np.max(Q[s', valid]) before the
//      store, Q[s, a] = Td<T>::apply(...);
//   2. learn: an unseen cell (s, a) is appended to the list; model[s, a] = (s', r, terminated);
//   3. plan, i = 0 .. n-1 in order: x_i = word i & 3 of philox(id, k, STREAM_PLAN | (i >> 2) << 8); j = mulhi32(x_i,
//      count); c_i = visited[j]; (p, rho, tau) = model[c_i]; m_i = np.max(Q[p, valid(p)]) as the table stands now;
//      Q[c_i] = Td<T>::apply(Q[c_i], rho, m_i, tau, lr_k, gamma, mode);
//   4. the next pick sees the table after these stores; the schedules advance once per step.
//
// Memory traffic.  The model entry of (s, a) -- "seen before?" -- is loaded right after the pick, beside Env::step and
// the gather of the next row.  count and every x_i are known when planning starts and neither the list nor the model
// changes while it runs, so the list loads of a group of DYNA_BATCH updates go out together, then their model loads:
// two round trips per group, not two per update.  Only the table read-modify-writes stay in order: update i loads the
// row of p_i and the cell c_i (independent of each other: one round trip) behind the store of update i - 1.
//
// Ordering.  A lane reads only what it wrote itself or what was there at launch.  Its loads follow its own earlier
// stores to the same address: a wavefront's vector memory instructions are issued in program order into one queue of
// the CU's vector cache, which serves same-address requests of one wavefront in that order (the write-through cache
// line a store hits is updated in place) -- the single-thread coherence every kernel of this file's family relies on
// when it gathers a row it stored to in an earlier step.
//
// The row of the current state stays in registers across the planning updates: a planning store that lands in that
// row (o / ld == s') is PATCHED into the registers, as the real step's own write is; NaN-ness of the row is recomputed
// after a group that patched.  Reloading instead would put a dependent round trip on every step's selection chain.
#pragma once
#include "qe_rollout_runs.h"

namespace qe {

constexpr int DYNA_MAX = 64;     // planning updates per step
constexpr int DYNA_BATCH = 4;    // list / model loads in flight per group: one Philox block
constexpr uint32_t DYNA_UNSEEN = 0xFFFFFFFFu;

// Model and list of all runs between launches (PopState, qe_host.h).
struct DynaModel {
    int32_t n;         // planning updates per step, 1 .. DYNA_MAX
    uint2* entry;      // [M][S * ld]
    int32_t* visited;  // [M][S * A]
    int32_t* count;    // [M]
    int64_t cells;     // S * A: the stride of `visited`
};

template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_dyna_rollout(RunsCtx<T> c, EnvCtx ev, long long steps, DynaModel w) {
    using M = typename LaneMask<NV>::type;
    constexpr int LD = 4 * NV;
    constexpr int LOG_LD = NV == 1 ? 2 : (NV == 2 ? 3 : (NV == 4 ? 4 : (NV == 8 ? 5 : 6)));
    static_assert((1 << LOG_LD) == LD, "the row stride is a power of two");
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    T* const q = c.q + r * c.S * LD;
    uint2* const model = w.entry + r * c.S * LD;
    int32_t* const visited = w.visited + r * w.cells;
    int32_t seen = w.count[r];
    const int plan = w.n;
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
        const int32_t cell = s * LD + act;
        const uint32_t known = model[cell].x;  // (in flight beside the environment step and the gather)
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
        q[cell] = q1;
        if (lane.n == s) {  // own write lands in the row held in registers
            row_nan |= q1 != q1;
            patch_own_write<NV>(row, act, q1);
        }
        // 2. the model learns the outcome; a later outcome of the cell overwrites this one
        if (known == DYNA_UNSEEN) visited[seen++] = cell;
        model[cell] = make_uint2((uint32_t)lane.n | (tr.terminated ? 0x80000000u : 0u), __float_as_uint(tr.reward));
        // 3. planning
        for (int i0 = 0; i0 < plan; i0 += DYNA_BATCH) {
            const U4 y = lane.draws(step, STREAM_PLAN | ((uint32_t)(i0 >> 2) << 8));
            const uint32_t xs[DYNA_BATCH] = {y.x, y.y, y.z, y.w};
            int32_t o[DYNA_BATCH];
            uint2 e[DYNA_BATCH];
#pragma unroll
            for (int j = 0; j < DYNA_BATCH; ++j) o[j] = visited[mulhi32(xs[j], (uint32_t)seen)];  // (seen >= 1: index < seen)
#pragma unroll
            for (int j = 0; j < DYNA_BATCH; ++j) e[j] = model[o[j]];
            bool patched = false;
#pragma unroll
            for (int j = 0; j < DYNA_BATCH; ++j) {
                if (i0 + j < plan) {
                    const int32_t p = (int32_t)(e[j].x & 0x7FFFFFFFu);
                    const bool term = (e[j].x >> 31) != 0;
                    const float rho = __uint_as_float(e[j].y);
                    RowV<T, NV> rp;
                    load_row_lane<NV>(rp, q, p);
                    const T q0 = q[o[j]];
                    const RowV<T, NV> rpm = masked_row<MASKED>(rp, valid_mask_lane<Env, NV, MASKED>(ev, r, p));
                    const T mp = row_nan_lane<NV>(rpm) ? quiet_nan<T>() : row_max_lane(rpm);
                    T up;
                    const T qn = Td<T>::apply(q0, rho, mp, term, lane.h, c.mode, &up);
                    q[o[j]] = qn;
                    if ((o[j] >> LOG_LD) == lane.n) {  // the store lands in the row held in registers
                        patched = true;
                        const int col = o[j] & (LD - 1);
                        patch_own_write<NV>(row, col, qn);
                    }
                }
            }
            if (patched) row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
        }
        lane.episode_end(tr, t);
        lane.advance_schedules();
    }
    w.count[r] = seen;
    lane.store();
}

}  // namespace qe
