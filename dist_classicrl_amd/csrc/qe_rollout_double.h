// qe_rollout_double.h -- population rollout with the double estimator: Double Q-learning (van Hasselt 2010; Sutton &
// Barto 6.7), two tables per run (gfx950).
//
// The sibling of k_rollout_runs (qe_rollout_runs.h): one run per lane, the same launch shape, per-run state, draws, log
// segments and schedules, no LDS, no barrier, no atomic.  Run r owns rows r*S .. r*S+S-1 of TWO [M*S, ld] tables, A
// (RunsCtx::q, the engine's table) and B (the extra kernel argument).  One step with draw counter k, x the ONE policy
// Philox block of (id, k):
//   pick     a from the sum row z[j] = T(A[s,j] + B[s,j]) (one addition in T), with the dispatcher's rule for one
//            agent exactly as k_rollout_runs applies it to its row: x0, x1, x2, eps_k, the NaN rule decided on z
//   step     s', r, terminated = Env::step(s, a)
//   coin     x3 >> 31: 0 -> X = A, Y = B; 1 -> X = B, Y = A
//   target   a* = np.argmax(X[s'][valid]) (first index of the maximum, ascending; a NaN counts as the maximum and the
//            first NaN wins); v = Y[s', a*]; no valid column: v = -inf, the empty maximum of the Q-learning path
//   update   X[s,a] = Td::apply(X[s,a], r, v, terminated, lr_k, gamma); Y is not written
// and the next pick reads the rows of s' as they stand after the store (Q-learning's order).
//
// Registers.  Only z is carried from step to step.  The coin is known before the gather, so the rows of s' are read as
// X and Y, 16 bytes of each at a time, straight into z and ONE running arg-maximum (best X so far, Y at its index):
// neither row is ever whole in registers.  The two cells of the picked column, X[s,a] and Y[s,a], are loaded once the
// pick is known -- two scalar-sized loads issued before Env::step and the gather, so they are back before the update
// needs them; the lane's own earlier store to that cell is ordered before them as any store and load of one thread
// are.  When s' == s only z[a] is patched, to T(X[s,a]' + Y[s,a]).
#pragma once
#include "qe_rollout_runs.h"

namespace qe {

// 16 bytes of a row of each table: the elements, and how many of them
template <typename T>
struct DoubleChunk;
template <>
struct DoubleChunk<float> {
    static constexpr int N = 4;
    using V = float4;
};
template <>
struct DoubleChunk<double> {
    static constexpr int N = 2;
    using V = double2;
};
__device__ __forceinline__ void chunk_values(const float4& c, float* out) {
    out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
}
__device__ __forceinline__ void chunk_values(const double2& c, double* out) {
    out[0] = c.x; out[1] = c.y;
}

// z = T(x + y) of row `row` of two tables, 16 bytes of each at a time
template <typename T, int NV>
__device__ __forceinline__ void load_sum_row_lane(RowV<T, NV>& z, const T* x, const T* y, int64_t row) {
    using C = DoubleChunk<T>;
    const typename C::V* px = reinterpret_cast<const typename C::V*>(x + row * (4 * NV));
    const typename C::V* py = reinterpret_cast<const typename C::V*>(y + row * (4 * NV));
#pragma unroll
    for (int k = 0; k < 4 * NV / C::N; ++k) {
        T xv[C::N], yv[C::N];
        chunk_values(px[k], xv);
        chunk_values(py[k], yv);
#pragma unroll
        for (int i = 0; i < C::N; ++i) z.v[C::N * k + i] = xv[i] + yv[i];
    }
}

// ... and, on the way, Y at np.argmax(X[valid]): a column replaces the running maximum if it is the first valid one, or
// if the maximum is not a NaN and the column is larger or a NaN.  No valid column: -inf.
template <typename T, int NV, typename M>
__device__ __forceinline__ T load_sum_row_argmax_lane(RowV<T, NV>& z, const T* x, const T* y, int64_t row, M valid) {
    using C = DoubleChunk<T>;
    const typename C::V* px = reinterpret_cast<const typename C::V*>(x + row * (4 * NV));
    const typename C::V* py = reinterpret_cast<const typename C::V*>(y + row * (4 * NV));
    T best = neg_inf<T>(), v = neg_inf<T>();
    bool have = false;
#pragma unroll
    for (int k = 0; k < 4 * NV / C::N; ++k) {
        T xv[C::N], yv[C::N];
        chunk_values(px[k], xv);
        chunk_values(py[k], yv);
#pragma unroll
        for (int i = 0; i < C::N; ++i) {
            const int j = C::N * k + i;
            z.v[j] = xv[i] + yv[i];
            const bool ok = (valid >> j) & 1;
            const bool take = ok && (!have || (best == best && (xv[i] > best || xv[i] != xv[i])));
            best = take ? xv[i] : best;
            v = take ? yv[i] : v;
            have |= ok;
        }
    }
    return v;
}

template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_double_rollout(RunsCtx<T> c, EnvCtx ev, long long steps, T* table_b) {
    using M = typename LaneMask<NV>::type;
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    T* const qa = c.q + r * c.S * (4 * NV);
    T* const qb = table_b + r * c.S * (4 * NV);
    RunLane<T, NV, MASKED> lane(c, ev, r);

    RowV<T, NV> z;
    load_sum_row_lane<T, NV>(z, qa, qb, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    bool z_nan = row_nan_lane<NV>(masked_row<MASKED>(z, valid));
    for (long long t = 0; t < steps; ++t) {
        const unsigned long long step = lane.step0 + (unsigned long long)t;
        const U4 x = lane.draws(step);
        const bool explore = (unsigned long long)x.x < eps_threshold(lane.eps_v);
        T zpick;
        const int act = lane.select(masked_row<MASKED>(z, valid), valid, explore, x, z_nan, &zpick);
        const int32_t s = lane.n;
        const bool coin = (x.w >> 31) != 0;
        T* const qx = coin ? qb : qa;
        const T* const qy = coin ? qa : qb;
        const int64_t cell = (int64_t)s * (4 * NV) + act;
        const T picked = qx[cell], other = qy[cell];
        const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
        lane.n = tr.next_obs;
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
        const T v = load_sum_row_argmax_lane<T, NV, M>(z, qx, qy, lane.n, valid);
        z_nan = row_nan_lane<NV>(masked_row<MASKED>(z, valid));
        lane.learning_rate(lane.lr_v);
        T u;
        const T q1 = Td<T>::apply(picked, tr.reward, v, tr.terminated, lane.h, c.mode, &u);
        qx[cell] = q1;
        if (lane.n == s) {  // own write lands in the sum row held in registers
            // (a NaN z[a] stays one: a NaN in either cell, or inf + -inf, survives the update of X[s,a] -- so OR suffices)
            const T z1 = q1 + other;
            z_nan |= z1 != z1;
            patch_own_write<NV>(z, act, z1);
        }
        lane.episode_end(tr, t);
        lane.advance_schedules();
    }
    lane.store();
}

// Greedy evaluation of every run of a double population: k_evaluate_runs with the sum row z in place of the row -- the
// pick at epsilon 0 from z (the evaluation's selection rule), Env::step, the gather of both rows.  No store, no coin.
template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_double_evaluate(RunsCtx<T> c, EnvCtx ev, long long steps, long long episodes,
                                                                long long* used, uint8_t* done, const T* table_b) {
    using M = typename LaneMask<NV>::type;
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    if (episodes && done[r]) {  // finished in an earlier launch: an empty log segment, nothing else
        if (c.seg_len) c.seg_cnt[r] = 0;
        return;
    }
    const T* const qa = c.q + r * c.S * (4 * NV);
    const T* const qb = table_b + r * c.S * (4 * NV);
    RunLane<T, NV, MASKED, false> lane(c, ev, r);
    bool empty = false, finished = false;

    RowV<T, NV> z;
    load_sum_row_lane<T, NV>(z, qa, qb, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    long long t = 0;
    while (t < steps) {
        const unsigned long long step = lane.step0 + (unsigned long long)t;
        const U4 x = lane.draws(step);
        const RowV<T, NV> zm = masked_row<MASKED>(z, valid);
        T zpick;
        int act = select_lane<T, NV, M>(zm, valid, false, x.y, x.z, &zpick, lane.nan_sel && row_nan_lane<NV>(zm));
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
        load_sum_row_lane<T, NV>(z, qa, qb, lane.n);
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
