// qe_rollout_visit.h -- population rollout with visit counts: an optimism bonus on the pick and a 1/N learning rate (gfx950).
//
// The sibling of k_rollout_runs (qe_rollout_runs.h): one run per lane, the same launch shape, per-run state, draws, log
// segments and schedules, no LDS, no barrier, no atomic, no cross-lane work.  What is new are two PLANES per run, both
// in global memory, both the run's own, both indexed like the table (o = s * ld + a, ld = 4 * NV the row stride):
//   N   uint32, how often the run has taken action a in state s (saturating at 2^32 - 1);
//   B   table dtype, the derived plane bonus(beta_r, N): T(0) when beta_r == 0, else T(beta_r / sqrt(float64(N))) -- a
//       float64 square root and a float64 division, both correctly rounded, and ONE rounding to T; N == 0 gives +inf.
//       The padding columns of B hold 0: the table's hold -inf, so the score there is -inf and never a NaN.
// One training step with draw counter k is the step of k_rollout_runs with three changes:
//   1. pick: the same Philox block, explore test and words, but select_lane sees the SCORE row, score_j = Q[s, j] +
//      B[s, j] (one add in T; invalid columns -inf through masked_row), with its NaN rule applied to that row; the
//      prediction handed to the update is Q[s, a], not the score;
//   2. count: N[s, a] <- N[s, a] + 1 (saturating) after Env::step, before the update; B[s, a] follows it;
//   3. rate: with visit_lr the update takes alpha = lr_k / float64(N[s, a]), the incremented count, a float64 division.
// The target m = np.max(Q[s', valid]) is taken on plain Q: the bonus changes the behaviour policy only.
//
// Memory traffic.  The B row of s' is gathered together with the Q row of s' (independent loads: one round trip).  The
// single cell N[s, a] is loaded right after the pick, in flight beside Env::step and the gather.  A step stores Q[s, a],
// N[s, a] and B[s, a], and computes ONE square root and division instead of the 4 * NV a recomputed row would take.
// When s' == s the held Q row and the held B row are both patched in registers, by the same select chain.
//
// Ordering.  A lane reads only what it wrote itself or what was there at launch (the single-work-item argument of
// qe_rollout_runs.h and qe_rollout_dyna.h): its loads follow its own earlier stores to the same address.
#pragma once
#include "qe_rollout_runs.h"

namespace qe {

constexpr uint32_t VISIT_MAX = 0xFFFFFFFFu;  // the counts saturate here

// The planes of all runs between launches (PopState, qe_host.h).
struct VisitPlanes {
    uint32_t* n;         // [M * S, ld]
    void* b;             // [M * S, ld] of the table dtype
    const double* beta;  // [M]
    int32_t visit_lr;    // alpha = lr / N[s, a]
};

// bonus(beta, N) in the table dtype (the definition above); the fill kernel and the rollout share it.
template <typename T>
__device__ __forceinline__ T visit_bonus(double beta, uint32_t n) {
    if (beta == 0.0) return (T)0;
    return (T)(beta / sqrt((double)n));
}

// B <- bonus(beta, N) over the real columns of every row, 0 in the padding (qe_population_set_visits /
// qe_population_set_visit_counts): one thread per cell.
template <typename T>
__global__ __launch_bounds__(256) void k_visit_fill(const uint32_t* n, T* b, const double* beta, int64_t cells_per_run, int64_t total,
                                                    int A, int ld) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int col = (int)(o % ld);
    b[o] = col < A ? visit_bonus<T>(beta[o / cells_per_run], n[o]) : (T)0;
}

// score row of the pick: Q + B, one add per column
template <typename T, int NV>
__device__ __forceinline__ RowV<T, NV> visit_score(const RowV<T, NV>& row, const RowV<T, NV>& bonus) {
    RowV<T, NV> s;
#pragma unroll
    for (int j = 0; j < 4 * NV; ++j) s.v[j] = row.v[j] + bonus.v[j];
    return s;
}

template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_visit_rollout(RunsCtx<T> c, EnvCtx ev, long long steps, VisitPlanes w) {
    using M = typename LaneMask<NV>::type;
    constexpr int LD = 4 * NV;
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    T* const q = c.q + r * c.S * LD;
    uint32_t* const cnt = w.n + r * c.S * LD;
    T* const bon = (T*)w.b + r * c.S * LD;
    const double beta = w.beta[r];
    const bool visit_lr = w.visit_lr != 0;
    RunLane<T, NV, MASKED> lane(c, ev, r);

    RowV<T, NV> row, brow;
    load_row_lane<NV>(row, q, lane.n);
    load_row_lane<NV>(brow, bon, lane.n);
    M valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
    for (long long t = 0; t < steps; ++t) {
        const unsigned long long step = lane.step0 + (unsigned long long)t;
        const U4 x = lane.draws(step);
        const bool explore = (unsigned long long)x.x < eps_threshold(lane.eps_v);
        // 1. the pick sees the score row; the update's prediction is the table's own value
        const RowV<T, NV> score = masked_row<MASKED>(visit_score<T, NV>(row, brow), valid);
        T scored;
        const int act = lane.select(score, valid, explore, x, row_nan_lane<NV>(score), &scored);
        const T picked = row_pick_lane(masked_row<MASKED>(row, valid), act);
        const int32_t s = lane.n;
        const int64_t cell = (int64_t)s * LD + act;
        const uint32_t seen = cnt[cell];  // (in flight beside the environment step and the gather)
        const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
        lane.n = tr.next_obs;
        load_row_lane<NV>(row, q, lane.n);
        load_row_lane<NV>(brow, bon, lane.n);
        valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
        const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
        const T m = row_nan_lane<NV>(rowm) ? quiet_nan<T>() : row_max_lane(rowm);
        // 2. the count, and the one cell of the bonus plane that follows it
        const uint32_t visits = seen == VISIT_MAX ? VISIT_MAX : seen + 1u;
        const T b1 = visit_bonus<T>(beta, visits);
        cnt[cell] = visits;
        bon[cell] = b1;
        // 3. the rate
        const double alpha = visit_lr ? lane.lr_v / (double)visits : lane.lr_v;
        lane.learning_rate(alpha);
        T u;
        const T q1 = Td<T>::apply(picked, tr.reward, m, tr.terminated, lane.h, c.mode, &u);
        q[cell] = q1;
        if (lane.n == s) {  // own writes land in the rows held in registers
#pragma unroll
            for (int j = 0; j < LD; ++j) {
                row.v[j] = j == act ? q1 : row.v[j];
                brow.v[j] = j == act ? b1 : brow.v[j];
            }
        }
        lane.episode_end(tr, t);
        lane.advance_schedules();
    }
    lane.store();
}

}  // namespace qe
