// qe_rollout_trace.h -- population rollout with eligibility traces: SARSA(lambda) and Watkins's Q(lambda) (gfx950).
//
// The sibling of k_rollout_runs_td (qe_rollout_runs_td.h) and k_nstep_rollout (qe_rollout_nstep.h): one run per lane, the
// same launch shape, per-run state, draws, log segments and schedules, no barrier, no atomic, no cross-lane work.  What
// is new is the run's K TRACE SLOTS (s_i, a_i, e_i), e_i of the table dtype T: a truncated sparse trace table.  A slot
// with e_i == 0 is free; live slots name distinct cells.  d = T(float64(gamma) * float64(lambda)) is the run's decay
// factor.  One step with draw counter k:
//   SARSA(lambda)
//   1. a = the pending action, else the pick from row(s) with draws(id, k), eps_k;
//   2. s', r, terminated = Env::step(s, a);
//   3. a' = pick(row(s'), draws(id, k + 1), eps_{k+1}) from the row of s' before any store of this step; v = Q[s', a'];
//   4. u = the increment of Td<T>::apply(Q[s, a], r, v, terminated, lr_k, gamma, mode) (iter: of type T; vec on a
//      float32 table: the float64 vec_inc, unrounded); the cell is not stored here;
//   5. mark: a live slot that holds (s, a) gets e = 1 (replacing) or e + 1 (accumulating); else (s, a, 1) goes into the
//      lowest free slot, else into the slot of the smallest e (lowest index among equals), whose cell is dropped;
//   6. sweep: every live slot Q[s_i, a_i] += u * e_i, one product and one add in T (float32 vec: in float64, rounded
//      once); free slots are not touched;
//   7. decay: terminated: every e_i = 0; else e_i = T(e_i * d), denormals kept; a trace that reaches 0 frees its slot;
//   8. the next pick and the next prediction Q[s', a'] read the table after the sweep.
//   Watkins's Q(lambda): Q-learning's order -- the pick comes from the row as the previous step's stores left it (sweep
//   stores with s_i == s' are patched into the held row); unless Q[s, a] == np.max(Q[s, valid]) (a NaN maximum is never
//   equal) every e_i = 0 before the mark; then 2 .. 7 with v = np.max(Q[s', valid]) before any store.
// With d = 0, or with K = 1 and replacing traces, the step is the one-step rule's, symbol for symbol.
//
// The slots live in dynamic LDS: three planes [slot][lane] (e, then s, then a), 64 * K * (8 + sizeof(T)) bytes per
// workgroup.  A lane touches only its own column -- 64 addresses, 64 banks -- and reads only what it wrote itself: the
// workgroup is one wavefront, there is no barrier.  Each lane keeps `hi`, one past its highest live slot, in a register:
// every slot from hi on is free, and the scans stop there, so a step costs what its live traces cost.  The find and the
// min-scan of the mark run over LDS only, ahead of Env::step.  The sweep is up to K independent read-modify-writes:
// their loads are issued in batches of TRACE_BATCH ahead of the adds, so a batch is one round trip, not one per cell;
// the marked cell is not loaded at all (its value is the prediction in hand).
// The slots are run state: loaded from the per-run arrays [slot][M] at launch start, stored there at launch end.
#pragma once
#include <type_traits>

#include "qe_rollout_runs_td.h"

namespace qe {

constexpr int TRACE_MAX = 32;
constexpr int TRACE_BATCH = 4;

enum TraceKind : int { TRACE_REPLACING = 0, TRACE_ACCUMULATING = 1 };  // qe_trace_kind

// The slots of all runs between launches (PopState, qe_host.h), their count and kind, and every run's lambda.
template <typename T>
struct TraceSlots {
    int32_t K;             // 1 .. TRACE_MAX
    int32_t kind;          // TraceKind
    int32_t* s;            // [K * M]: slot i of run r at [i * M + r]
    int32_t* a;
    T* e;                  // 0: the slot is free
    const double* lambda;  // [M]
};

inline size_t trace_lds_bytes(int K, size_t esize) { return (size_t)RUNS_BLOCK * (size_t)K * (8 + esize); }

template <typename T, class Env, int NV, bool MASKED, int RULE>
__global__ __launch_bounds__(RUNS_BLOCK) void k_trace_rollout(RunsCtx<T> c, EnvCtx ev, long long steps, int32_t* pending,
                                                             TraceSlots<T> w) {
#pragma clang fp contract(off)
    static_assert(RULE == TD_Q_LEARNING || RULE == TD_SARSA, "Expected SARSA's trace form needs policy weights: not built");
    using M = typename LaneMask<NV>::type;
    constexpr bool F32 = std::is_same<T, float>::value;
    extern __shared__ __align__(16) unsigned char trace_lds[];
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    const int K = w.K;
    // this lane's column of the three planes: slot i at [i * RUNS_BLOCK]
    T* const we = reinterpret_cast<T*>(trace_lds) + threadIdx.x;
    int32_t* const ws = reinterpret_cast<int32_t*>(reinterpret_cast<T*>(trace_lds) + K * RUNS_BLOCK) + threadIdx.x;
    int32_t* const wa = ws + K * RUNS_BLOCK;
    T* const q = c.q + r * c.S * (4 * NV);
    RunLane<T, NV, MASKED> lane(c, ev, r);
    const T decay = (T)(lane.h.gamma * w.lambda[r]);
    const bool accumulate = w.kind == TRACE_ACCUMULATING;
    const bool vec32 = F32 && c.mode == 1;

    int hi = 0;  // one past the highest live slot: slots hi .. K-1 hold e == 0
    for (int i = 0; i < K; ++i) {
        const T e = w.e[(int64_t)i * c.M + r];
        we[i * RUNS_BLOCK] = e;
        ws[i * RUNS_BLOCK] = w.s[(int64_t)i * c.M + r];
        wa[i * RUNS_BLOCK] = w.a[(int64_t)i * c.M + r];
        if (e != T(0)) hi = i + 1;
    }

    // RunLane::episode_end, kept here with the log index written out twice: with the shared form the double NV = 4 unmasked
    // SARSA build needs 130 VGPRs, not 126, and loses a wave
    auto episode_end = [&](const Transition& tr, long long t) {
        lane.acc += tr.reward;
        if (tr.terminated) {
            if (lane.logged < c.seg_len) {
                c.seg_step[r * c.seg_len + lane.logged] = (int32_t)(c.t_call + t);
                c.seg_ret[r * c.seg_len + lane.logged] = lane.acc;
                ++lane.logged;
            }
            lane.sum += lane.acc;
            ++lane.count;
            lane.acc = 0.0f;
        }
    };
    auto clear = [&]() {
        for (int i = 0; i < hi; ++i) we[i * RUNS_BLOCK] = T(0);
        hi = 0;
    };
    // step 5: the slot of (s, act), LDS only
    auto mark = [&](int32_t s, int act) -> int {
        int hit = -1, fre = -1, lo = 0;
        T lo_e = T(0);
        for (int i = 0; i < hi; ++i) {
            const T e = we[i * RUNS_BLOCK];
            const bool live = e != T(0);
            if (live && ws[i * RUNS_BLOCK] == s && wa[i * RUNS_BLOCK] == act) hit = i;
            if (!live && fre < 0) fre = i;
            if (i == 0 || e < lo_e) { lo = i; lo_e = e; }
        }
        int k = hit;
        T e1 = T(1);
        if (hit >= 0) {
            if (accumulate) e1 = we[hit * RUNS_BLOCK] + T(1);
        } else {
            k = fre >= 0 ? fre : (hi < K ? hi : lo);  // (hi < K: slot hi is free; else every slot is live: the smallest)
            ws[k * RUNS_BLOCK] = s;
            wa[k * RUNS_BLOCK] = act;
        }
        we[k * RUNS_BLOCK] = e1;
        if (k >= hi) hi = k + 1;
        return k;
    };
    // steps 6 and 7: slot mk is the marked one, whose cell holds `pred`; stored(s_i, a_i, new value) after every store
    auto sweep = [&](int mk, T pred, T u, double u64, bool term, auto stored) {
        int top = 0;
        for (int i0 = 0; i0 < hi; i0 += TRACE_BATCH) {
            T e[TRACE_BATCH], qv[TRACE_BATCH];
            int32_t ss[TRACE_BATCH], aa[TRACE_BATCH];
#pragma unroll
            for (int j = 0; j < TRACE_BATCH; ++j) {
                const bool in = i0 + j < hi;
                e[j] = in ? we[(i0 + j) * RUNS_BLOCK] : T(0);
                ss[j] = in ? ws[(i0 + j) * RUNS_BLOCK] : 0;
                aa[j] = in ? wa[(i0 + j) * RUNS_BLOCK] : 0;
            }
#pragma unroll
            for (int j = 0; j < TRACE_BATCH; ++j)
                qv[j] = (e[j] != T(0) && i0 + j != mk) ? q[(int64_t)ss[j] * (4 * NV) + aa[j]] : pred;
#pragma unroll
            for (int j = 0; j < TRACE_BATCH; ++j) {
                if (e[j] != T(0)) {
                    T qn;
                    if (vec32) {
                        const double inc = u64 * (double)e[j];
                        qn = (T)((double)qv[j] + inc);
                    } else {
                        const T inc = u * e[j];
                        qn = qv[j] + inc;
                    }
                    q[(int64_t)ss[j] * (4 * NV) + aa[j]] = qn;
                    stored(ss[j], aa[j], qn);
                    const T en = term ? T(0) : e[j] * decay;
                    we[(i0 + j) * RUNS_BLOCK] = en;
                    if (en != T(0)) top = i0 + j + 1;
                }
            }
        }
        hi = top;
    };
    // step 4: the increment of Td<T>::apply
    auto increment = [&](T pred, float reward, T v, bool term, T* u, double* u64) {
        if constexpr (F32) {
            if (c.mode == 0) (void)Td<float>::apply(pred, reward, v, term, lane.h, 0, u);
            else *u64 = Td<float>::vec_inc(pred, reward, v, term, lane.h);
        } else {
            (void)Td<double>::apply(pred, reward, v, term, lane.h, c.mode, u);
        }
    };

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
            const int mk = mark(s, act);
            const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
            lane.n = tr.next_obs;
            load_row_lane<NV>(row, q, lane.n);
            valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
            row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
            const double eps_n = lane.next_eps();
            T v;
            const int next = lane.pick_on_policy(row, valid, row_nan, step + 1ull, eps_n, &v);
            lane.learning_rate(lane.lr_v);
            T u = T(0);
            double u64 = 0.0;
            increment(picked, tr.reward, v, tr.terminated, &u, &u64);
            T carry = v;  // the next prediction is the cell as this step's sweep leaves it
            sweep(mk, picked, u, u64, tr.terminated, [&](int32_t si, int32_t ai, T qn) {
                if (si == lane.n && ai == next) carry = qn;
            });
            picked = carry;
            act = next;
            episode_end(tr, t);
            lane.advance_schedules(eps_n);
        }
        pending[r] = act;
    } else {
        for (long long t = 0; t < steps; ++t) {
            const unsigned long long step = lane.step0 + (unsigned long long)t;
            T picked;
            const int act = lane.pick_on_policy(row, valid, row_nan, step, lane.eps_v, &picked);
            {  // Watkins's cut: a non-greedy action ends every trace
                const T top = row_nan ? quiet_nan<T>() : row_max_lane(masked_row<MASKED>(row, valid));
                if (!(picked == top)) clear();
            }
            const int32_t s = lane.n;
            const int mk = mark(s, act);
            const Transition tr = Env::step(ev, r, s, lane.aux, act, step);
            lane.n = tr.next_obs;
            load_row_lane<NV>(row, q, lane.n);
            valid = valid_mask_lane<Env, NV, MASKED>(ev, r, lane.n);
            const RowV<T, NV> rowm = masked_row<MASKED>(row, valid);
            row_nan = row_nan_lane<NV>(rowm);
            const T m = row_nan ? quiet_nan<T>() : row_max_lane(rowm);
            lane.learning_rate(lane.lr_v);
            T u = T(0);
            double u64 = 0.0;
            increment(picked, tr.reward, m, tr.terminated, &u, &u64);
            bool patched = false;
            sweep(mk, picked, u, u64, tr.terminated, [&](int32_t si, int32_t ai, T qn) {
                if (si == lane.n) {  // own write lands in the row held in registers
                    patched = true;
                    patch_own_write<NV>(row, ai, qn);
                }
            });
            if (patched) row_nan = row_nan_lane<NV>(masked_row<MASKED>(row, valid));
            episode_end(tr, t);
            lane.advance_schedules();
        }
    }
    for (int i = 0; i < K; ++i) {  // (slots from hi on: e == 0, written so; their s and a are not read by anyone)
        w.e[(int64_t)i * c.M + r] = we[i * RUNS_BLOCK];
        w.s[(int64_t)i * c.M + r] = ws[i * RUNS_BLOCK];
        w.a[(int64_t)i * c.M + r] = wa[i * RUNS_BLOCK];
    }
    lane.store();
}

}  // namespace qe
