// qe_rollout_dyna_sample.h -- population rollout with Dyna-Q over a SAMPLE MODEL: up to K remembered outcomes per cell
// with their counts, and planning updates that draw one of them in proportion to its count (gfx950).
//
// The sibling of k_dyna_rollout (qe_rollout_dyna.h) for stochastic environments: one run per lane, the same launch
// shape, per-run state, draws, log segments, schedules and visited list, no LDS, no barrier, no atomic, no cross-lane
// work.  The last-outcome model of that kernel is replaced by K slots per table cell, K = 2 .. DYNA_OUTCOMES_MAX, a
// run-time value; both arrays are indexed like the table (o = s * ld + a) times K, so a cell's slots are contiguous:
//   cnt   one uint32 per slot: how often the slot's outcome was observed, 0 = free.  Occupied slots form a prefix in
//         order of first observation; a cell is seen when and only when cnt[o * K] != 0;
//   key   one 8-byte entry per slot: word 0 = next_obs | terminated << 31, word 1 = the bits of the float32 reward.
// One training step with draw counter k ("sample model"):
//   1. the step of k_rollout_runs, as in k_dyna_rollout;
//   2. learn (s', r, terminated) of (s, a): an unseen cell is appended to the list.  A slot MATCHES when its reward has
//      the same 32 bits, its flag is the same, and the flag is set or its next_obs is s'.  Match: the slot's next_obs
//      becomes s' and its count goes up by one unless the cell's total N is 2^32 - 1.  No match: the first free slot,
//      else -- none free, or N is 2^32 - 1 and a new slot would push it past that -- the occupied slot with the smallest
//      count (lowest index among equals), becomes (s', r, terminated, 1);
//   3. plan, i = 0 .. n-1 in order: c_i as in k_dyna_rollout; y_i = word i & 3 of philox(id, k, STREAM_OUTCOME |
//      (i >> 2) << 8); t = mulhi32(y_i, N(c_i)); the slot is the first j with t < n_0 + .. + n_j; (p, rho, tau) come
//      from it; the update is k_dyna_rollout's;
//   4. as there.
//
// Memory traffic.  The K counts and K keys of (s, a) are loaded right after the pick, beside Env::step and the gather
// of the next row, where k_dyna_rollout loads its one entry; the learn step then stores one key and one count.  In
// planning, the list loads of a group of DYNA_BATCH updates go out together, then the K counts of each of the four
// cells (4 * 8 registers at most), then -- the slots chosen -- the four keys: three round trips per group, one more
// than k_dyna_rollout, and not one more per update.  The slot loops are unrolled to DYNA_OUTCOMES_MAX and predicated
// on j < K: no register is indexed dynamically, so nothing lives in scratch.  A free slot's count is 0 and adds nothing
// to a running sum, so the slot walk needs no predicate of its own: t < N, and the sum reaches N at the last occupied
// slot.
//
// Ordering and the held row: as qe_rollout_dyna.h argues.  A lane's loads of cnt / key follow its own earlier stores
// to the same addresses in program order; the planning loop stores to neither.
#pragma once
#include "qe_rollout_dyna.h"

namespace qe {

constexpr int DYNA_OUTCOMES_MAX = 8;  // slots per cell

// Sample model and list of all runs between launches (PopState, qe_host.h).
struct SampleModel {
    int32_t n;         // planning updates per step, 1 .. DYNA_MAX
    int32_t K;         // slots per cell, 2 .. DYNA_OUTCOMES_MAX
    uint32_t* cnt;     // [M][S * ld][K]
    uint2* key;        // [M][S * ld][K]
    int32_t* visited;  // [M][S * A]
    int32_t* count;    // [M]
    int64_t cells;     // S * A: the stride of `visited`
};

template <typename T, class Env, int NV, bool MASKED>
__global__ __launch_bounds__(RUNS_BLOCK) void k_dyna_sample_rollout(RunsCtx<T> c, EnvCtx ev, long long steps, SampleModel w) {
    using M = typename LaneMask<NV>::type;
    constexpr int LD = 4 * NV;
    constexpr int LOG_LD = NV == 1 ? 2 : (NV == 2 ? 3 : (NV == 4 ? 4 : (NV == 8 ? 5 : 6)));
    constexpr int KM = DYNA_OUTCOMES_MAX;
    static_assert((1 << LOG_LD) == LD, "the row stride is a power of two");
    const int64_t r = (int64_t)blockIdx.x * RUNS_BLOCK + threadIdx.x;
    if (r >= c.M) return;
    const int K = w.K;
    T* const q = c.q + r * c.S * LD;
    uint32_t* const cnt = w.cnt + r * c.S * LD * K;
    uint2* const key = w.key + r * c.S * LD * K;
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
        const int64_t slot0 = (int64_t)cell * K;
        uint32_t kn[KM];  // (in flight beside the environment step and the gather)
        uint2 kk[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j) kn[j] = j < K ? cnt[slot0 + j] : 0u;
#pragma unroll
        for (int j = 0; j < KM; ++j) kk[j] = j < K ? key[slot0 + j] : make_uint2(0u, 0u);
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
        // 2. the model learns the outcome: match, else the first free slot, else the rarest outcome goes
        {
            const uint32_t w0 = (uint32_t)lane.n | (tr.terminated ? 0x80000000u : 0u), w1 = __float_as_uint(tr.reward);
            if (kn[0] == 0u) visited[seen++] = cell;
            uint32_t total = 0u, least = 0xFFFFFFFFu;
            int at = -1, spare = -1, rare = 0;
            uint32_t held = 0u;
#pragma unroll
            for (int j = KM - 1; j >= 0; --j) {  // (downwards: the lowest index wins every tie)
                if (j < K) {
                    total += kn[j];
                    const bool same = kn[j] != 0u && kk[j].y == w1 && ((kk[j].x ^ w0) >> 31) == 0u && (tr.terminated || kk[j].x == w0);
                    if (same) {
                        at = j;
                        held = kn[j];
                    }
                    if (kn[j] == 0u) spare = j;
                    if (kn[j] != 0u && kn[j] <= least) {
                        least = kn[j];
                        rare = j;
                    }
                }
            }
            const int put = at >= 0 ? at : (spare >= 0 && total != 0xFFFFFFFFu ? spare : rare);  // (N never passes 2^32 - 1)
            const uint32_t now = at >= 0 ? held + (total != 0xFFFFFFFFu ? 1u : 0u) : 1u;
            key[slot0 + put] = make_uint2(w0, w1);
            cnt[slot0 + put] = now;
        }
        // 3. planning
        for (int i0 = 0; i0 < plan; i0 += DYNA_BATCH) {
            const U4 y = lane.draws(step, STREAM_PLAN | ((uint32_t)(i0 >> 2) << 8));
            const U4 z = lane.draws(step, STREAM_OUTCOME | ((uint32_t)(i0 >> 2) << 8));
            const uint32_t xs[DYNA_BATCH] = {y.x, y.y, y.z, y.w};
            const uint32_t ys[DYNA_BATCH] = {z.x, z.y, z.z, z.w};
            int32_t o[DYNA_BATCH];
            uint32_t pn[DYNA_BATCH][KM];
            uint2 e[DYNA_BATCH];
#pragma unroll
            for (int j = 0; j < DYNA_BATCH; ++j) o[j] = visited[mulhi32(xs[j], (uint32_t)seen)];  // (seen >= 1: index < seen)
#pragma unroll
            for (int j = 0; j < DYNA_BATCH; ++j)
#pragma unroll
                for (int k = 0; k < KM; ++k) pn[j][k] = k < K ? cnt[(int64_t)o[j] * K + k] : 0u;
#pragma unroll
            for (int j = 0; j < DYNA_BATCH; ++j) {
                uint32_t total = 0u;
#pragma unroll
                for (int k = 0; k < KM; ++k) total += pn[j][k];
                const uint32_t pick = mulhi32(ys[j], total);  // < total (a listed cell has total >= 1)
                uint32_t sum = 0u;
                int slot = 0;
#pragma unroll
                for (int k = 0; k < KM - 1; ++k) {  // (past the last occupied slot the sum stays at total > pick)
                    sum += pn[j][k];
                    slot += sum <= pick ? 1 : 0;
                }
                e[j] = key[(int64_t)o[j] * K + min(slot, K - 1)];  // (the clamp binds only on a model no upload accepts)
            }
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
