// qe_mdp_solve.h -- dynamic programming over the outcome records of a TableEnv (qe_envs.h), wave64 for gfx950:
// value iteration (Q*, V* of the MDP) and iterative evaluation of every run's greedy policy of a population.
//
// The law is the one TableEnv::step samples from.  For a cell (s, a) with K records, a running maximum t = 0 of the
// thresholds: slot j < K - 1 weighs w_j = max(0, thr_j - t) and then t = max(t, thr_j); slot K - 1 weighs 2^32 - t -- the
// measure of "the first j < K - 1 with u < thr_j, else slot K - 1" for a uniform 32-bit u.  p_j = w_j * 2^-32, exact in
// float64.  The backup of a cell over a value vector V (mdp_backup, shared by both solvers):
//     acc = 0.0;  for j ascending with w_j > 0:  x = double(r_j) + (terminated_j ? 0.0 : gamma * V[next_j]);  acc = acc + p_j * x
// one product and one add each, never contracted (-ffp-contract=off, see Makefile); a terminated outcome bootstraps 0, as
// Td<T>::apply does, and the auto-reset successor plays no part.
//
// Shape of a sweep (k_mdp_value_sweep, k_mdp_policy_sweep): one thread per (row, action), row = a state, or a (run,
// state) pair; a workgroup of MDP_BLOCK threads holds MDP_BLOCK / A whole rows.  Every thread streams its K 16-byte records
// (uint4 loads, all issued before the first use) and gathers V[next]; the backups meet in LDS and the first threads of
// the workgroup, one per row, walk their row's columns in ascending order -- the maximum, or the sum over the tie set --
// so the result does not depend on thread order.  Each sweep reads only the previous sweep's values (Jacobi, ping-pong
// buffers).  The residual max |V_t - V_{t-1}| crosses workgroups as an integer atomicMax on the bit pattern of the
// non-negative double, which orders like the double: deterministic.
//
// No host synchronisation per sweep.  The host enqueues batches of sweeps; sweep i of a batch has a residual word of its
// own, zeroed before the batch, and starts by reading the word of sweep i - 1: if that is <= tol the sweep does nothing
// and leaves its own word 0, so every later sweep of the batch does nothing either.  The stop is thus exactly the first
// sweep with residual <= tol, and the values of that sweep stay in the buffer of its parity.  The population form keeps
// one word per (sweep, run) and a done flag per run for the batches behind the one a run froze in.
#pragma once
#include "qe_envs.h"

namespace qe {

constexpr int MDP_BLOCK = 256;      // threads of a sweep workgroup: MDP_BLOCK / A rows (A <= MDP_BLOCK)
constexpr int MDP_BATCH = 32;       // sweeps the host enqueues between two reads of the residual words
constexpr uint32_t MDP_STATUS_DEAD_END = 1u, MDP_STATUS_NAN = 2u;

// q(s, a; V) of the cell whose K records start at `rec`.  `v` is the value vector the records' next states index.
template <int K>
__device__ __forceinline__ double mdp_backup(const uint4* __restrict__ rec, const double* __restrict__ v, double gamma) {
    uint4 r[K];
#pragma unroll
    for (int j = 0; j < K; ++j) r[j] = rec[j];
    double nv[K];
#pragma unroll
    for (int j = 0; j < K; ++j) nv[j] = v[r[j].y];  // (every record's next state is in range: qe_env_create_table)
    uint32_t t = 0u;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const unsigned long long w =
            j < K - 1 ? (unsigned long long)(r[j].x > t ? r[j].x - t : 0u) : 0x100000000ull - (unsigned long long)t;
        t = r[j].x > t ? r[j].x : t;
        const double boot = gamma * nv[j];
        const double x = (double)__uint_as_float(r[j].z) + (r[j].w != 0u ? 0.0 : boot);
        const double px = ((double)w * 0x1p-32) * x;
        acc = w != 0ull ? acc + px : acc;
    }
    return acc;
}

// whether column a of state s is valid: the environment's mask (n_words packed words per state), or every column
__device__ __forceinline__ bool mdp_valid(const uint32_t* __restrict__ mask, int n_words, int64_t s, int a) {
    return !mask || ((mask[s * n_words + (a >> 5)] >> (a & 31)) & 1u) != 0u;
}

// maximum over the wavefront of the bit patterns of non-negative doubles, then one atomicMax per wavefront
__device__ __forceinline__ void mdp_residual_max(unsigned long long bits, unsigned long long* word) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(bits, d, 64);
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0ull) atomicMax(word, bits);
}

// One sweep of value iteration: V_t[s] = max over the valid a of q(s, a; V_{t-1}), 0.0 for a state without a valid column.
// res_prev: the residual word of the previous sweep of this batch (NULL: the batch's first sweep); res: this sweep's.
template <int K>
__global__ __launch_bounds__(MDP_BLOCK) void k_mdp_value_sweep(const uint4* __restrict__ rec, const uint32_t* __restrict__ mask,
                                                               int n_words, int64_t S, int A, int rows_per_block,
                                                               const double* __restrict__ v_prev, double* __restrict__ v_next,
                                                               double gamma, double tol, const unsigned long long* res_prev,
                                                               unsigned long long* res) {
    __shared__ double q[MDP_BLOCK];
    if (res_prev && __longlong_as_double((long long)*res_prev) <= tol) return;  // (the whole grid alike)
    const int tid = threadIdx.x;
    const int lr = tid / A, a = tid - lr * A;
    const int64_t s = (int64_t)blockIdx.x * rows_per_block + lr;
    if (lr < rows_per_block && s < S) q[tid] = mdp_backup<K>(rec + ((uint64_t)s * (uint64_t)A + (uint64_t)a) * K, v_prev, gamma);
    __syncthreads();
    const int64_t s1 = (int64_t)blockIdx.x * rows_per_block + tid;
    unsigned long long bits = 0ull;
    if (tid < rows_per_block && s1 < S) {
        double m = 0.0;
        bool any = false;
        for (int j = 0; j < A; ++j) {
            if (!mdp_valid(mask, n_words, s1, j)) continue;
            const double x = q[tid * A + j];
            m = (!any || x > m) ? x : m;
            any = true;
        }
        v_next[s1] = m;
        bits = (unsigned long long)__double_as_longlong(fabs(m - v_prev[s1]));
    }
    mdp_residual_max(bits, res);
}

// Q[s, a] = q(s, a; v) for every cell, masked cells included (the Q_t of the sweep that made V_t from v = V_{t-1}).
template <int K>
__global__ __launch_bounds__(MDP_BLOCK) void k_mdp_q_values(const uint4* __restrict__ rec, int64_t cells, const double* __restrict__ v,
                                                            double gamma, double* __restrict__ q_out) {
    const int64_t c = (int64_t)blockIdx.x * MDP_BLOCK + threadIdx.x;
    if (c < cells) q_out[c] = mdp_backup<K>(rec + (uint64_t)c * K, v, gamma);
}

// The greedy tie set of every (run, state): bit a of gmask[r * S + s] = column a is valid and row[a] equals the maximum
// of the valid columns, row = the run's table row in the table dtype, T(A[s, .] + B[s, .]) with the double estimator
// (table_b non-NULL), as k_double_evaluate forms it -- what select_lane ties over at epsilon 0.  status[r]: bit 0 if
// some state of the run has no valid column, bit 1 if a valid column of the run holds a NaN.
template <typename T>
__global__ __launch_bounds__(MDP_BLOCK) void k_mdp_tie_sets(const T* __restrict__ table_a, const T* __restrict__ table_b, int ld,
                                                            const uint32_t* __restrict__ mask, int n_words, int64_t rows,
                                                            int64_t S, int A, unsigned long long* __restrict__ gmask,
                                                            uint32_t* status) {
    const int64_t row = (int64_t)blockIdx.x * MDP_BLOCK + threadIdx.x;
    if (row >= rows) return;
    const int64_t r = row / S, s = row - r * S;
    const T* const pa = table_a + row * ld;
    const T* const pb = table_b ? table_b + row * ld : nullptr;
    T m = 0;
    bool any = false, nan = false;
    for (int j = 0; j < A; ++j) {
        if (!mdp_valid(mask, n_words, s, j)) continue;
        const T z = pb ? pa[j] + pb[j] : pa[j];
        nan |= z != z;
        m = (!any || z > m) ? z : m;
        any = true;
    }
    unsigned long long g = 0ull;
    for (int j = 0; j < A; ++j) {
        if (!mdp_valid(mask, n_words, s, j)) continue;
        const T z = pb ? pa[j] + pb[j] : pa[j];
        g |= (unsigned long long)(z == m ? 1u : 0u) << j;
    }
    gmask[row] = g;
    const uint32_t st = (any ? 0u : MDP_STATUS_DEAD_END) | (nan ? MDP_STATUS_NAN : 0u);
    if (st) atomicOr(&status[r], st);
}

// Before the first sweep: a run with a NaN in a valid cell is done at sweep 0 with a NaN residual.
__global__ __launch_bounds__(MDP_BLOCK) void k_mdp_policy_begin(const uint32_t* __restrict__ status, int64_t M, uint8_t* done,
                                                                int32_t* sweeps, double* residual) {
    const int64_t r = (int64_t)blockIdx.x * MDP_BLOCK + threadIdx.x;
    if (r >= M) return;
    const bool nan = (status[r] & MDP_STATUS_NAN) != 0u;
    done[r] = nan ? 1 : 0;
    sweeps[r] = 0;
    residual[r] = nan ? __longlong_as_double(0x7FF8000000000000ll) : 0.0;
}

// One sweep of greedy-policy evaluation of every run that is not frozen:
//     V_t[r, s] = (sum over the tie set, ascending, from 0.0, of q(s, a; V_{t-1}[r, .])) / double(|tie set|),  0.0 if empty.
// A run is skipped when done[r] (frozen in an earlier batch, or NaN) or when its word of the previous sweep of this batch
// is <= tol (it froze there, or was skipped there already); a skipped run's word stays 0.
template <int K>
__global__ __launch_bounds__(MDP_BLOCK) void k_mdp_policy_sweep(const uint4* __restrict__ rec,
                                                                const unsigned long long* __restrict__ gmask, int64_t rows,
                                                                int64_t S, int A, int rows_per_block,
                                                                const double* __restrict__ v_prev, double* __restrict__ v_next,
                                                                const double* __restrict__ gammas, double tol,
                                                                const uint8_t* __restrict__ done, const unsigned long long* res_prev,
                                                                unsigned long long* res) {
    __shared__ double q[MDP_BLOCK];
    const int tid = threadIdx.x;
    const int lr = tid / A, a = tid - lr * A;
    const int64_t row = (int64_t)blockIdx.x * rows_per_block + lr;
    if (lr < rows_per_block && row < rows) {
        const int64_t r = row / S, s = row - r * S;
        const bool skip = done[r] || (res_prev && __longlong_as_double((long long)res_prev[r]) <= tol);
        if (!skip && ((gmask[row] >> a) & 1ull))
            q[tid] = mdp_backup<K>(rec + ((uint64_t)s * (uint64_t)A + (uint64_t)a) * K, v_prev + r * S, gammas[r]);
    }
    __syncthreads();
    const int64_t row1 = (int64_t)blockIdx.x * rows_per_block + tid;
    if (tid < rows_per_block && row1 < rows) {
        const int64_t r = row1 / S;
        if (done[r] || (res_prev && __longlong_as_double((long long)res_prev[r]) <= tol)) return;
        const unsigned long long g = gmask[row1];
        double sum = 0.0;
        for (int j = 0; j < A; ++j)
            if ((g >> j) & 1ull) sum = sum + q[tid * A + j];
        const double v = g ? sum / (double)__popcll(g) : 0.0;
        v_next[row1] = v;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(v - v_prev[row1]));
        if (bits != 0ull) atomicMax(&res[r], bits);
    }
}

// After a batch of n sweeps (sweeps base + 1 .. base + n): every run that was not done takes the first sweep of the batch
// whose word is <= tol -- done, frozen at that sweep -- else sweep base + n with its word.  res is [n][M].
__global__ __launch_bounds__(MDP_BLOCK) void k_mdp_policy_batch_end(const unsigned long long* __restrict__ res, int n, int64_t M,
                                                                    double tol, int32_t base, uint8_t* done, int32_t* sweeps,
                                                                    double* residual) {
    const int64_t r = (int64_t)blockIdx.x * MDP_BLOCK + threadIdx.x;
    if (r >= M || done[r]) return;
    for (int i = 0; i < n; ++i) {
        const double x = __longlong_as_double((long long)res[(int64_t)i * M + r]);
        if (x <= tol || i == n - 1) {
            done[r] = x <= tol ? 1 : 0;
            sweeps[r] = base + i + 1;
            residual[r] = x;
            return;
        }
    }
}

// Every run's values from the buffer of the parity of its last sweep; NaN for a run with status bit 1.
__global__ __launch_bounds__(MDP_BLOCK) void k_mdp_policy_collect(const double* __restrict__ v0, const double* __restrict__ v1,
                                                                  const int32_t* __restrict__ sweeps,
                                                                  const uint32_t* __restrict__ status, int64_t rows, int64_t S,
                                                                  double* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * MDP_BLOCK + threadIdx.x;
    if (row >= rows) return;
    const int64_t r = row / S;
    const double v = (sweeps[r] & 1) ? v1[row] : v0[row];
    out[row] = (status[r] & MDP_STATUS_NAN) ? __longlong_as_double(0x7FF8000000000000ll) : v;
}

}  // namespace qe
