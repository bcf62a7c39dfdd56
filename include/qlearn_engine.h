/*
 * qlearn_engine.h -- C ABI of the MI355X (gfx950) tabular Q-learning engine.
 *
 * This is the drop-in boundary for the ONE hot path of dist_classicrl: batched env.step() ->
 * epsilon-greedy (masked) arg-max -> TD target -> update of Q[s,a], with the Q-table resident in
 * HBM.  The reference has no FFI layer (it is pure Python/NumPy); each entry point below names the
 * reference interface it stands in for, paths relative to /root/reference/src/dist_classicrl/.
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every pointer is a HOST pointer unless the name ends in _dev.
 *   - every call returns 0 on success or a negative qe_status; qe_last_error() gives the text
 *     (thread-local).  The handle is NOT thread-safe (one host thread per engine, as the
 *     reference's single_thread runtime).
 *   - `states`/`actions` are int32 like the reference's NDArray[np.int32]; rewards float32;
 *     `terminated` and action masks are one byte per element (non-zero = true / valid).
 *   - table layout in HBM: row-major (state, action), row stride `ld` = action_size rounded up to a
 *     multiple of 4 elements (so every row starts 16-byte aligned for float4 loads).
 *   - randomness is counter based: Philox4x32-10, key = seed, counter = (agent, step, stream).
 *     One "vector step" (one choose_actions call, or one step of a rollout) consumes one step
 *     index; see oracle/draws.py for the exact protocol.
 */
#ifndef QLEARN_ENGINE_H
#define QLEARN_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QE_ABI_VERSION 2

typedef struct qe_engine qe_engine;
typedef struct qe_env qe_env;

enum qe_status {
    QE_OK = 0,
    QE_ERR_INVALID = -1,     /* bad argument (maps to Python ValueError / AssertionError) */
    QE_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime error */
    QE_ERR_OOM = -3,
    QE_ERR_UNSUPPORTED = -4, /* shape outside what a fused kernel supports */
    QE_ERR_INDEX = -5        /* state/action index out of range (NumPy would raise IndexError) */
};

enum qe_dtype { QE_F32 = 0, QE_F64 = 1 };

/* Update semantics of a batch of transitions.
 *   QE_LEARN_ITER : algorithms/base_algorithms/q_learning_optimal.py:770-817 (learn_iter, what
 *                   `learn` :893-934 dispatches to): strictly sequential over agents.
 *   QE_LEARN_VEC  : :819-891 (learn_vec / _learn_vec + add_q_values :235-250): all reads precede
 *                   all writes, colliding updates accumulate in agent order, each addition in float64 rounded into
 *                   the table dtype -- np.add.at exactly, at any number of collisions. */
enum qe_learn_mode { QE_LEARN_ITER = 0, QE_LEARN_VEC = 1 };

enum qe_env_kind {
    QE_ENV_HASH = 0,  /* HashTabularEnv (build-defined synthetic MDP) */
    QE_ENV_GRID = 1,  /* GridLakeEnv: FrozenLake-style side x side grid */
    QE_ENV_BANDIT = 2, /* environments/rigged_two_armed_bandit.py:55-80 */
    QE_ENV_TICTACTOE = 3, /* environments/tiktaktoe_mod.py:67-237 + flatten_multidiscrete_wrapper.py:106-161 */
    QE_ENV_TABLE = 4 /* a finite MDP given as tables (qe_env_create_table; not through qe_env_create) */
};

typedef struct qe_env_params {
    int32_t kind;          /* qe_env_kind */
    int32_t masked;        /* HASH: observations carry an action mask (TICTACTOE always does) */
    uint32_t seed;         /* HASH, GRID, TICTACTOE */
    int32_t p_term_256;    /* HASH: terminate when (hash & 0xff) < p_term_256 */
    int32_t side;          /* GRID */
    int32_t episode_len;   /* BANDIT */
    uint32_t agent_offset; /* global id of local agent 0 (multi-GPU sharding of agents) */
    int32_t reserved;
} qe_env_params;

typedef struct qe_rollout_stats {
    double kernel_ms;        /* HIP-event time of the timed region on the engine's stream */
    int64_t launches;        /* kernel launches issued (graph nodes count individually) */
    int64_t episodes;        /* episodes that ended during this rollout */
    int64_t involved;        /* agent-steps that went through the ordered (contested) path */
    int64_t episodes_dropped; /* episode-log overflow (0 unless capacity was exceeded) */
    double dominant_ms;      /* summed HIP-event time of the sampled dominant-kernel launches */
    int64_t dominant_launches; /* how many launches were sampled (<= 256, spread over the call) */
    int64_t dominant_env_steps; /* env-steps (agent x vector step) those sampled launches processed */
    double device_clock_ms;  /* persistent path: in-kernel constant-rate clock, launch start -> results published (0 otherwise) */
    double host_begin_us;    /* host time spent inside qe_rollout_begin (enqueue) ... */
    double host_end_us;      /* ... and inside qe_rollout_end (wait + result hand-over) */
    int64_t kernel_variant;  /* which kernel build ran.  bits 0-3 path: 1 step-wise, 2 persistent, 3 wide, 4 turnstile,
                                5 evaluation; persistent path: bits 4-5 LEAN (0 generic build, 1 plain training rollout,
                                2 the same with the delta log), bit 6 draw-producing helper wavefronts, bit 7 every lane an
                                agent, bit 8 built without the general ordered path ("light"), bit 9 the 512-agent build,
                                bit 10 the dataflow kernel (sharers of a row ordered by value hand-over in LDS),
                                bits 12-19 16-byte loads per row, bit 20 masked environment (tests assert on these);
                                path 6: population (qe_population_rollout), path 7: population greedy evaluation
                                (qe_population_evaluate), both with the same NV and masked bits; path 8: population with
                                an on-policy update rule (SARSA / Expected SARSA): those NV and masked bits, and the rule
                                (qe_update_rule) in bits 4-5; path 9: population with the double estimator (Double
                                Q-learning, qe_population_set_double) and path 10: its greedy evaluation, both with
                                the NV and masked bits of path 6; path 11: population with an n-step on-policy rule
                                (qe_population_set_n_step): the rule in bits 4-5, NV and masked as path 6, and n in
                                bits 24-28, which no other path uses; path 12: population with eligibility traces
                                (qe_population_set_traces): the rule in bits 4-5 (0 = Watkins's Q(lambda), 1 =
                                SARSA(lambda)), NV and masked as path 6, the slot count K in bits 24-29 and the trace
                                kind (qe_trace_kind) in bit 30, which no other field of that path uses; path 13:
                                population with Dyna-Q (qe_population_set_planning): NV and masked as path 6, and the
                                planning updates per step in bits 24-30 -- with bit 4 set the planning order is
                                prioritized sweeping (qe_population_set_sweeping) and bits 5-9 hold its queue length
                                minus 1; with bits 21-23 non-zero the model is the sample model
                                (qe_population_set_model_outcomes) and they hold its slots per cell minus 1, bits no
                                other path uses --; path 14: population with visit counts
                                (qe_population_set_visits): NV and masked as path 6, visit_lr in bit 4 and "some run's
                                beta is above 0" in bit 5; path 15: population with n-step Tree Backup
                                (qe_population_set_tree_backup): NV and masked as path 6, and n in bits 24-28 */
    int64_t complex_steps;   /* persistent path: vector steps that needed the general ordered path (full build); the
                                dataflow kernel reports its dataflow rounds beyond the first of a step instead */
} qe_rollout_stats;

/* ---- lifetime -------------------------------------------------------------------------------
 * qe_create      <- OptimalQLearningBase.__init__ (q_learning_optimal.py:84-98): zero (S, A) table,
 *                   seeds the draw protocol.  `device` = HIP device ordinal. */
int qe_abi_version(void);
const char* qe_last_error(void);
int qe_create(qe_engine** out, int64_t state_size, int32_t action_size, double discount_factor,
              uint64_t seed, int32_t dtype, int32_t device);
int qe_destroy(qe_engine* e);
int qe_synchronize(qe_engine* e);
/* Use the caller's HIP stream (hipStream_t as void*) instead of the engine's own. */
int qe_set_stream(qe_engine* e, void* hip_stream);
/* Tuning knobs (never change results).  QE_OPT_ROLLOUT_PATH: 0 = automatic, 1 = one kernel pair per
 * vector step, 2 = persistent single-workgroup kernel (needs num_agents <= 512 and num_agents *
 * lanes_per_row <= 1024), 3 = step-wise with chip-wide token rounds for the ordered path ("wide"),
 * 4 = one launch per vector step whose resident workgroups hand shared rows from agent to agent
 * ("turnstile": learn_iter, up to ~60 000 agents; where it does not apply the automatic choice is used). */
enum qe_option { QE_OPT_ROLLOUT_PATH = 0, QE_OPT_USE_GRAPH = 1 /* 1 (default): replay the step-wise kernels from a HIP graph */,
                 QE_OPT_TOKEN_ROUNDS = 2 /* wide mode: chip-wide rounds per step; 0 (default) = chosen from the previous call */,
                 QE_OPT_LISTED_MIN_AGENTS = 3 /* wide mode: agent count from which the rounds walk compacted lists (default 16384) */,
                 QE_OPT_EVENT_TIMING = 4 /* 1 (default): bracket every rollout with HIP events (kernel_ms); 0: persistent rollouts
                                            report the in-kernel clock only and put no event into the stream */,
                 QE_OPT_HOST_BLOCK = 5 /* 1 (default): a persistent rollout writes its results (control words, final observations,
                                          episode log) into page-locked host memory itself and qe_rollout_end spins on a sequence
                                          word there; 0: stream synchronisation + copies */,
                 QE_OPT_LANE_ORDERED_PATH = 6 /* persistent path, plain training rollouts of up to 128 agents: 0 (default) = automatic,
                                                 1 = the dataflow kernel (sharers of a row hand their values on in LDS), 2 = the
                                                 build with the general ordered path (deep chains of sharers), 3 = the sparse
                                                 build (rows rarely shared; full wavefronts only, else 1) */,
                 QE_OPT_TURN_FORWARD = 7 /* turnstile path, fp32 tables: 1 (default) = a row's progress word carries the value its last
                                            writer stored, successors whose view of the row can differ in that one column only take it
                                            from their poll; 0 = they always re-read the table (measurement switch) */,
                 QE_OPT_TURN_POLL = 8 /* turnstile path: 0 (default) = progress words are polled with returning atomics, 1 = with
                                         agent-scope loads (sc1); measured equal, kept as a measurement switch */,
                 QE_OPT_STAMP_HASH_BITS = 9 /* step-wise / wide paths: touch counters in 2^value hashed slots instead of one per
                                               row (rows that collide count as shared: a few more agents on the ordered path,
                                               same results); 0 (default) = automatic: 21 bits for tables of more than 2^22 rows,
                                               1 = one slot per row whatever the size */ };
int qe_set_option(qe_engine* e, int32_t option, int64_t value);

/* ---- Q-table I/O ----------------------------------------------------------------------------
 * q_table property / save (q_learning_optimal.py:96, 252-261), parallel_runtime.py:70-77,171-176
 * (rebind / copy back).  host buffers are C-contiguous (S, A) of `host_dtype`. */
int qe_table_upload(qe_engine* e, const void* host, int32_t host_dtype);
int qe_table_download(qe_engine* e, void* host, int32_t host_dtype);
/* Streaming form for save / load (:252-261; the table of BASELINE config 4 is 1.28 GB): rows
 * [first_row, first_row + rows) as a C-contiguous (rows, A) block in the TABLE's dtype. */
int qe_table_download_rows(qe_engine* e, void* host, int64_t first_row, int64_t rows);
int qe_table_upload_rows(qe_engine* e, const void* host, int64_t first_row, int64_t rows);
/* get_q_values / set_q_value(s) / add_q_values (:100-250); add follows np.add.at (duplicates
 * accumulate in index order). op: 0 = read into vals, 1 = write, 2 = add. */
int qe_table_cells(qe_engine* e, const int32_t* states, const int32_t* actions, int64_t n,
                   double* vals, int32_t op);
void* qe_table_dev(qe_engine* e);       /* device pointer of the table (for RCCL plumbing) */
int64_t qe_table_row_stride(qe_engine* e); /* ld, in elements */

/* ---- draw counter ---------------------------------------------------------------------------*/
int qe_set_step_counter(qe_engine* e, uint64_t step);  /* population: every run continues from `step` */
uint64_t qe_get_step_counter(qe_engine* e);            /* population: the counter of run 0 (see qe_population_step_counters) */
int qe_set_agent_offset(qe_engine* e, uint32_t offset); /* draw-protocol id of local agent 0 */

/* ---- action selection -----------------------------------------------------------------------
 * choose_actions and all eight variants behind it (q_learning_optimal.py:263-726): one kernel
 * family, same distribution, draws per oracle/draws.py.  masks: n*A bytes or NULL.
 * Returns -1 in out_actions[i] when agent i has no selectable action (as :302, :348).
 * `deterministic`: bit 0 = greedy selection (exploration rate ignored); bit 1 (QE_SELECT_NUMPY_EMPTY_MASK)
 * = the NumPy variants' treatment of an agent whose mask has no valid action: its greedy pick is
 * uniform over ALL actions (where(mask, Q, -inf) ties everywhere, :497-503, :618-628), only its
 * exploratory pick is impossible (-1; the reference raises IndexError, :470); the greedy pick is uniform over ALL
 * actions too when valid actions exist but every one of them holds -inf (the same tie); bit 2 (QE_SELECT_NUMPY_MAX) = the row
 * maximum is np.max (the NumPy variants, :428, :466, :548, :616): NaN as soon as a valid column holds one, so no
 * action ties with it (-1; the reference raises IndexError) -- without it the list variants' scan, which steps
 * over NaN columns (:290-296, :337-344).  Consumes one step index. */
#define QE_SELECT_DETERMINISTIC 1
#define QE_SELECT_NUMPY_EMPTY_MASK 2
#define QE_SELECT_NUMPY_MAX 4
int qe_choose_actions(qe_engine* e, const int32_t* states, int64_t n, const uint8_t* masks,
                      double exploration_rate, int32_t deterministic, int32_t* out_actions);

/* ---- learning -------------------------------------------------------------------------------
 * learn / learn_iter / learn_vec (q_learning_optimal.py:770-934). next_masks: n*A bytes or NULL. */
int qe_learn(qe_engine* e, const int32_t* states, const int32_t* actions, const float* rewards,
             const int32_t* next_states, const uint8_t* terminated, int64_t n, double lr,
             const uint8_t* next_masks, int32_t mode);

/* ---- device-resident environments + fused rollout -------------------------------------------
 * The batched env contract (environments/custom_env.py:31-84) as realised by
 * SyncVectorEnv(SAME_STEP) (benchmarks/throughput_benchmark.py:109-123). */
int qe_env_create(qe_env** out, qe_engine* e, int64_t num_agents, const qe_env_params* p);
/* A finite MDP given as tables (environments/device_envs.py:TabularMDPEnv encodes them).  Every (s, a) has `k` outcome
 * slots (1 <= k <= 8), element [(s * A + a) * k + j] of the four outcome arrays; the outcome is the first j < k - 1 with
 * u < thr[j], else slot k - 1 (unused slots repeat the last outcome), u a 32-bit word hashed from (agent_offset + agent,
 * seed, vector step).  On termination the next observation is drawn from the start support the same way (first j <
 * n_start - 1 with u' < start_thr[j], else the last entry; start_thr non-decreasing); the first reset draws from it too.
 * masks: S * A bytes (non-zero = valid) or NULL; with masks the observations carry them, as a masked HASH env's do.
 * All pointers are host pointers; the arrays are copied to the device and owned by the environment.  States out of
 * range -> QE_ERR_INDEX; bad k / n_start / shapes -> QE_ERR_INVALID.  params->kind must be QE_ENV_TABLE (seed,
 * agent_offset are used; masked is taken from `masks`). */
typedef struct qe_table_mdp {
    int32_t k;                  /* outcome slots per (state, action), 1..8 */
    int32_t n_start;            /* entries of the start support, >= 1 */
    const uint32_t* thr;        /* S*A*k */
    const int32_t* next_state;  /* S*A*k */
    const float* reward;        /* S*A*k */
    const uint8_t* terminated;  /* S*A*k */
    const uint32_t* start_thr;  /* n_start */
    const int32_t* start_state; /* n_start */
    const uint8_t* masks;       /* S*A or NULL */
} qe_table_mdp;
int qe_env_create_table(qe_env** out, qe_engine* e, int64_t num_agents, const qe_env_params* p, const qe_table_mdp* t);
int qe_env_destroy(qe_env* env);
int qe_env_reset(qe_env* env, int32_t has_seed, uint32_t seed);
/* current observations (+ masks n*A bytes, + per-agent running episode returns); any may be NULL */
int qe_env_observe(qe_env* env, int32_t* obs, uint8_t* masks, float* agent_rewards);
/* restore observations / env-internal counters / running returns (resume, curr_state_dict) */
int qe_env_restore(qe_env* env, const int32_t* obs, const uint32_t* aux, const float* agent_rewards);
int qe_env_aux(qe_env* env, uint32_t* aux);
/* host-driven env.step (actions in, transition out); outputs may be NULL */
int qe_env_step(qe_env* env, const int32_t* actions, int32_t* obs, float* rewards,
                uint8_t* terminated, uint8_t* masks);

/* qe_rollout <- SingleThreadQLearning.run_steps hot loop (single_thread_runtime.py:63-64) =
 * `steps` x BaseRuntime.run_single_step (base_runtime.py:184-222) incl. _learn's schedule reads
 * (:224-263).  eps[t], lr[t] are the schedule values the reference would read at vector step t.
 * trace_actions: optional host buffer steps*n int32 receiving every selected action (tests). */
int qe_rollout(qe_engine* e, qe_env* env, int64_t steps, const double* eps, const double* lr,
               int32_t mode, int32_t* trace_actions, qe_rollout_stats* stats);
/* Split form for pipelining: qe_rollout_begin only ENQUEUES a rollout (no host synchronisation) in
 * one of two slots; qe_rollout_end waits for that slot and fetches its statistics and episode log
 * (qe_episode_log then refers to it).  Beginning rollout k+1 before ending rollout k keeps the GPU
 * busy while the host post-processes, and lets the RCCL exchange of chunk k overlap chunk k+1.
 * qe_rollout == begin(slot 0) + end(slot 0). */
int qe_rollout_begin(qe_engine* e, qe_env* env, int64_t steps, const double* eps, const double* lr,
                     int32_t mode, int32_t slot);
int qe_rollout_end(qe_engine* e, int32_t slot, qe_rollout_stats* stats);
/* One call for a whole run_steps body (single_thread_runtime.py:63-75) that fits one launch: qe_rollout +
 * the episode log (first `cap` entries into ep_step / ep_ret; the rest stays available through
 * qe_episode_log) + the float32 running sum of the returns in log order (:67) + what the resume dict
 * needs (observations, env-internal state, running per-agent returns; any may be NULL).  Returns the
 * number of episodes that ended, or a negative qe_status. */
int64_t qe_rollout_fused(qe_engine* e, qe_env* env, int64_t steps, const double* eps, const double* lr, int32_t mode,
                         qe_rollout_stats* stats, int64_t cap, int32_t* ep_step, float* ep_ret, float* ret_sum,
                         int32_t* obs, uint32_t* aux, float* agent_rewards);
/* Largest `steps` of one qe_rollout / qe_rollout_begin / qe_evaluate call on this environment for which
 * the episode log cannot overflow even if every agent finishes an episode in every step (the caller
 * chops longer calls: single_thread_runtime.py:63-64 has no such limit). */
int64_t qe_rollout_chunk_limit(qe_engine* e, qe_env* env, int32_t learn);
/* Schedule plan: the eps[t] / lr[t] values of a whole training call (same meaning as in qe_rollout),
 * uploaded once.  Afterwards qe_rollout_begin may be called with eps == NULL and lr == NULL: each
 * such call consumes the next `steps` values of the plan, so a call chopped into many short rollouts
 * (replica exchange every 100 steps) pays for one upload instead of one per rollout.  A new plan
 * replaces the old one; it may only be set while no rollout is in flight. */
int qe_schedule_plan(qe_engine* e, const double* eps, const double* lr, int64_t count);
/* qe_evaluate <- BaseRuntime.evaluate_steps / evaluate_episodes (base_runtime.py:293-384): greedy,
 * no learning.  Runs `steps` vector steps. */
int qe_evaluate(qe_engine* e, qe_env* env, int64_t steps, qe_rollout_stats* stats);
/* Episode log of the last rollout/evaluate: (vector step within the call, agent, return), sorted
 * by (step, agent) = the order base_runtime.py:218-221 appends.  Returns the count; copies at most
 * `cap` entries. */
int64_t qe_episode_log(qe_engine* e, int64_t cap, int32_t* step, int32_t* agent, float* ret);

/* ---- multi-GPU replica sync (replaces the MPI tier, q_learning_async_dist.py:164-357) ---------
 * Each GPU logs (cell, delta) for its own updates into a caller-owned device buffer of
 * capacity entries x 8 bytes {uint32 cell; float delta}; remote logs are applied with atomicAdd.
 * Slot of a record: (vector steps logged so far) * N + agent, cell = state * row_stride + action.
 * Capacity rule: WHOLE STEPS ONLY.  A vector step is logged when all N of its records fit below `capacity`; a step
 * that does not fit -- and every later one -- writes nothing, on every kernel path, and qe_delta_log_count (a multiple
 * of N) counts only records that were written.  Slots from the count on are never touched.  qe_delta_log_reset
 * restarts at slot 0; attach(NULL, 0) detaches.
 * Limits: float32 tables only (attach and the apply entry points answer QE_ERR_UNSUPPORTED otherwise).  A record
 * holds the cell in 32 bits; qe_create admits no table of 2^32 cells or more (S * row_stride, padded rows included),
 * so every cell of an engine's table can be named.  The apply kernels skip
 * records whose cell lies outside the table and count them; the next qe_synchronize or qe_table_download reports
 * QE_ERR_INDEX once (the valid records have been applied). */
int qe_delta_log_attach(qe_engine* e, void* dev_buf, int64_t capacity);
int64_t qe_delta_log_count(qe_engine* e);
int qe_delta_log_reset(qe_engine* e);
int qe_delta_apply_dev(qe_engine* e, const void* dev_entries, int64_t count);
/* Same over an all-gathered buffer: applies entries [0, count) except [skip_begin, skip_end) -- this
 * rank's own segment, which is already in its table -- in ONE launch. */
int qe_delta_apply_skip_dev(qe_engine* e, const void* dev_entries, int64_t count, int64_t skip_begin,
                            int64_t skip_end);

/* Deterministic form: `dev_entries` holds the OTHER ranks' records stably sorted by cell (so that within a
 * cell they are in rank-major, slot-minor order); every cell receives its additions sequentially in that
 * order -- no float atomics, the same result on every run. */
int qe_delta_apply_sorted_dev(qe_engine* e, const void* dev_entries, int64_t count);
/* The whole apply step of one exchange: `gathered_dev` is the all-gathered buffer, `world` segments of `capacity`
 * records of which the first `count` are valid; the records of every rank but `rank` are stably sorted by cell inside
 * the engine (radix sort, csrc/qe_delta_sort.h) and added per cell in rank-major, slot-minor order.  Same result as
 * qe_delta_apply_sorted_dev over the concatenated, stably sorted records; nothing but HIP kernels on the engine's stream.
 * (Stands in for the parameter server's apply loop, q_learning_async_dist.py:359-447.) */
int qe_delta_apply_gathered_dev(qe_engine* e, const void* gathered_dev, int64_t capacity, int64_t count, int32_t world,
                                int32_t rank);

/* ---- population: many independent single-agent runs in one launch ------------------------------------
 * M runs of the classic one-agent Q-learner (SingleThreadQLearning with one environment, single_thread_runtime.py)
 * share one MDP and one seed; run r is, bit for bit, the standalone one-agent rollout on the same environment kind with
 * agent_offset = (the environment's agent_offset) + r, its own schedules and discount.
 *   qe_create_population  an engine whose table holds runs * state_size rows (run r: rows r*S .. r*S+S-1); its
 *                         environments (num_agents must equal runs) move in states [0, state_size).  qe_table_upload /
 *                         qe_table_download[_rows] / qe_table_cells see the whole [runs * S, A] table.  Rows of at
 *                         most 64 actions (QE_ERR_UNSUPPORTED beyond).  Every rollout, learn, choose, evaluate, replay
 *                         and delta-log entry point above returns QE_ERR_UNSUPPORTED on it.
 *   qe_population_configure  per-run schedule descriptors (eps, lr: runs entries each) and discounts (runs doubles);
 *                         any of the three may be NULL (left as they are; initially constant 0 and discount 0).
 *   qe_population_schedules  the per-run schedule values now (either pointer may be NULL).
 *   qe_population_rollout  `steps` steps of every run (schedules advance once per step, as update(1) after each read).
 *                         Per-run outputs, each `runs` entries, any may be NULL: episodes ended, float32 sequential sum
 *                         of their returns, observations, env-internal state, running returns, status (1 = some step
 *                         had no selectable action: the call returns QE_ERR_INDEX after filling the outputs, the other
 *                         runs are unaffected).  `log` != 0 keeps the episode log of the call (qe_population_log).
 *                         Returns the number of episodes that ended, or a negative qe_status.
 *   qe_population_evaluate  greedy evaluation of every run: run r is the standalone one-agent evaluate_steps (episodes
 *                         == 0: `steps` steps) or evaluate_episodes (episodes > 0: the run stops at the end of the step in
 *                         which its episode count reaches `episodes`, or after `steps` steps, whichever comes first; no
 *                         launch follows once every run has stopped).  Tables and schedules are untouched; the
 *                         environment state moves on.  Per-run outputs, each `runs` entries, any may be NULL: episodes
 *                         ended, float32 sequential sum of their returns, steps taken, status (bit 0: some step had no
 *                         selectable action -- QE_ERR_INDEX after filling the outputs; bit 1: episode mode stopped by
 *                         the bound `steps`, not an error).  `log` as for qe_population_rollout.  Returns the number of
 *                         episodes that ended, or a negative qe_status.
 *   qe_population_log     the latest call's episode log in (run, episode) order: step within the call and return of
 *                         the first `cap` entries; returns the count.
 *   qe_population_step_counters / qe_population_set_step_counters  every run's draw counter (`runs` entries).  Each
 *                         call of the rollout or of a step-mode evaluation advances every run by `steps`; an
 *                         episode-mode evaluation advances run r by the steps it took, so the counters may differ.
 *   qe_population_set_update_rule  the TD target of every run of the population (one rule per population):
 *                         Q-learning (the default) bootstraps from max Q[s', .]; SARSA from Q[s', a'] with a' the action
 *                         the run takes next (chosen before the update, with the draws and epsilon of the next step);
 *                         Expected SARSA from (1 - eps') * max + eps' * mean of Q[s', valid], eps' the next step's epsilon
 *                         clamped to [0, 1].  Not a population engine or an unknown rule -> QE_ERR_INVALID.  Greedy
 *                         evaluation does not depend on the rule.  qe_population_update_rule returns the rule (or a
 *                         negative qe_status).
 *   qe_population_pending_actions / qe_population_set_pending_actions  SARSA's run state besides the tables: the action
 *                         already chosen for each run's next step (`runs` entries, -1 = none: the run picks at its next
 *                         step).  The rollout leaves it behind; set it (NULL: none for every run) when the environment
 *                         state is restored or reset.  Entries outside [-1, action_size) -> QE_ERR_INVALID.  Other rules
 *                         neither read nor write it.
 *   qe_population_set_double / qe_population_double  the double estimator (Double Q-learning, van Hasselt 2010): every run
 *                         owns two tables, A (the engine's table: every qe_table_* entry point keeps seeing A only) and B
 *                         (a second allocation of the same shape and row stride, zero when the switch is turned on, freed
 *                         when it is turned off).  A run picks from the sum row T(A[s, .] + B[s, .]); bit 31 of the unused
 *                         fourth word of the step's policy draws chooses the table X that is updated (0: A, 1: B), and
 *                         X[s, a] bootstraps from Y[s', argmax X[s', valid]], Y the other table (first index of the
 *                         maximum, a NaN counting as the maximum).  Greedy evaluation picks from the sum row.  An
 *                         orthogonal switch, not an update rule: it exists for Q-learning only.  Not a population engine
 *                         -> QE_ERR_INVALID; the update rule is not Q-learning -> QE_ERR_UNSUPPORTED, and so is
 *                         qe_population_set_update_rule to another rule while the switch is on.  qe_population_double
 *                         returns 1 / 0 (or a negative qe_status).
 *   qe_population_table_b_upload / _download / _download_rows  qe_table_upload / qe_table_download /
 *                         qe_table_download_rows on table B; QE_ERR_INVALID while the switch is off.
 *   qe_population_set_n_step / qe_population_n_step  the bootstrapping horizon n of the on-policy rules, 1 (the default:
 *                         the one-step rules above) .. 16: n-step SARSA and n-step Expected SARSA (Sutton & Barto ch. 7).
 *                         A run keeps a window of its last transitions (s, a, r), at most n - 1 between steps.  Each step
 *                         appends one; a window of n entries updates and drops its oldest one, a terminated step updates
 *                         all of them, oldest first, and empties the window.  Entry j bootstraps from the fold of the
 *                         later rewards onto the one-step rule's scalar v of this step: g_L = v, g_i = T(r_i + gamma *
 *                         g_{i+1}), with the arithmetic of the learn mode.  Setting n empties every window.  Not a
 *                         population engine or n out of range -> QE_ERR_INVALID.  n > 1 while the rule is Q-learning (an
 *                         uncorrected n-step Q-learning is no off-policy method; qe_population_set_tree_backup is) or the double switch is on ->
 *                         QE_ERR_UNSUPPORTED, and so is switching to either of those while n > 1.  Greedy evaluation
 *                         neither reads nor clears the windows.
 *   qe_population_window / qe_population_set_window  the windows, run state besides the tables and the pending actions:
 *                         `len` has `runs` entries (0 .. n - 1), `states`, `actions` and `rewards` runs * (n - 1), run r's
 *                         entries at [r * (n - 1) + i], oldest first; unused slots read 0 and are ignored when set.  The
 *                         rollout leaves them behind; set them (len NULL: every window empty, its entries are never
 *                         updated) when the environment state is restored or reset.  A length above n - 1, or a state or
 *                         action outside the table -> QE_ERR_INVALID.  With n = 1 there is nothing to read or set.
 *   qe_population_set_tree_backup / qe_population_tree_backup  n-step Tree Backup under a greedy target policy (Sutton &
 *                         Barto 7.5), the n-step form of Q-learning: the horizon n, 1 (the default: the one-step kernel,
 *                         nothing allocated) .. 16.  An orthogonal switch like the double estimator, not an update rule and
 *                         not n_step.  A run keeps a window of entries (s, a, r, f), at most n - 1 between steps; f says
 *                         whether a was greedy: Q[s, a] == np.max(Q[s, valid]) on the row the pick saw (a NaN maximum is
 *                         never equal).  A step is Q-learning's step up to the bootstrap v = np.max(Q[s', valid]); it
 *                         appends its entry; a window of n entries updates and drops its oldest one, a terminated step
 *                         updates all of them, oldest first, and empties the window.  Entry j bootstraps from g_{j+1}:
 *                         g_L = v; for j < i < L, g_i = T(r_i + gamma * g_{i+1}) with the arithmetic of the learn mode if
 *                         f_i, else np.max(Q[s_i, valid(s_i)]) as the table stands at that update -- so only the nearest
 *                         non-greedy entry after j matters, and the flag of entry j itself is not read.  Setting n empties
 *                         every window.  Not a population engine or n out of range -> QE_ERR_INVALID.  n > 1 while the rule
 *                         is not Q-learning, the double switch is on, n_step > 1, traces are on, planning is on or visit
 *                         counts are on -> QE_ERR_UNSUPPORTED, and so is switching to any of those while n > 1.  Greedy
 *                         evaluation neither reads nor clears the windows.
 *   qe_population_tree_window / qe_population_set_tree_window  those windows, run state besides the tables: `len` has
 *                         `runs` entries (0 .. n - 1), `states`, `actions`, `rewards` and `greedy` (0 or 1) runs * (n - 1),
 *                         run r's entries at [r * (n - 1) + i], oldest first; unused slots read 0 and are ignored when set.
 *                         Set them (len NULL: every window empty, its entries are never updated) when the environment
 *                         state is restored or reset.  A length above n - 1, a state or action outside the table, or a flag
 *                         other than 0 or 1 -> QE_ERR_INVALID.  With n = 1 there is nothing to read or set.
 *   qe_population_set_traces  eligibility traces (Sutton & Barto ch. 12): SARSA(lambda) under QE_RULE_SARSA, Watkins's
 *                         Q(lambda) under QE_RULE_Q_LEARNING.  `lambda` has `runs` entries in [0, 1]; NULL turns traces off
 *                         (the one-step kernels, the default) and frees the slots.  Every run keeps K slots (s_i, a_i, e_i),
 *                         K in 1 .. 32, e_i of the table dtype T; a slot with e_i == 0 is free and live slots name distinct
 *                         cells.  A step computes the one-step rule's increment u of Q[s, a] without storing the cell,
 *                         marks (s, a) -- e = 1 (QE_TRACE_REPLACING) or e + 1 (QE_TRACE_ACCUMULATING) if a live slot holds
 *                         it, else the lowest free slot, else the slot of the smallest e (lowest index among equals) takes
 *                         (s, a, 1) -- then adds u * e_i to the cell of every live slot (one product and one add in T; vec
 *                         mode on a float32 table: in float64, rounded once) and decays: e_i = 0 after a terminated step,
 *                         else e_i = T(e_i * d) with d = T(gamma * lambda), one float64 product rounded once.  Q(lambda)
 *                         zeroes every e_i before the mark when the action taken is not a greedy one (Q[s, a] != max Q[s,
 *                         valid]).  Setting traces frees every slot.  Not a population engine, K or kind out of range ->
 *                         QE_ERR_INVALID; the rule is Expected SARSA, the double switch is on, n > 1, a lambda outside
 *                         [0, 1] or not finite, or a d outside [0, 1] -> QE_ERR_UNSUPPORTED, and so is switching to Expected
 *                         SARSA, the double estimator or n > 1 while traces are on.  Greedy evaluation neither reads nor
 *                         clears the slots.
 *   qe_population_trace_config  returns 1 while traces are on, else 0 (or a negative qe_status); K (0 while off), the
 *                         kind and the `runs` lambdas go to the pointers that are not NULL.
 *   qe_population_traces / qe_population_set_trace_state  the slots, run state besides the tables and the pending
 *                         actions: runs * K entries each, run r's slot i at [r * K + i], values as float64 (exact for
 *                         either dtype); free slots read (0, 0, 0.0).  The rollout leaves them behind; set them (all three
 *                         NULL: every slot free) when the environment state is restored or reset.  QE_ERR_INVALID while
 *                         traces are off, and from the setter for a state or action outside the table, a value that is
 *                         negative, not finite or not representable in T, or two live slots of one run naming one cell.
 *   qe_population_set_planning  Dyna-Q (Sutton & Barto ch. 8): n planning updates after every training step, n in 0 .. 64;
 *                         0 (the default) turns planning off and forgets the model.  Every run keeps a model -- for every
 *                         cell c = s * A + a its last observed outcome (next_obs, reward, terminated), or "unseen" -- and
 *                         the list of its seen cells in order of first observation.  A step with draw counter k is
 *                         Q-learning's step; then model[s, a] = (s', r, terminated), s' the observation the environment
 *                         returns (an unseen cell joins the list first); then, for i = 0 .. n-1 in order: x_i = word i & 3
 *                         of the Philox block (agent id, k_lo, k_hi, 2 | (i >> 2) << 8) under the engine's seed,
 *                         c_i = list[mulhi32(x_i, count)], (p, rho, tau) = model[c_i], m_i = the maximum of row p over the
 *                         environment's valid columns for observation p as the table stands then (a NaN there: NaN; no
 *                         valid column: -inf) and Q[c_i] = the step's update of (Q[c_i], rho, m_i, tau) with the learning
 *                         rate of step k.  The model outlives calls and environment resets; greedy evaluation neither
 *                         reads nor writes it.  Setting n > 0 while planning is on keeps the model.  Not a population
 *                         engine or n out of range -> QE_ERR_INVALID; a rule other than Q-learning, the double switch on,
 *                         n_step > 1, traces on, or a run's table of 2^31 cells or more (state_size * row stride) ->
 *                         QE_ERR_UNSUPPORTED, and so is switching to any of those while planning is on.
 *   qe_population_planning  n, 0 while planning is off (or a negative qe_status).
 *   qe_population_model / qe_population_set_model  the model and the list: next_states (-1: unseen), rewards and
 *                         terminated hold runs * S * A entries, run r's cell c at [r * S * A + c]; visited holds
 *                         runs * S * A cells, run r's j-th at [r * S * A + j], -1 from count[r] on; count holds runs
 *                         entries.  The download fills the pointers that are not NULL (unseen cells read -1, 0.0f, 0).
 *                         The upload takes all five, or all NULL: every run forgets everything.  QE_ERR_INVALID while
 *                         planning is off, and from the upload for a next state outside [0, S) that is not -1, a count
 *                         that differs from the number of seen cells, or a list entry (below count) that is out of range,
 *                         unseen in the model or listed twice; entries from count on and the rewards and flags of unseen
 *                         cells are not read.  While sweeping is on (below) the upload also rebuilds every predecessor
 *                         list in its canonical order and empties every queue.
 *   qe_population_set_model_outcomes  the sample model of Sutton & Barto ch. 8 for stochastic environments: K slots per cell,
 *                         K in 1 .. 8; 1 (the default) is the last-outcome model above.  It needs planning on.  K > 1: every
 *                         cell keeps up to K distinct outcomes (next_obs, reward, terminated) with a uint32 count each;
 *                         occupied slots form a prefix in order of first observation, and a cell is seen when slot 0 is
 *                         occupied.  Learning (s', r, terminated) of (s, a): a slot MATCHES when its reward has the same 32
 *                         bits, its flag is the same, and the flag is set or its next_obs is s'.  On a match the slot's
 *                         next_obs becomes s' and its count goes up by one unless the cell's total N (the sum of its
 *                         counts) is 2^32 - 1; else the first free slot, or with none free the slot with the smallest count
 *                         (the lowest index among equals), becomes (s', r, terminated, 1).  Planning update i draws c_i as
 *                         above, then y_i = word i & 3 of the Philox block (agent id, k_lo, k_hi, 3 | (i >> 2) << 8),
 *                         t = mulhi32(y_i, N(c_i)), and takes (p, rho, tau) from the first slot j with t < n_0 + .. + n_j;
 *                         the rest is the update above.  Changing K forgets the model, setting the same K keeps it, and
 *                         turning planning off frees it (K is 1 again).  QE_ERR_INVALID: not a population engine, K out of
 *                         range or planning off; QE_ERR_UNSUPPORTED: K > 1 while sweeping is on (sweeping over a sample
 *                         model needs expected updates, which are not built; qe_population_set_sweeping is refused likewise
 *                         while K > 1), or a (dtype, row stride) whose kernel is not built.
 *   qe_population_model_outcomes  K (or a negative qe_status).
 *   qe_population_outcome_model / qe_population_set_outcome_model  the sample model (K > 1) and the list: next_states,
 *                         rewards, terminated and counts hold runs * S * A * K entries, slot j of run r's cell c at
 *                         [(r * S * A + c) * K + j]; a free slot reads -1, 0.0f, 0, 0; visited and count as above.  The
 *                         upload takes all six, or all NULL: every run forgets everything.  It refuses (QE_ERR_INVALID, and
 *                         nothing changes) what the checks above refuse and: an occupied slot behind a free one, an
 *                         occupied slot with count 0 or a free one with another count, two slots of a cell that match each
 *                         other, and a cell whose counts add up to more than 2^32 - 1.  While K > 1, qe_population_model
 *                         returns QE_ERR_UNSUPPORTED (read the model here) and qe_population_set_model loads its
 *                         last-outcome model as slot 0 with count 1.  QE_ERR_INVALID while planning is off or K is 1.
 *   qe_population_set_sweeping  prioritized sweeping (Moore & Atkeson 1993; Sutton & Barto 8.4) as the order of the planning
 *                         updates: queue_length slots per run, 1 .. 32, and every run's threshold theta (finite, >= 0);
 *                         queue_length 0 (thresholds ignored) turns it off, frees the index and the queues, and gives
 *                         uniform Dyna-Q back.  It needs planning on.  Every run keeps, beside the model, a predecessor
 *                         list per state x -- the seen cells whose model entry is (x, ., terminated = 0), most recently
 *                         linked first -- and a queue of K (cell, priority) slots.  With inc(c, rho, m, tau) the increment
 *                         the step's update of (Q[c], rho, m, tau) reports (of the table dtype; on a float32 table in vec
 *                         mode the float64 increment before it is rounded), P(u) = |float64(u)| and rowmax(p) the maximum
 *                         of row p over its valid columns as the table stands, a step with draw counter k is: Q-learning's
 *                         step with increment u0; the model learns (s, a) -> (s', r, terminated) -- a linked cell whose next
 *                         state changes or that turns terminated is unlinked by a walk from the head of its list, a cell
 *                         that is not terminated and not linked goes to the head of the list of s', a cell whose next
 *                         state and flag did not change keeps its place --; if P(u0) > theta, propagate(s); then at most n
 *                         times: stop if the queue is empty, c = pop(), (p, rho, tau) = model[c], Q[c] = the update of
 *                         (Q[c], rho, rowmax(p), tau) with the learning rate of step k and increment u, and if
 *                         P(u) > theta, propagate(c / A).  propagate(x): m = rowmax(x); for every cell d of the list of x,
 *                         head to tail, u = inc(d, model[d].reward, m, false) -- nothing is stored -- and if P(u) > theta,
 *                         insert(d, P(u)).  insert(c, P): a live slot holding c keeps max(old, P); else the lowest free
 *                         slot takes it; else the slot of the smallest priority (lowest index among equals) is replaced if
 *                         P is strictly greater, and the newcomer is dropped if not.  pop(): the slot of the largest
 *                         priority, lowest index among equals; it becomes free.  No draw is consumed and a NaN increment
 *                         is never queued.  The index is knowledge like the model, the queue is run state like the trace
 *                         slots.  Turning it on (or changing queue_length) builds the canonical index of the model in hand
 *                         and empties the queues.  QE_ERR_INVALID: not a population engine, planning off, queue_length out
 *                         of range, thresholds NULL, negative or not finite; QE_ERR_UNSUPPORTED: a (dtype, row stride)
 *                         whose kernel is not built.
 *   qe_population_sweeping  queue_length, 0 while sweeping is off (or a negative qe_status).
 *   qe_population_predecessors / qe_population_set_predecessors  the index: head holds runs * S entries, the cell s * A + a
 *                         at the head of each state's list or -1; next holds runs * S * A entries, the next cell of the
 *                         same list, -1 at a tail and at a cell that is not linked.  The upload takes both, or both NULL:
 *                         the canonical index of the model in hand -- its seen cells with terminated == 0 linked in
 *                         visited-list order, each at the head of its next state's list.  An upload is checked against
 *                         the model in hand, in O(S * A) per run: every node reached from head[x] is in range, seen, not
 *                         terminated and has next state x, no node is reached twice, the nodes reached are all the seen
 *                         cells that are not terminated, and every other cell holds -1; anything else is QE_ERR_INVALID and
 *                         changes nothing.  Either upload empties every queue.
 *   qe_population_queue / qe_population_set_queue  the queues: cells and priorities hold runs * K entries, run r's slot i at
 *                         [r * K + i]; a free slot reads (-1, 0.0).  The upload takes both, or both NULL: every queue
 *                         empty.  QE_ERR_INVALID from the upload for a cell that is out of range, unseen in the model or
 *                         held by two slots of a run, a priority that is NaN or negative, or a free slot whose priority
 *                         is not 0.  The four are QE_ERR_INVALID while sweeping is off.
 *   qe_population_set_visits  per-cell visit counts N(s, a) of every run, uint32, zero when counting is turned on, with a
 *                         count-based optimism bonus and, with visit_lr != 0, the sample-average learning rate.  `bonus`
 *                         holds every run's beta (NULL: all zero); NULL with visit_lr == 0 turns counting off and forgets
 *                         the counts.  bonus(beta, N) = T(0) when beta == 0, else T(beta / sqrt(float64(N))): a float64
 *                         square root and division and one rounding to the table dtype T; N == 0 gives +inf.  A training
 *                         step is Q-learning's step with three changes: the pick (same draws, same selection variant)
 *                         sees the score row Q[s, j] + bonus(beta, N[s, j]) -- one add in T over the valid columns, a NaN
 *                         there like any other -- while the prediction stays Q[s, a]; after the environment step N[s, a]
 *                         becomes N[s, a] + 1, saturating at 2^32 - 1 (a step without a selectable action counts at action
 *                         0); with visit_lr the update takes lr / float64(N[s, a]), the incremented count, rounded to float
 *                         on a float32 table as lr is.  The target stays the maximum of plain Q.  The counts are
 *                         knowledge: they outlive calls and environment resets, and the evaluation calls neither read nor
 *                         write them.  Turning counting on again while it is on keeps the counts.  Not a population engine
 *                         -> QE_ERR_INVALID; a rule other than Q-learning, the double switch on, n_step > 1, traces on,
 *                         planning on, a beta that is negative or not finite, or a (dtype, row stride) whose kernel is
 *                         not built -> QE_ERR_UNSUPPORTED, and so is switching to any of those modes while counting is on.
 *   qe_population_visits  whether counting is on, visit_lr, and (while on) every run's beta; any pointer may be NULL.
 *   qe_population_visit_counts / qe_population_set_visit_counts  the counts, runs * S * A entries, run r's cell (s, a) at
 *                         [(r * S + s) * A + a]; the upload takes NULL for "all zero" and rewrites the bonus plane.
 *   qe_population_visit_bonus  the bonus the next pick adds to every cell, the same layout, as `dtype` (QE_F32 / QE_F64).
 *                         The three are QE_ERR_INVALID while counting is off. */
enum qe_trace_kind { QE_TRACE_REPLACING = 0, QE_TRACE_ACCUMULATING = 1 };
enum qe_update_rule { QE_RULE_Q_LEARNING = 0, QE_RULE_SARSA = 1, QE_RULE_EXPECTED_SARSA = 2 };
enum qe_run_schedule_kind { QE_SCHED_CONSTANT = 0, QE_SCHED_LINEAR = 1, QE_SCHED_EXPONENTIAL = 2 };
typedef struct qe_run_schedule {
    double value;      /* the value read at the next step */
    double min_value;  /* EXPONENTIAL: floor, v <- max(v * factor, min_value) */
    double factor;     /* EXPONENTIAL: decay_rate ** 1; LINEAR: 1 * decay_rate, v <- v + factor */
    int32_t kind;      /* qe_run_schedule_kind */
    int32_t reserved;
} qe_run_schedule;
int qe_create_population(qe_engine** out, int64_t runs, int64_t state_size, int32_t action_size, uint64_t seed,
                         int32_t dtype, int32_t device);
int64_t qe_population_runs(qe_engine* e); /* 0: not a population engine */
int qe_population_configure(qe_engine* e, const qe_run_schedule* eps, const qe_run_schedule* lr, const double* gamma);
int qe_population_schedules(qe_engine* e, double* eps_values, double* lr_values);
int64_t qe_population_rollout(qe_engine* e, qe_env* env, int64_t steps, int32_t mode, int32_t log, qe_rollout_stats* stats,
                              int64_t* ep_count, float* ep_sum, int32_t* obs, uint32_t* aux, float* agent_rewards,
                              uint32_t* status);
int64_t qe_population_evaluate(qe_engine* e, qe_env* env, int64_t steps, int64_t episodes, int32_t log,
                               qe_rollout_stats* stats, int64_t* ep_count, float* ep_sum, int64_t* used, uint32_t* status);
int64_t qe_population_log(qe_engine* e, int64_t cap, int32_t* step, float* ret);
int qe_population_step_counters(qe_engine* e, uint64_t* out);
int qe_population_set_step_counters(qe_engine* e, const uint64_t* in);
int qe_population_set_update_rule(qe_engine* e, int32_t rule);
int qe_population_update_rule(qe_engine* e);
int qe_population_pending_actions(qe_engine* e, int32_t* out);
int qe_population_set_pending_actions(qe_engine* e, const int32_t* in);
int qe_population_set_double(qe_engine* e, int32_t on);
int qe_population_double(qe_engine* e);
int qe_population_table_b_upload(qe_engine* e, const void* host, int32_t host_dtype);
int qe_population_table_b_download(qe_engine* e, void* host, int32_t host_dtype);
int qe_population_table_b_download_rows(qe_engine* e, void* host, int64_t first_row, int64_t rows);
int qe_population_set_n_step(qe_engine* e, int32_t n);
int qe_population_n_step(qe_engine* e);
int qe_population_window(qe_engine* e, int32_t* len, int32_t* states, int32_t* actions, float* rewards);
int qe_population_set_window(qe_engine* e, const int32_t* len, const int32_t* states, const int32_t* actions,
                             const float* rewards);
int qe_population_set_tree_backup(qe_engine* e, int32_t n);
int qe_population_tree_backup(qe_engine* e);
int qe_population_tree_window(qe_engine* e, int32_t* len, int32_t* states, int32_t* actions, float* rewards, uint8_t* greedy);
int qe_population_set_tree_window(qe_engine* e, const int32_t* len, const int32_t* states, const int32_t* actions,
                                  const float* rewards, const uint8_t* greedy);
int qe_population_set_traces(qe_engine* e, int32_t trace_length, int32_t trace_kind, const double* lambda);
int qe_population_trace_config(qe_engine* e, int32_t* trace_length, int32_t* trace_kind, double* lambda);
int qe_population_traces(qe_engine* e, int32_t* states, int32_t* actions, double* values);
int qe_population_set_trace_state(qe_engine* e, const int32_t* states, const int32_t* actions, const double* values);
int qe_population_set_planning(qe_engine* e, int32_t planning_steps);
int qe_population_planning(qe_engine* e);
int qe_population_model(qe_engine* e, int32_t* next_states, float* rewards, uint8_t* terminated, int32_t* visited,
                        int32_t* count);
int qe_population_set_model(qe_engine* e, const int32_t* next_states, const float* rewards, const uint8_t* terminated,
                            const int32_t* visited, const int32_t* count);
int qe_population_set_model_outcomes(qe_engine* e, int32_t model_outcomes);
int qe_population_model_outcomes(qe_engine* e);
int qe_population_outcome_model(qe_engine* e, int32_t* next_states, float* rewards, uint8_t* terminated, uint32_t* counts,
                                int32_t* visited, int32_t* count);
int qe_population_set_outcome_model(qe_engine* e, const int32_t* next_states, const float* rewards, const uint8_t* terminated,
                                    const uint32_t* counts, const int32_t* visited, const int32_t* count);
int qe_population_set_sweeping(qe_engine* e, int32_t queue_length, const double* thresholds /* [runs] */);
int qe_population_sweeping(qe_engine* e);
int qe_population_predecessors(qe_engine* e, int32_t* head, int32_t* next);
int qe_population_set_predecessors(qe_engine* e, const int32_t* head, const int32_t* next);
int qe_population_queue(qe_engine* e, int32_t* cells, double* priorities);
int qe_population_set_queue(qe_engine* e, const int32_t* cells, const double* priorities);
int qe_population_set_visits(qe_engine* e, const double* bonus /* [runs]; NULL: all zero */, int32_t visit_lr);
int qe_population_visits(qe_engine* e, int32_t* on, int32_t* visit_lr, double* bonus);
int qe_population_visit_counts(qe_engine* e, uint32_t* out);
int qe_population_set_visit_counts(qe_engine* e, const uint32_t* in /* NULL: zero */);
int qe_population_visit_bonus(qe_engine* e, void* out, int32_t dtype);

/* ---- dynamic programming over a QE_ENV_TABLE environment (Sutton & Barto ch. 4; csrc/qe_mdp_solve.h) ------------------
 * The MDP is the law the environment samples from, read from its device records.  For (s, a) with k slots and a running
 * maximum t = 0: slot j < k - 1 weighs w_j = max(0, thr_j - t), then t = max(t, thr_j); slot k - 1 weighs 2^32 - t;
 * p_j = w_j * 2^-32 (exact in float64).  Backup of a cell over a float64 value vector V:
 *     acc = 0.0;  for j ascending with w_j > 0:  x = double(r_j) + (terminated_j ? 0.0 : gamma * V[next_j]);  acc = acc + p_j * x
 * (one product, one add, no contraction; a terminated outcome bootstraps 0 and the auto-reset successor plays no part).
 * The valid columns of s are the environment's mask for s, or all of them; a state without one has value 0.0.
 *
 * qe_env_table_solve: value iteration.  V_0 = 0; sweep t >= 1: Q_t[s,a] = backup(s, a; V_{t-1}) for every cell, masked ones
 * included, V_t[s] = max over the valid a, res_t = max_s |V_t[s] - V_{t-1}[s]|; every sweep reads only V_{t-1}.  The result
 * is (Q_t, V_t) of the first t with res_t <= tol, else of t = max_sweeps; *sweeps_out = t, *residual_out = res_t.  Returns
 * 1 = stopped by tol, 0 = by max_sweeps.  gamma in [0, 1], tol >= 0, both finite, 1 <= max_sweeps: else QE_ERR_INVALID.  An
 * environment of another kind is QE_ERR_UNSUPPORTED.  Any action_size a device environment admits; works on the
 * environment of a population engine as well (the MDP of one run).
 *
 * qe_population_policy_values: the exact value of every run's greedy policy.  In state s of run r, row = the run's table
 * row in the table dtype (double estimator on: A[s,.] + B[s,.], one addition in that dtype, as its greedy evaluation forms
 * it), m = the maximum of the valid columns, G = the valid columns with row[a] == m: greedy selection with uniform
 * tie-breaking, as qe_population_evaluate performs it (the 2^-32 bias of its pick is ignored).  V_0[r,.] = 0;
 *     V_t[r,s] = (sum over a in G, ascending, from 0.0, of backup(s, a; V_{t-1}[r,.])) / double(|G|),  0.0 if G is empty;
 * res_t[r] = max_s |V_t[r,s] - V_{t-1}[r,s]|.  Run r freezes at its first t with res_t[r] <= tol: v_out[r,.] = V_t[r,.],
 * sweeps_out[r] = t, residual_out[r] = res_t[r], and later sweeps neither read nor write it; else it stops at max_sweeps.
 * gammas: one discount per run, each in [0, 1], or NULL for the runs' own (qe_population_configure); 1.0 gives the
 * undiscounted return qe_population_evaluate reports.  status_out[r]: bit 0 = some state of the run has no valid column
 * (informational), bit 1 = a valid cell of the run's row (as formed above) is NaN: its values and residual are NaN and its
 * sweeps 0.  Returns the number of runs stopped by tol.  Tables, schedules, draw counters, environment state, windows,
 * traces and model are not touched; any output may be NULL.  An engine that is not a population, or not the
 * environment's, is QE_ERR_INVALID.
 *
 * Both enqueue their sweeps in batches on the engine's stream and synchronise once per batch; their device buffers live
 * for the call (allocation failure: QE_ERR_OOM, nothing stays allocated). */
int qe_env_table_solve(qe_env* env, double gamma, double tol, int32_t max_sweeps, double* q_out /* S*A or NULL */,
                       double* v_out /* S or NULL */, int32_t* sweeps_out, double* residual_out);
int qe_population_policy_values(qe_engine* e, qe_env* env, const double* gammas /* runs; NULL = the runs' own */, double tol,
                                int32_t max_sweeps, double* v_out /* runs*S */, int32_t* sweeps_out, double* residual_out,
                                uint32_t* status_out /* each runs, may be NULL */);

/* ---- diagnostics -----------------------------------------------------------------------------------
 * Occupies `blocks` CUs (one workgroup each, most of a CU's LDS) for `microseconds` (at most 200 000) on a stream of its
 * own and returns at once: tests take part of the chip away with it while a rollout runs, the situation of a collective
 * running beside the next chunk of a replica (nothing in the reference to stand in for). */
int qe_debug_occupy_cus(qe_engine* e, int32_t blocks, int32_t microseconds);
/* The turnstile path tags its per-row records with a step count that runs through the engine's life (32 bits of it
 * in the records; a call never starts on, reaches or crosses a multiple of 2^32 -- it is moved to the next multiple
 * plus 1 and the records are cleared).  qe_debug_set_turn_epoch places that count (the records are cleared before the
 * next turnstile call), qe_debug_turn_epoch reads the tag the next call would start from before any move: tests reach
 * the 2^31 / 2^32 edges with them, which otherwise take some 30 hours of turnstile steps. */
int qe_debug_set_turn_epoch(qe_engine* e, uint64_t value);
uint64_t qe_debug_turn_epoch(qe_engine* e);

/* ---- experience replay (algorithms/buffers/experience_replay.py:13-120; WIP and unused upstream) --
 * Ring buffer of (state, action, reward, next_state, done) in HBM.  Index SELECTION stays with the
 * caller (the reference draws `rng.choice(len, batch, replace=False)` from a NumPy Generator, :103-105;
 * the Python mirror does exactly that), the library stores, gathers and learns.
 *   qe_replay_create  <- ExperienceReplay.__init__ :56-66       qe_replay_push   <- push :68-86 (n in order)
 *   qe_replay_len     <- __len__ :111-120                       qe_replay_gather <- the fancy indexing of sample :103-109
 *   qe_replay_learn   : gather + qe_learn without leaving the device (what a replay-driven trainer does next) */
typedef struct qe_replay qe_replay;
int qe_replay_create(qe_replay** out, int32_t device, int64_t capacity);
int qe_replay_destroy(qe_replay* rb);
int qe_replay_push(qe_replay* rb, const int64_t* states, const int64_t* actions, const double* rewards,
                   const int64_t* next_states, const uint8_t* done, int64_t n);
/* Wire the ring to the fused rollout: from now on every transition (s, a, r, s', done) of every agent and
 * vector step of qe_rollout / qe_rollout_begin / qe_rollout_fused on this engine is pushed device to device,
 * in (step, agent) order -- what a host loop calling push after every env.step would store (:68-86);
 * position / full advance accordingly -- once the rollout is enqueued: a call that is refused (e.g.
 * QE_ERR_UNSUPPORTED for a forced path that does not fit) leaves position, full and the entries as they were.
 * A rollout that pushes more than `capacity` entries stores only its last `capacity`: every slot is written
 * at most once per rollout, so a ring smaller than one vector step (capacity < num_agents) also ends with
 * whole entries, those of the latest pushes.  rb == NULL detaches. */
int qe_replay_attach(qe_engine* e, qe_replay* rb);
int64_t qe_replay_len(qe_replay* rb);
int64_t qe_replay_position(qe_replay* rb);
int32_t qe_replay_full(qe_replay* rb);
int qe_replay_gather(qe_replay* rb, const int64_t* indices, int64_t n, int64_t* states, int64_t* actions,
                     double* rewards, int64_t* next_states, uint8_t* done);
int qe_replay_learn(qe_replay* rb, qe_engine* e, const int64_t* indices, int64_t n, double lr, int32_t mode);

#ifdef __cplusplus
}
#endif
#endif /* QLEARN_ENGINE_H */
