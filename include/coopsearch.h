/*
 * include/coopsearch.h -- C ABI of libcoopsearch_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of WZN1ng/Cooperative-Search: the flight_easy / flight environment
 * reset + step + reward + obs/state emission, batched over B independent environments that live in HBM.
 * The reference has no FFI: its boundary is a duck-typed Python object.  Every
 * entry point below names the reference method it replaces (paths relative to the reference repo); the
 * Python mirror of that object protocol lives in cooperative-search_amd/env.py.  Two bindings sit on these symbols:
 * torch.ops.coopsearch.* (csrc/torch_ops.cpp, the default: tensor checks in C++, torch's current HIP stream) and
 * ctypes (_lib.py, the torch-free route; INTEGRATION.md shows both stubs).
 *
 * Conventions
 *   - plain C types only; every *_dev pointer is DEVICE memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()); `stream` is a hipStream_t passed as void* (NULL = the legacy default stream);
 *   - nothing allocates, synchronises or copies on the step path; all work is enqueued on `stream`;
 *   - return value: 0 = OK, negative = CS_E_*; cs_last_error() gives a thread-local message;
 *   - n_targets <= 16 and n_agents <= 8: every kernel layout (16 lanes per env with lane t owning target t; 8 lanes per env
 *     with lane t owning agent t and targets t, t + 8; one env per lane) is built on these bounds.  Which layout a call runs
 *     on is chosen by batch size: the dispatch table is in DESIGN.md section 4; all of them give the same results.
 *
 * Numerics contract: agent positions and yaw are fp64 and follow the reference's
 * float operations one for one (same order, no FMA contraction, correctly rounded sin/cos of the
 * accumulated yaw); the uniform draws are NumPy's MT19937 stream per env, consumed in the reference's
 * order; rewards, flags and counts are integers.  Emitted obs/state/reward tensors are fp32.
 */
#ifndef COOPSEARCH_H
#define COOPSEARCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_ABI_VERSION 7   /* 2: cs_layout.ahead_off (pre-twisted MT words), cs_mt_canonical; 3: cs_layout.job_off;
                              4: cs_source_hash, CS_KERNEL_OCT; 5: CS_KERNEL_ODE; 6: cs_epsilon (exploration schedule),
                              cs_epsilon_step, CS_KERNEL_LANEV; 7: CS_CHECK_ACTIONS, cs_has_legacy_kernels;
                              still 7: cs_gru_seq_forward, cs_gru_seq_backward, cs_learn_last_error were ADDED, then
                              cs_episode_returns, then cs_policy_pack_device, then cs_collect_flight, cs_compact_out and
                              cs_store_episodes_compact, then cs_snapshot_bytes, cs_snapshot and cs_restore, then cs_render_params and
                              cs_render_episodes, then cs_gae and cs_ppo_loss, then cs_coverage_params and cs_coverage_actions, then cs_sweep_params and cs_sweep_episodes, then
                              cs_motion_params and cs_move_targets, then cs_belief_params and cs_belief_actions,
                              then cs_plan_params and cs_plan_actions, then cs_forecast_params, cs_belief_forecast and cs_plan_forecast_actions,
                              then cs_label_params, cs_label_episodes and cs_bc_loss, then cs_grid_params, cs_grid_features and
                              cs_feature_episodes, then cs_local_params and cs_local_coverage_actions, then cs_local_belief_params and
                              cs_local_belief_actions, then cs_local_label_params, cs_local_grid_features and cs_local_feature_episodes,
                              then cs_local_plan_params and cs_local_plan_actions, then cs_local_belief_forecast and
                              cs_local_plan_forecast_actions
                              (no existing export or struct changed: a version-7 caller works unchanged) */
#define CS_MAX_AGENTS 8
#define CS_MAX_TARGETS 16
#define CS_MAX_MAP 64
#define CS_MT_PAD 32      /* words 0..31 of an env's MT19937 row are mirrored behind word 623 */
#define CS_MT_STRIDE 672  /* uint32 words per env row: 624 state + 32 mirror + 16 unused (21 x 128 bytes) */
#define CS_TAPE_STRIDE 16 /* uint32 words per env of the lane kernel's hit tape (cs_layout.tape_off) */
#define CS_JOB_BYTES 256  /* bytes per env and record of the flight map-update job records (cs_layout.job_off) */

enum { CS_OK = 0, CS_E_CONFIG = -1, CS_E_ARG = -2, CS_E_LAUNCH = -3 };

/* action selection of cs_policy_forward / cs_rollout_policy */
enum {
    CS_SELECT_SOFTMAX = 1, /* agent/agent.py:77-97 (_choose_action_from_softmax, alg == 'reinforce'):
                              prob = (1 - epsilon) * softmax(q) + epsilon / n_actions; default (0) is :68-75, argmax with
                              epsilon-greedy exploration */
    CS_SELECT_SAMPLE = 2   /* with CS_SELECT_SOFTMAX: draw from Categorical(prob); without it argmax(prob) -- the
                              reference samples unless (epsilon == 0 and evaluate) */
};

/* cs_step / cs_rollout flags */
enum {
    CS_FREEZE_DONE = 1,  /* an env that was terminated on entry is left untouched: reward 0, terminated 1.
                            (The reference has no terminal guard, flight_env_easy.py:303-314; leave this
                            flag clear to reproduce that, as the B = 1 adapter does.) */
    CS_AUTO_RESET = 2,   /* an env that was terminated on entry is reset(init=False) first, then stepped */
    CS_ACTIONS_I64 = 4,  /* actions_dev holds int64 (torch.long) instead of int32 */
    CS_KERNEL_GROUP = 8, /* flight_easy: force the 16-lanes-per-env kernels (the default of cs_step up to the lane kernels' range) */
    CS_KERNEL_LANE = 16, /* flight_easy: force the first-generation lane-per-env kernel (the default for teams of 6 to 8 at very
                            large batches; smaller teams get CS_KERNEL_LANEV's kernel); same results */
    CS_KERNEL_SOLO = 32, /* (rounds 1-2: the 16-lanes-per-env ROLLOUT kernels, one wavefront or a kinematics / detection pair per four
                            envs.  Removed in round 6 -- no dispatch row had selected them since round 3: cs_rollout answers this flag
                            and the next with CS_E_CONFIG; the values stay reserved) */
    CS_KERNEL_DUO = 64,
    CS_KERNEL_OCT = 128, /* cs_rollout, flight_easy: force the 8-lanes-per-env kernel (lane t owns agent t and targets t, t + 8;
                            nothing replicated but the header: four and more wavefronts per SIMD -- the default between
                            the pair kernel's range and the lane kernel's); same results */
    CS_KERNEL_OD = 256,  /* cs_rollout, flight_easy: force the octet PAIR kernel (the 8-lane layout with a kinematics wavefront
                            running steps ahead of a detection wavefront, per 8 envs); same results */
    CS_KERNEL_ODE = 512, /* ... with a third wavefront per 8 envs that writes the outputs (default up to 8192 envs when obs
                            and state are both requested); same results */
    CS_KERNEL_LANEV = 1024, /* flight_easy, teams of up to 5: force the second-generation lane-per-env kernel (targets in
                            registers, half-wavefront staging of the get_state rows: three to four wavefronts per SIMD instead of
                            two; CS_KERNEL_LANE forces the first generation); same results */
    CS_CHECK_ACTIONS = 2048 /* debug aid: validate every action of the call on the device BEFORE anything is stepped.  A value
                            outside 0..2 makes the call return CS_E_ARG with the reference's IndexError wording ("list index out
                            of range": dyaw[act], flight_env_easy.py:259-262) and leaves the env state untouched.  Without the
                            flag the kernels treat any value other than 1 / 2 as 0 (no bounds check in the hot loops).  Python's
                            negative indices (dyaw[-1]) are NOT accepted by the batched path; the B = 1 adapter maps them like the
                            reference.  Synchronises the stream: a call made while the stream is being captured (or while the
                            capture state cannot be queried) is NOT checked, silently.  A library built with
                            -DCS_CHECK_ACTIONS_ALWAYS checks every call; the torch op layer sets the flag for batches of up to
                            64 envs (COOPSEARCH_CHECK_ACTIONS=0 / 1 turns that off / on for every batch). */
};

/* Exploration schedule of RolloutWorker.generate_episode -- common/rollout.py:35-41 (episode / epoch scale: one anneal before
 * the episode: the caller's), :75-76 (STEP scale, the QMIX and DOP default, common/arguments.py:78-82, 137-141: after every
 * executed env step `epsilon = epsilon - anneal_epsilon if epsilon > min_epsilon else epsilon`), :133-135 (the value persists
 * across episodes).  The reference has ONE worker and one scalar; a batch of B envs is B independent workers, each with its own
 * epsilon annealed by its own executed steps (a frozen, finished env does not anneal -- its episode loop has ended).
 *   eps_dev == NULL: every env uses `epsilon` for the whole call (no schedule).
 *   eps_dev != NULL: double [B], env b's epsilon: read when the call starts, annealed on the device after every step env b
 *                    executes (if per_step), written back when the call ends.
 * All arithmetic is the reference's: IEEE doubles, one subtraction per executed step. */
typedef struct cs_epsilon {
    double epsilon;       /* value of every env when eps_dev is NULL */
    double anneal;        /* args.anneal_epsilon */
    double min_epsilon;   /* args.min_epsilon */
    int32_t per_step;     /* != 0: args.epsilon_anneal_scale == 'step' */
    int32_t reserved;
    double *eps_dev;      /* NULL or double [B], in / out */
    double *trace_dev;    /* NULL or double [T][B], out: the epsilon env b's action selection of step t used */
} cs_epsilon;

/* Environment constants: common/arguments.py:27-34 (map_size, target_num, target_mode, agent_mode, n_agents,
 * view_range) and :233-284 (get_flight_args / get_flight_easy_args), plus the parsed target file
 * (main.py:19-32 load_targets; units of map_size/10). */
typedef struct cs_config {
    int32_t variant;      /* 0 = flight_easy (env/flight_env_easy.py), 1 = flight (env/flight_env.py) */
    int32_t n_agents;     /* 1..CS_MAX_AGENTS */
    int32_t n_targets;    /* 1..CS_MAX_TARGETS (reference: 15) */
    int32_t map_size;     /* reference: 50 */
    int32_t view_range;   /* reference: 7 */
    int32_t time_limit;   /* reference: 200 */
    int32_t agent_mode;   /* 0..3, flight_env_easy.py:139-180 */
    int32_t target_mode;  /* 0 = target file + gaussian jitter, 1 = uniform; flight_env_easy.py:95-136 */
    double velocity;      /* args.agent_velocity = 1 */
    double safe_dist;     /* 1 */
    double detect_prob;   /* 0.9 */
    double force_dist;    /* 3 */
    double force_factor;  /* POTENTIAL_FORCE_FACTOR = 0.8, flight_env_easy.py:65 */
    double cx[CS_MAX_TARGETS], cy[CS_MAX_TARGETS], dx[CS_MAX_TARGETS], dy[CS_MAX_TARGETS];
    int32_t deter[CS_MAX_TARGETS]; /* 1 = 't' fixed, 0 = 'f' jittered */
    int64_t batch;        /* B: environments resident on this device */
} cs_config;

/* Byte offsets of the per-env arrays inside the caller-allocated state blob (all 256-byte aligned). */
typedef struct cs_layout {
    size_t total_bytes;
    size_t tgt_off;    /* double [B][16][2]   target (x, y)                                             */
    size_t agent_off;  /* double [B][8][4]    agent (x, y, yaw, spare)                                   */
    size_t hdr_off;    /* int32  [B][16]      CS_H_* words below                                         */
    size_t mt_off;     /* uint32 [B][CS_MT_STRIDE] MT19937 state, circular (incremental) form + cursor in hdr;
                          words 624..655 mirror words 0..31                                          */
    size_t ahead_off;  /* int32  [B]          number of words at the cursor that are ALREADY twisted (their outputs
                          are temper(word)): the lane-per-env kernel regenerates the state 192 words at a time,
                          coalesced, ahead of consumption; 0 = the plain circular form.  0 <= ahead <= 624   */
    size_t tape_off;   /* uint32 [B][CS_TAPE_STRIDE] hit tape of the twisted words: bit r of words 0..9 = "the draw made of
                          stream words 2r, 2r+1 counted from the stream position `base` satisfies rand() <= detect_prob";
                          words 10, 11 = base (value of CS_H_WORDS_LO/HI when written), 12, 13 = the integer threshold
                          it was built for.  Derived data: written by cs_mt_advance / the lane kernel, ignored (and
                          rebuilt) whenever it does not match the cursor                                        */
    size_t prob_off;   /* float  [B][map*map] probability map, first index = x cell (flight only)        */
    size_t job_off;    /* uint8  [2][B][CS_JOB_BYTES] flight only: what the map sweep needs of the step that ran before
                          it (pending-pass flags, newly found masks, target cells, agent positions), double buffered so
                          that cs_rollout can sweep step t's map while step t + 1 runs.  Derived data: rewritten by
                          every cs_reset / cs_step / cs_rollout before it is read                              */
} cs_layout;

/* words of the per-env header */
enum {
    CS_H_FOUND = 0,     /* bit j = target j found                       (Target.find, flight_env_easy.py:12) */
    CS_H_NEWLY = 1,     /* targets found by the last detection pass     (tgt_found, flight_env.py:238)       */
    CS_H_TARGET_FIND = 2, /* env.target_find                             (flight_env_easy.py:42)              */
    CS_H_FLAGS = 3,     /* bit0 win_flag, bit1 map update pending, bit2 reset-time map update pending,
                           bits 8..15 out_flag[i]                                                            */
    CS_H_TIME_STEP = 4, /* env.time_step                                                                      */
    CS_H_TOTAL_REWARD = 5, /* env.total_reward (integer)                                                      */
    CS_H_MT_POS = 6,    /* cursor into the circular MT19937 state, 0..623, always even                        */
    CS_H_EPISODES = 7,  /* resets performed                                                                  */
    CS_H_WORDS_LO = 8,  /* 32-bit MT outputs consumed since cs_seed (u64, lo/hi)                             */
    CS_H_WORDS_HI = 9,
    CS_H_CURR_REWARD = 10, /* env.curr_reward of the last detection pass                                     */
    CS_H_NEWLY_RESET = 11, /* flight: targets found by the reset-time pass of a fused auto-reset              */
    CS_H_WORDS = 16
};

int cs_abi_version(void);
/* Hash of the sources this library was compiled from (cooperative-search_amd/build.py:source_hash; "" for a build that
 * did not pass it): how the loader tells a library built from other sources, instead of comparing file mtimes. */
const char *cs_source_hash(void);
/* 0 (since round 6: the 16-lanes-per-env ROLLOUT kernels of rounds 1-2 are gone; CS_KERNEL_SOLO / CS_KERNEL_DUO make cs_rollout
 * return CS_E_CONFIG, a CS_KERNEL_GROUP rollout is T launches of the 16-lane step kernel).  Kept for ABI 7 callers. */
int cs_has_legacy_kernels(void);
const char *cs_last_error(void);

/* Fills `out` with the state-blob layout for cfg (cfg->batch envs).  Host only. */
int cs_state_layout(const cs_config *cfg, cs_layout *out);

/* Zeroes the blob and sets every probability map to 0.5 (FlightSearchEnv.__init__, flight_env.py:53). */
int cs_init(const cs_config *cfg, void *state_dev, void *stream);

/* np.random.seed(seeds[b]) for env b's private stream (the reference shares one global stream between a
 * single env and everything else, and never seeds it: SURVEY.md Appendix C Q1). */
int cs_seed(const cs_config *cfg, void *state_dev, const uint32_t *seeds_dev, void *stream);

/* env.reset(init) -- flight_env_easy.py:79-182, flight_env.py:83-191 -- for every env with mask[b] != 0
 * (mask_dev NULL = all).  Ends with the reference's reset-time detection pass (and map update for flight).
 * obs_dev / state_dev_out (either may be NULL) receive get_obs() / get_state() of ALL envs afterwards:
 *   obs   float [B][n][4]            flight_easy   (get_obs, flight_env_easy.py:218-221)
 *         float [B][n][map*map + 4]  flight        (get_obs, flight_env.py:223-230: map first, 4 features last)
 *   state float [B][4n + 3m]                       (get_state, flight_env_easy.py:190-216) */
int cs_reset(const cs_config *cfg, void *state_dev, const uint8_t *mask_dev, int init,
             float *obs_dev, float *state_out_dev, void *stream);

/* env.step(act_list) -- flight_env_easy.py:303-314 (_agent_step :255-291, _potential_energy_force :293-301,
 * _update_obs :223-253), flight_env.py:357-368 (+ _update_prob_map :275-303) -- for every env.
 *   actions_dev    int32 or int64 [B][n], values 0/1/2 (validated only with CS_CHECK_ACTIONS)
 *   reward_dev     float [B]   (integer valued)     terminated_dev / win_dev  uint8 [B]
 *   obs_dev / state_out_dev as in cs_reset (may be NULL) */
int cs_step(const cs_config *cfg, void *state_dev, const void *actions_dev, int flags,
            float *reward_dev, uint8_t *terminated_dev, uint8_t *win_dev,
            float *obs_dev, float *state_out_dev, void *stream);

/* T consecutive env.step calls from ONE call: actions [T][B][n]; reward [T][B]; terminated/win [T][B];
 * obs [T][B][n][obs width]; state_out [T][B][4n+3m] (obs/state_out may be NULL).  Same results as T cs_step calls
 * with the same flags.  flight_easy: one launch with the env resident in registers; flight: one launch per step in
 * which the map sweep of step t (update + the map part of get_obs) runs beside the kinematics / detection of step
 * t + 1 -- the two are independent once the sweep reads the step's job record (cs_layout.job_off).
 * flight_easy: obs_dev must be 16-byte aligned (CS_E_ARG otherwise): an (env, agent) observation is one 16-byte store;
 * state_out_dev may be anywhere (a table that is not 16-byte aligned, or whose rows per step are not, takes scalar stores). */
int cs_rollout(const cs_config *cfg, void *state_dev, const void *actions_dev, int T, int flags,
               float *reward_dev, uint8_t *terminated_dev, uint8_t *win_dev,
               float *obs_dev, float *state_out_dev, void *stream);

/* MT19937 pre-pass: for every env with fewer than `min_ahead` twisted words ahead of its cursor, twist the whole row
 * ahead (ahead -> 624) in one coalesced sweep.  Does not change any stream: only WHEN its words are regenerated.
 * cs_rollout's lane-per-env path runs it before every 64-step chunk for teams of 6 and more (smaller teams refresh
 * their rows inside the kernels).  Callers that drive cs_step should call it every ~32 steps with min_ahead ~400
 * (BatchedFlightEnv.step does): a single step reads its draws from the env's hit tape while that is valid, which keeps
 * the MT19937 window -- a load that depends on the header's cursor -- off the critical path of the launch (7.3 instead
 * of 7.8 us per step at 4096 envs); a row that runs out simply falls back to twisting on demand. */
int cs_mt_advance(const cs_config *cfg, void *state_dev, int min_ahead, void *stream);

/* Writes every env's MT19937 row in CANONICAL form -- all 624 words twisted ahead of the cursor -- to
 * rows_out_dev (uint32 [B][CS_MT_STRIDE]) without changing the state.  Two states that describe the same position of the same
 * stream have equal canonical rows (and equal CS_H_MT_POS), however much of the row each kernel had pre-twisted. */
int cs_mt_canonical(const cs_config *cfg, void *state_dev, uint32_t *rows_out_dev, void *stream);

/* get_obs() + get_state() of every env without stepping. */
int cs_emit(const cs_config *cfg, void *state_dev, float *obs_dev, float *state_out_dev, void *stream);

/* ---- env snapshot / restore -------------------------------------------------------------------------------------
 * An env's LOGICAL state as one fixed-size record, and back.  The state blob itself is not such a thing: its MT19937 row is
 * stored in a form that depends on which kernel ran last (cs_layout.ahead_off), words 624..655 mirror words 0..31, the hit
 * tape (cs_layout.tape_off) is accepted by threshold and word count alone, and CS_H_FLAGS bits 1-2 and the job records are
 * leftovers of the last launch.  Copying one env's arrays over another's is therefore wrong; these two calls are the way.
 * Two envs in the same logical state give byte-equal records, whichever kernels brought them there.
 *
 * Record (cs_snapshot_bytes(cfg) bytes, a multiple of 16; CS_SNAPSHOT_VERSION 1):
 *      0  uint32 [16]     0x50534343, format version, variant, n_agents, n_targets, map_size, 0 ...
 *     64  uint32 [16]     the env's CS_H_* words with CS_H_FLAGS bits 1-2 clear (words 12..15 zero)
 *    128  double [16][2]  targets (x, y); rows >= n_targets zero
 *    384  double [8][4]   agents (x, y, yaw, 0); rows >= n_agents zero
 *    640  uint32 [624]    the MT19937 row in cs_mt_canonical's form; its cursor is CS_H_MT_POS above
 *   3136  float [map_size^2]  flight only: the probability map
 * so cs_snapshot_bytes = 3136 for flight_easy and 3136 + 4 map_size^2 for flight.  A record is per env: it can go to an env
 * of any batch size or shard whose variant, n_agents, n_targets and map_size are the record's.  Everything else lives in
 * cs_config, not in the record, and belongs to the RESTORING env: time_limit, detect_prob, view_range, velocity, safe_dist,
 * the force constants, agent_mode, target_mode and the target file.
 *
 * Both calls enqueue on `stream` and never synchronise; records_dev must be 16-byte aligned (CS_E_ARG otherwise). */
#define CS_SNAPSHOT_VERSION 1
/* Host only; 0 for a config that cs_state_layout refuses. */
size_t cs_snapshot_bytes(const cs_config *cfg);
/* Record i (at records_dev + i * cs_snapshot_bytes) = env env_idx_dev[i] (int64 [count]; NULL: env i, count <= batch).  The
 * state is only read.  An index outside 0..batch-1 gives an all-zero record, which cs_restore refuses. */
int cs_snapshot(const cs_config *cfg, const void *state_dev, const int64_t *env_idx_dev, int64_t count, void *records_dev,
                void *stream);
/* Env dst_idx_dev[i] takes record src_idx_dev[i] of the n_records at records_dev, for i < count (int64 [count] each; NULL: i).
 * src may repeat (one state forked into many envs); the dst entries must be distinct, as cs_store_episodes' slots.  A
 * restored env holds the record's header words, targets, agents and map, its row in canonical form with the mirror words
 * rebuilt and ahead = 624, a hit tape rebuilt from THAT row (no tape of the env's previous stream survives), and nothing
 * pending for the map sweep.  Envs not named in dst are untouched, bit for bit.  An entry whose record header does not match
 * cfg (its 16 identification words; also a cursor word that is not an even value below 624, or a nonzero header word 12..15),
 * or whose src / dst index is out of range, leaves its env untouched -- that is all a record is checked for: the remaining
 * CS_H_* words, targets, agents, row and map ARE the state and are taken as they are, so records come from cs_snapshot.
 * status_dev (int32 [4], may be NULL) names the FIRST refused entry: {1, kind, i, value} with kind 1 = src out of range, 2 = dst out of range (value: the index), 3 = record refused (value: the first offending uint32 word of the
 * record); {0, -1, -1, 0} when every entry was applied.  obs_dev / state_out_dev as in cs_reset: get_obs() / get_state() of
 * ALL envs afterwards, either may be NULL. */
int cs_restore(const cs_config *cfg, void *state_dev, const void *records_dev, int64_t n_records, const int64_t *src_idx_dev,
               const int64_t *dst_idx_dev, int64_t count, int32_t *status_dev, float *obs_dev, float *state_out_dev, void *stream);

/* Per-device partial sums of the evaluation metrics of runner.py:86-96 / rollout.py:190-198:
 * out4_dev[0] += sum total_reward, [1] += sum win_flag, [2] += sum target_find, [3] += number of envs.
 * (double[4]; the caller zeroes it, then all-gathers / all-reduces the partials over RCCL.) */
int cs_metrics(const cs_config *cfg, void *state_dev, double *out4_dev, void *stream);

/* ---- caller-side row f3: fused forward of the shared recurrent agent network ------------
 * Replaces the per-agent batch-1 loop of agent/agent.py:33-75 (choose_action) over network/base_net.py:5-46
 * ([conv ->] fc1 -> ReLU -> GRUCell(64) -> fc2[Linear, ReLU, Linear]): ONE launch for all rows = B * n_agents, fp32 on
 * the matrix cores, epsilon-greedy choice on the device; for flight, one more launch for the conv front end. */

/* floats in a packed weight blob */
size_t cs_policy_packed_floats(void);

/* HOST: torch-layout weights (fc1.weight [64][in_dim], rnn.weight_ih / weight_hh [192][64], fc2.0.weight [64][64],
 * fc2.2.weight [n_actions][64] and their biases) -> packed_host[cs_policy_packed_floats()], to be copied to the device.
 * in_dim = [16 conv features +] 4 + n_actions + n_agents <= 32 (agent.py:41-52, base_net.py:31-39).
 * The network runs on the 16-bit matrix pipe with every fp32 operand split into two halves (csrc/policy_dev.h): a WEIGHT whose
 * magnitude exceeds 65504 (or is not finite) is refused with CS_E_ARG; an ACTIVATION (a ReLU output of fc1 / fc2) beyond 65504
 * SATURATES there (min(relu(.), 65504): one v_med3_f32 per conversion, values inside the range unchanged bit for bit) -- with
 * |obs| <= 1 and |h| < 1 no activation gets that far while the rows of fc1 / fc2.0 have an L1 norm below ~6e4, as any trained
 * network's do; the q-values stay finite either way (tests/test_gpu_policy.py). */
int cs_policy_pack(const float *fc1_w, const float *fc1_b, const float *w_ih, const float *b_ih, const float *w_hh,
                   const float *b_hh, const float *fc2a_w, const float *fc2a_b, const float *fc2b_w, const float *fc2b_b,
                   int in_dim, int n_actions, float *packed_host);

/* DEVICE: cs_policy_pack in ONE launch on `stream`, every pointer a device pointer (the learner's parameters where they live;
 * packed_dev [cs_policy_packed_floats()]).  For every weight that cs_policy_pack accepts, the blob is cs_policy_pack's output word
 * for word (the same split_f16 conversions, zero padding and fp32 biases; every word is written).  cs_policy_pack's refusal is
 * kept, all or nothing, without a host synchronisation: if any entry of the five weight matrices is not finite or exceeds 65504
 * in magnitude, packed_dev is left exactly as it was and status_dev (int32 [4]) receives {1, tensor, index, value bits} -- tensor
 * in cs_policy_pack's check order (0 fc1.weight, 1 rnn.weight_ih, 2 rnn.weight_hh, 3 fc2.0.weight, 4 fc2.2.weight), the FIRST
 * offending flat index in that order and the float's bits; otherwise status_dev = {0, -1, -1, 0}.  Returns CS_E_ARG (null
 * pointer, in_dim outside 1..32, n_actions outside 1..16) before any launch, CS_E_LAUNCH if the launch fails. */
int cs_policy_pack_device(const float *fc1_w, const float *fc1_b, const float *w_ih, const float *b_ih, const float *w_hh,
                          const float *b_hh, const float *fc2a_w, const float *fc2a_b, const float *fc2b_w,
                          const float *fc2b_b, int in_dim, int n_actions, float *packed_dev, int32_t *status_dev,
                          void *stream);

/* One forward over rows = B*n (row r: env r / n_agents, agent r % n_agents).  obs row r = 4 floats at
 * obs_dev + r*obs_stride + obs_offset (floats); last_dev[r] = previous action or < 0 for none
 * (last_dev NULL = raw mode: the row at obs_dev + r*obs_stride + obs_offset already holds all 4 + n_actions +
 * n_agents non-conv inputs);
 * feat_dev (NULL for flight_easy): float [rows / rows_per_feat][16] conv features (cs_policy_conv_features) that go in
 * front of the obs columns; rows r*rows_per_feat .. +rows_per_feat-1 share feature row r (rows_per_feat = n_agents
 * when the features were computed once per env);
 * hidden_dev float [rows][64] updated in place; q_dev float [rows][n_actions] or NULL; actions_dev int64 [rows]:
 * select = 0: argmax_a q (first maximum), or with probability epsilon a uniform action; CS_SELECT_SOFTMAX: the softmax
 * rule of agent.py:77-97.  Random choices come from a counter-based generator keyed by (seed, step, row0 + row): row0 =
 * global index of this call's row 0 (env_offset * n_agents for a sharded batch), so the noise does not depend on the
 * sharding.
 * avail_actions (agent/agent.py:70, :87 mask q / prob with the env's get_avail_agent_actions) is not an input: both envs
 * of this path return all ones for every agent (flight_env_easy.py:184-188, flight_env.py:193-197), so the mask is the
 * identity; a caller with a real mask applies it to q_dev and selects on its side. */
int cs_policy_forward(const float *packed_dev, const float *obs_dev, int obs_stride, int obs_offset,
                      const int64_t *last_dev, const float *feat_dev, int rows_per_feat, float *hidden_dev, float *q_dev,
                      int64_t *actions_dev, int rows, int n_agents, int n_actions, float epsilon, const double *eps_env_dev,
                      uint64_t seed, uint32_t step, uint64_t row0, int select, void *stream);
/* (eps_env_dev: NULL, or double [rows / n_agents]: row r explores with epsilon eps_env_dev[r / n_agents] instead of `epsilon` --
 * the per-env schedule of cs_epsilon for callers that drive the loop step by step; cs_epsilon_step anneals it.) */

/* One step of the exploration schedule for a caller that drives the loop itself (cs_policy_forward -> cs_epsilon_step ->
 * cs_step): for every env that the NEXT cs_step(flags) will execute (not: terminated on entry and frozen),
 * eps_dev[b] = eps_dev[b] - anneal if eps_dev[b] > min_epsilon else eps_dev[b] (common/rollout.py:75-76); trace_row_dev (NULL or
 * double [B]) receives the values BEFORE the anneal, i.e. what the action selection of this step used. */
int cs_epsilon_step(const cs_config *cfg, void *state_dev, int flags, double *eps_dev, double anneal, double min_epsilon,
                    double *trace_row_dev, void *stream);

/* flight: the conv front end of base_net.py:9-18,31-36 with the reference's hyper-parameters (common/arguments.py:256-265:
 * Conv2d(1,4,k=4,s=2) -> ReLU -> Conv2d(4,1,k=3,s=1,p=1) -> ReLU -> Linear(576,16)) on n_maps 50x50 probability maps;
 * map m = 2500 floats at maps_dev + m*map_stride.  The weight pointers are the torch tensors as they are (device).
 * All agents of an env observe the same map (flight_env.py:223-230): run it once per env on the env's first obs row
 * (map_stride = n_agents * 2504) and pass rows_per_feat = n_agents to cs_policy_forward. */
int cs_policy_conv_features(const float *conv1_w_dev, const float *conv1_b_dev, const float *conv2_w_dev,
                            const float *conv2_b_dev, const float *lin_w_dev, const float *lin_b_dev,
                            const float *maps_dev, int64_t map_stride, int n_maps, float *feat_dev, void *stream);
/* The backward pass of cs_policy_conv_features for the learners: dfeat_dev [n_maps][16] = dloss/dfeat of every map -> the
 * six weight gradients in the weights' own layouts (64, 4, 36, 1, 16*576 and 16 floats), summed over all maps and WRITTEN
 * (not accumulated).  No gradient with respect to the maps.  Nothing is kept from the forward: both activation planes are
 * recomputed on chip with the forward's own arithmetic, so the ReLU gates are exactly the ones the forward applied.  A map
 * whose 16 dfeat values are all zero is skipped.  No float atomics: every workgroup writes one partial gradient set to
 * scratch_dev and a second launch adds the sets in a fixed order, so reruns are bit-identical.  scratch_dev holds at least
 * the number of floats that cs_policy_conv_features_backward_scratch(n_maps, &floats) reports (a function of the device and
 * n_maps only); its contents need not be initialised and mean nothing afterwards. */
int cs_policy_conv_features_backward_scratch(int n_maps, int64_t *floats_out);
int cs_policy_conv_features_backward(const float *conv1_w_dev, const float *conv1_b_dev, const float *conv2_w_dev,
                                     const float *conv2_b_dev, const float *lin_w_dev, const float *lin_b_dev,
                                     const float *maps_dev, int64_t map_stride, int n_maps, const float *dfeat_dev,
                                     float *d_conv1_w_dev, float *d_conv1_b_dev, float *d_conv2_w_dev, float *d_conv2_b_dev,
                                     float *d_lin_w_dev, float *d_lin_b_dev, float *scratch_dev, int64_t scratch_floats,
                                     void *stream);
const char *cs_policy_last_error(void);

/* Fused closed loop (flight_easy, n_agents <= 5): T x (cs_policy_forward -> cs_step) in ONE launch, i.e. the body of
 * RolloutWorker.generate_episode's loop (common/rollout.py:43-76) for all B envs with the hidden state, the chosen
 * actions and the envs resident on chip between steps.  Same results, bit for bit, as T pairs of
 * cs_policy_forward(..., step = step0 + s) and cs_step(flags) calls.
 *   packed_dev   cs_policy_pack output            hidden_dev  float [B*n][64], in/out
 *   last_dev     int64 [B][n] action before the first step (< 0 = none)
 *   actions_dev  int64 [T][B][n] chosen actions (out); the other outputs as in cs_rollout.
 * Same results, bit for bit, as T triples cs_policy_forward(step0 + s, eps_env_dev) -> cs_epsilon_step -> cs_step. */
int cs_rollout_policy(const cs_config *cfg, void *state_dev, const float *packed_dev, float *hidden_dev,
                      const int64_t *last_dev, int T, int flags, const cs_epsilon *eps, uint64_t seed, uint32_t step0,
                      uint64_t row0, int select, int64_t *actions_dev, float *reward_dev, uint8_t *terminated_dev,
                      uint8_t *win_dev, float *obs_dev, float *state_out_dev, void *stream);
/* (eps: the exploration schedule, see cs_epsilon; with eps->eps_dev the per-step anneal of rollout.py:75-76 runs INSIDE the
 * launch, env by env, and the carried values come back in eps_dev.) */

/* Closed loop for flight (the loop body of common/rollout.py:43-76 with the conv network of network/base_net.py:9-36):
 * T x (cs_policy_conv_features -> cs_policy_forward -> cs_step) enqueued by ONE call.  Bit for bit the results of the T
 * triples of calls; what changes is the data movement: the conv front end reads every env's probability map where it
 * lives in the state blob (one 10 KB read per env instead of a pass over the n observation copies), and with
 * obs_dev == NULL the n copies of the map that get_obs emits (flight_env.py:223-230) are never written -- the network
 * is their only consumer inside the loop.  The map update still runs every step.
 *   conv1_w_dev .. lin_b_dev   the six tensors of cs_policy_conv_features
 *   scratch_dev                float [B][16 + 4 n_agents] (conv features; the agents' own 4 observation floats)
 *   last_dev                   int64 [B][n] action before the first step (< 0 = none)
 *   actions_dev                int64 [T][B][n] chosen actions (out); obs_dev / state_out_dev NULL or as in cs_rollout */
int cs_rollout_policy_flight(const cs_config *cfg, void *state_dev, const float *packed_dev, const float *conv1_w_dev,
                             const float *conv1_b_dev, const float *conv2_w_dev, const float *conv2_b_dev,
                             const float *lin_w_dev, const float *lin_b_dev, float *hidden_dev, const int64_t *last_dev,
                             float *scratch_dev, int T, int flags, const cs_epsilon *eps, uint64_t seed, uint32_t step0, uint64_t row0,
                             int select, int64_t *actions_dev, float *reward_dev, uint8_t *terminated_dev, uint8_t *win_dev,
                             float *obs_dev, float *state_out_dev, void *stream);

/* cs_rollout_policy_flight with obs_dev == NULL that ALSO records what an episode batch needs, each map once (map-once
 * episode storage): all agents of an env observe the same map, and step t's o_next is step t + 1's o.
 *   map_tab_dev    float [T+1][B][map*map]  row 0: every env's probability map on entry; row t + 1: after step t (written
 *                  by the step's map sweep beside its update, one 16-byte-wide copy per env; 16-byte aligned)
 *   state_tab_dev  float [T+1][B][4n+3m]    row 0: get_state() on entry; row t + 1: after step t
 * Both tables are written for EVERY env and row, a frozen, finished env included (its rows repeat).  The agents' own 4
 * observation floats are not recorded: they are state[4i..4i+3] of the same instant (one float4 written to both places).
 * Actions, rewards, flags, hidden state and the carried epsilon are cs_rollout_policy_flight's, bit for bit. */
int cs_collect_flight(const cs_config *cfg, void *state_dev, const float *packed_dev, const float *conv1_w_dev,
                      const float *conv1_b_dev, const float *conv2_w_dev, const float *conv2_b_dev, const float *lin_w_dev,
                      const float *lin_b_dev, float *hidden_dev, const int64_t *last_dev, float *scratch_dev, int T, int flags,
                      const cs_epsilon *eps, uint64_t seed, uint32_t step0, uint64_t row0, int select, int64_t *actions_dev,
                      float *reward_dev, uint8_t *terminated_dev, uint8_t *win_dev, float *map_tab_dev, float *state_tab_dev,
                      void *stream);

/* ---- caller-side rows f1 / f2: episode batch assembly ------------------------------------------------------------
 * common/rollout.py:66-76,105-132 (the eleven per-episode arrays and their padding: steps after termination are zero
 * rows with padded = 1, terminated = 1) and common/replay_buffer.py:41-61 (store_episode) in one pass over the
 * collector's step-major tables.  All destinations are float32 [slots][T][...] arrays (a fresh [B][T][...] batch, or
 * the ring of a replay buffer); env b's episode goes to slot slot_dev[b] (NULL: slot b).
 *   o_tab [T+1][B][n][obs_w]   s_tab [T+1][B][state_w]   u_tab int64 [T][B][n]   r_tab [T][B]   term_tab u8 [T][B] */
typedef struct cs_episode_out {
    float *o, *u, *s, *r, *o_next, *s_next, *avail_u, *avail_u_next, *u_onehot, *padded, *terminated;
} cs_episode_out;

int cs_store_episodes(int B, int T, int n_agents, int n_actions, int obs_w, int state_w, const float *o_tab_dev,
                      const float *s_tab_dev, const int64_t *u_tab_dev, const float *r_tab_dev,
                      const uint8_t *term_tab_dev, const int64_t *slot_dev, const cs_episode_out *out, void *stream);
/* The same episodes in the map-once format (cs_collect_flight's tables -> a fresh batch or ring slots): float32
 *   map [slots][T+1][cells]   s_full [slots][T+1][state_w]   u [slots][T][n]   r / padded / terminated [slots][T]
 * With L the number of real (un-padded) steps of an episode, rows t <= L of map / s_full are the tables' rows and rows
 * t > L are zero; u, r, padded, terminated are cs_store_episodes' keys of the same names.  One pass over the wide keys,
 * 16-byte pieces where the rows' alignment allows.
 *   map_tab [T+1][B][cells]   s_tab [T+1][B][state_w]   u_tab int64 [T][B][n]   r_tab [T][B]   term_tab u8 [T][B] */
typedef struct cs_compact_out {
    float *map, *s_full, *u, *r, *padded, *terminated;
} cs_compact_out;

int cs_store_episodes_compact(int B, int T, int n_agents, int cells, int state_w, const float *map_tab_dev,
                              const float *s_tab_dev, const int64_t *u_tab_dev, const float *r_tab_dev,
                              const uint8_t *term_tab_dev, const int64_t *slot_dev, const cs_compact_out *out, void *stream);
const char *cs_episodes_last_error(void);

/* ---- episode frames: the state (and map) rows of E episodes -> RGB pictures -----------------
 * The reference's only picture is env.render(), a matplotlib scatter of one instant (flight_env_easy.py:324-343).  This
 * call draws EVERY row of E recorded episodes as a size x size RGB frame in one launch: the flight map as a heat layer,
 * every agent's sensor disc, the path it has flown so far, the targets (found ones in another colour), the agents as
 * triangles pointing along their heading, and a progress bar of found targets.  The frame is DEFINED by
 * render.render_episodes_torch (stock torch ops, integer geometry after one quantisation); the kernel reproduces it byte
 * for byte.
 *   states_dev  float [E][R][4n + 3m]  get_state() rows: agent i = (xn, yn, cos, sin) at 4i, target j = (xn, yn, found) at 4n + 3j
 *   maps_dev    float [E][R][side^2]   the flight map of every row, row-major [ix * side + iy]; NULL: no heat layer
 *   counts_dev  int32 [E]              real rows of episode e: frame t is drawn from row min(t, clamp(counts[e], 1, R) - 1);
 *                                      rows past the count are never read
 *   frames_dev  uint8 [E][R][size][size][3], 4-byte aligned; every byte is written (no clearing needed)
 * With U = 16 * size sub-units across the map, the radii below are in sub-units (render.RenderSpec computes them). */
enum {
    CS_RENDER_HEAT = 1, CS_RENDER_SENSOR = 2, CS_RENDER_TRAIL = 4, CS_RENDER_TARGETS = 8, CS_RENDER_AGENTS = 16, CS_RENDER_BAR = 32
};
typedef struct cs_render_params {
    int32_t n_agents;     /* 1..8 */
    int32_t n_targets;    /* 1..16 */
    int32_t state_width;  /* floats per state row: 4 n_agents + 3 n_targets */
    int32_t size;         /* W: frame width and height in pixels, a multiple of 4 in 16..1024 */
    int32_t side;         /* cells per map side, 1..CS_MAX_MAP (looked at only with maps_dev) */
    int32_t map_width;    /* floats per map row: side * side (looked at only with maps_dev) */
    int32_t rv;           /* sensor radius, 0..32767 */
    int32_t rt;           /* target disc radius, 0..32767 */
    int32_t rtr;          /* trail radius, 0..32767 */
    int32_t tri_len;      /* L: an agent's triangle reaches L ahead of its position, L / 2 behind, 0.6 L to each side; 0..16383 */
    int32_t layers;       /* CS_RENDER_* bits */
    int32_t reserved;     /* 0 */
    uint8_t background[4], sensor_tint[4], sensor_ring[4], target[4], target_found[4], bar_on[4], bar_off[4];   /* r, g, b, 0 */
    const uint8_t *palette_dev;   /* uint8 [8][3]: trail and triangle colour of agent i */
    const uint8_t *lut_dev;       /* uint8 [256][3]: heat colour of rint(clamp(p, 0, 1) * 255) */
} cs_render_params;

/* One launch on `stream`, no synchronisation.  CS_E_CONFIG (before any launch) for n_agents outside 1..8, n_targets outside
 * 1..16, state_width != 4n + 3m, size not a multiple of 4 or outside 16..1024, E < 1, R < 1, a radius out of range, a NULL
 * pointer (maps_dev alone may be NULL), frames_dev not 4-byte aligned, or, with maps_dev, side outside 1..CS_MAX_MAP or
 * map_width != side * side.  The message is cs_episodes_last_error()'s. */
int cs_render_episodes(const cs_render_params *p, const float *states_dev, const float *maps_dev, const int32_t *counts_dev,
                       int E, int R, uint8_t *frames_dev, void *stream);

/* ---- greedy coverage baseline: a sweep of a shared belief grid, one launch per decision ------
 * The reference has no hand-written policy to compare a learner with (policy/trandition.py is a stub with a Random subclass).
 * This one is the classical answer to cooperative search: every env keeps a belief grid G, int32 [side * side], row-major
 * [ix * side + iy], in Q16 -- 65536 = "nobody has looked here", the caller fills it with 65536 when an episode starts --; every
 * call lets G regrow towards 65536, multiplies the cells inside an agent's sensor disc by keep / 65536, and then lets the agents
 * choose in index order: each takes the action whose look-ahead disc holds the most belief that no earlier agent has claimed.
 * The policy is DEFINED by baseline.coverage_actions_torch (stock torch ops, integer arithmetic after one quantisation); the
 * kernel reproduces actions and grid element for element.  It reads only the first 4 n_agents floats of a get_state() row:
 * agent i = (xn, yn, cos, sin) at 4i; targets, found flags and flight's map are never looked at.
 *   state_dev    float [B][state_width]     grid_dev  int32 [B][side * side], in / out, values 0..65536 (a cell outside
 *                                           that range is read as the nearer bound, in the kernel and in the definition)
 *   actions_dev  int64 [B][n_agents], out: 0 straight, 1 = + pi / 18, 2 = - pi / 18 (the env's coding) */
typedef struct cs_coverage_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP (R = 16 view_range sub-units of 1/16 cell) */
    int32_t keep;         /* rint((1 - detect_prob) * 65536), 0..65536 */
    int32_t regrow;       /* every call: G += (65536 - G) >> regrow; 1..16 */
    int32_t lookahead;    /* distance of the look-ahead point in cells, 0..side */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_coverage_params;

/* One launch on `stream`, one workgroup per env, no atomics, no synchronisation.  CS_E_CONFIG (before any launch) for a field
 * out of range, a NULL or misaligned pointer or B < 1.  The message is cs_episodes_last_error()'s. */
int cs_coverage_actions(const cs_coverage_params *p, const float *state_dev, int B, int32_t *grid_dev, int64_t *actions_dev,
                        void *stream);

/* ---- coverage under a limited communication range: n private grids per env, one launch per decision ---
 * cs_coverage_actions decides from one grid per env: every agent knows at once what every team-mate has swept.  Here agent i keeps a
 * grid of its own and hears only the agents within comm_range cells of it.  Per call: every grid regrows; agent i sweeps its own disc
 * on its own grid (S_i); i and j are linked iff i == j, or comm_range < 0, or (X_i - X_j)^2 + (Y_i - Y_j)^2 < (16 comm_range)^2 in
 * sub-units (strict, 64-bit: comm_range 0 links nobody); M_i = min over the linked j of S_j, cell by cell, is written back -- ONE hop
 * per call: news travels along a chain of linked agents one hop per decision --; then the agents choose in index order as
 * cs_coverage_actions' do, agent i on M_i less the chosen footprints of the linked agents before it.  With comm_range -1 and equal
 * grids this IS cs_coverage_actions (every grid equals its grid); with comm_range 0 every agent is a one-agent cs_coverage_actions.
 * DEFINED by local.local_coverage_actions_torch (stock torch ops, integer after one quantisation); the kernel reproduces grids and
 * actions bit for bit.
 *   state_dev    float [B][state_width]     grids_dev  int32 [B][n_agents][side * side], in / out, values 0..65536 (a cell outside
 *                                           that range is read as the nearer bound)
 *   actions_dev  int64 [B][n_agents], out: 0 straight, 1 = + pi / 18, 2 = - pi / 18 (the env's coding) */
typedef struct cs_local_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t keep;         /* rint((1 - detect_prob) * 65536), 0..65536 */
    int32_t regrow;       /* every call: G += (65536 - G) >> regrow; 1..16 */
    int32_t lookahead;    /* distance of the look-ahead point in cells, 0..side */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t comm_range;   /* communication range in whole cells, 0..128, or -1: unlimited */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_local_params;

/* One launch on `stream`, one workgroup per env, no global atomics, no synchronisation.  CS_E_CONFIG (before any launch) for a field
 * out of range, a non-zero `reserved`, a NULL or misaligned pointer or B < 1.  The message is cs_episodes_last_error()'s. */
int cs_local_coverage_actions(const cs_local_params *p, const float *state_dev, int B, int32_t *grids_dev, int64_t *actions_dev,
                              void *stream);

/* ---- swept-area accounting of recorded episodes, one launch per episode batch ---------------
 * How much of the map a team's sensors have swept by row t of an episode, and how much of a row's sweeping lands on ground
 * already seen: the measure of HOW a policy searches, beside the found-fraction curve, and -- as its per-step increment -- a
 * count-based exploration bonus.  Rows are get_state() rows as render's tables hold them (row 0: the reset pose, row t + 1:
 * after step t); only the first 4 n_agents floats of a row are read: agent i = (xn, yn, cos, sin) at 4i.  Positions are
 * quantised as cs_coverage_actions quantises them and a cell is swept at a row when its centre lies within 16 view_range
 * sub-units of any agent (the sweep test of the coverage policy).  DEFINED by sweep.sweep_episodes_torch (stock torch ops,
 * integer after one quantisation); the kernel reproduces the three outputs element for element.
 *   states_dev  float [E][rows][state_width]     counts_dev  int32 [E]: row t of episode e is valid if t < clamp(counts[e], 0, rows);
 *                                                a row at or past the count is never read
 *   first_dev   int32 [E][side * side], out: the first valid row at which the cell (ix * side + iy) is swept, -1 if never
 *   new_dev     int32 [E][rows], out: the number of cells with first == t        (0 at and past the count)
 *   seen_dev    int32 [E][rows], out: the number of cells swept at row t         (0 at and past the count) */
typedef struct cs_sweep_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t rows;         /* rows per episode (T + 1), >= 1 */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_sweep_params;

/* One launch on `stream`, one workgroup per episode, no atomics, no synchronisation; every element of the three outputs is
 * written.  CS_E_CONFIG (before any launch) for a field out of range, a NULL or misaligned pointer or E < 1.  The message is
 * cs_episodes_last_error()'s. */
int cs_sweep_episodes(const cs_sweep_params *p, const float *states_dev, const int32_t *counts_dev, int E, int32_t *first_dev,
                      int32_t *new_dev, int32_t *seen_dev, void *stream);

/* ---- moving targets: one move of every unfound target of every live env, one launch ----------
 * The reference's targets never move: tgt is written by cs_reset and only read afterwards, so swept ground never goes stale.
 * This call is the opt-in scenario in which it does.  Target j < n_targets of env b moves when the env is live on entry --
 * the predicate by which cs_step with CS_FREEZE_DONE leaves an env alone: win bit of CS_H_FLAGS clear and CS_H_TIME_STEP <
 * time_limit -- and bit j of CS_H_FOUND is clear.  Every other double of tgt keeps its bits: found targets, slots >=
 * n_targets, every target of a finished env.  The call reads tgt, agent and hdr and writes tgt, nothing else; nothing else in
 * the blob is derived from an unfound target's position.  DEFINED by motion.move_targets_torch (stock torch ops, fp64, every
 * operation rounded once; no sqrt, no division, no transcendental); the kernel reproduces it bit for bit.
 *   heading  one of 16: CX[k], CY[k] = cos, sin(2 pi k / 16) as doubles (the literals of csrc/motion.h and motion.py)
 *   walk     k = key >> 28 with, in uint32 arithmetic,
 *              fmix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 *              key = seed; for w in (g & 0xffffffff, g >> 32, CS_H_EPISODES, CS_H_TIME_STEP / persist, j): key = fmix(key ^ w) + 0x9E3779B9
 *            g = env_offset + b, the global env index: a pure function of the env's own logical state and its global index --
 *            no state of its own, so snapshots and resume need nothing new, a sharded batch equals the whole batch, and one
 *            state forked into several env indices diffuses differently in each
 *   evade    d2_i = (x - ax_i)^2 + (y - ay_i)^2 over the agents i < n_agents; if some d2_i <= sense * sense, the nearest such
 *            agent (lowest i on ties) gives (dx, dy) = (x - ax, y - ay) and k is the lowest index that maximises
 *            dx CX[k] + dy CY[k]; otherwise k is the walk heading
 *   move     x' = min(max(x + speed CX[k], 0), map_size), y' likewise with CY
 * When the moves happen is the caller's business (motion.MovingTargetEnv: before every `every`-th step). */
enum { CS_MOTION_WALK = 0, CS_MOTION_EVADE = 1 };
typedef struct cs_motion_params {
    int32_t mode;         /* CS_MOTION_WALK or CS_MOTION_EVADE */
    int32_t persist;      /* time steps for which a walk heading is kept: 1..65536 */
    uint32_t seed;        /* seed of the heading keys */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
    double speed;         /* cells per move: finite, 0..map_size; 0: no launch, nothing moves */
    double sense;         /* evade: the radius inside which a target sees an agent: finite, 0..2 map_size */
    int64_t env_offset;   /* global index of env 0, 0..2^62 */
} cs_motion_params;

/* One launch on `stream` (none when speed is 0), 16 lanes per env, no atomics, no synchronisation.  CS_E_CONFIG (before any
 * launch) for a cfg that cs_state_layout refuses, a field out of range, a non-zero `reserved`, a NULL pointer or a state_dev
 * that is not 16-byte aligned.  The message is cs_episodes_last_error()'s (cs_last_error() holds it too). */
int cs_move_targets(const cs_config *cfg, void *state_dev, const cs_motion_params *p, void *stream);

/* ---- target-density filter policy for moving targets, one launch per decision ----------------
 * cs_coverage_actions' belief grid knows nothing of motion.  This policy keeps, per env, the expected density D of unfound
 * targets -- int32 [side * side], row-major [ix * side + iy], Q16: 65536 = one cell's worth of "nobody has looked", the caller
 * fills it with 65536 when an episode starts; a cell is read as clamp(cell, 0, 2^19), so a whole map sums to at most 2^31 -- and
 * the quantised positions of the agents at the previous call (prev, read clamped to +-2^15; slots >= n_agents are never
 * touched).  A call PREDICTS (only if moved): every cell sends its mass through the targets' motion model -- one sixteenth along
 * each of the 16 headings of cs_move_targets (displacement dx[k], dy[k] sub-units of 1/16 cell), or, in mode CS_MOTION_EVADE for
 * a cell whose centre lies within sense16 sub-units of an agent's PREVIOUS position, all of it along the heading that leads away
 * from the nearest such agent -- split bilinearly over four cells, destinations clamped to the map; then it SWEEPS: the cells
 * within 16 view_range sub-units of a current agent are multiplied by keep / 65536; then the agents CHOOSE as
 * cs_coverage_actions' do.  DEFINED by belief.belief_actions_torch (stock torch ops, integer after one quantisation); the kernel
 * reproduces grid, prev and actions element for element.
 *   state_dev  float [B][state_width] (the first 4 n_agents floats of a get_state() row are read)
 *   grid_dev   int32 [B][side * side], in / out     prev_dev  int32 [B][8][2], in / out     actions_dev  int64 [B][n_agents], out */
typedef struct cs_belief_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t keep;         /* rint((1 - detect_prob) * 65536), 0..65536 */
    int32_t lookahead;    /* distance of the look-ahead point in cells, 0..side */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t mode;         /* the motion model: CS_MOTION_WALK or CS_MOTION_EVADE */
    int32_t moved;        /* 1: the targets moved since the previous call (predict first); 0: they did not */
    int32_t sense16;      /* rint(16 sense), 0..2048 (evade only) */
    int32_t dx[16];       /* rint(16 speed cos(2 pi k / 16)), -1024..1024 */
    int32_t dy[16];       /* rint(16 speed sin(2 pi k / 16)), -1024..1024 */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_belief_params;

/* One launch on `stream`, one workgroup per env, atomics on LDS only (integer: the result does not depend on their order), no
 * synchronisation.  CS_E_CONFIG (before any launch) for a field out of range, a non-zero `reserved`, a NULL or misaligned
 * pointer or B < 1.  The message is cs_episodes_last_error()'s. */
int cs_belief_actions(const cs_belief_params *p, const float *state_dev, int B, int32_t *grid_dev, int32_t *prev_dev,
                      int64_t *actions_dev, void *stream);

/* ---- the density filter under a limited communication range: n private densities per env, one launch per decision (DESIGN.md
 * section 26) ---------------------------------------------------------------------------------------------------------------
 * cs_belief_actions keeps one density per env and predicts it with the positions of all agents.  Here agent i keeps a density of
 * its own (cells read as clamp(cell, 0, 2^19)) and the link mask of the previous call: bit j of heard[i] says that agent i heard
 * agent j then; it is read as (heard[i] & ((1 << n_agents) - 1)) | (1 << i).  A call PREDICTS (only if moved): agent i runs
 * cs_belief_actions' prediction step on its own grid, its evade test seeing only the agents in heard[i], at their prev positions;
 * it SWEEPS: agent i multiplies by keep / 65536 the cells within 16 view_range sub-units of ITS OWN current position (S_i); it
 * MERGES: with cs_local_coverage_actions' link test on the current positions, M_i = min over the linked j of S_j, cell by cell (one
 * hop per call; the minimum starts at 2^19 + 1), is written back; it STORES prev[i] = the quantised position and heard[i] = the
 * mask of the agents linked to i now, for i < n_agents (slots >= n_agents of both are never touched); then the agents CHOOSE as
 * cs_local_coverage_actions' do.  With comm_range -1 and equal grids this IS cs_belief_actions; with comm_range 0 every agent is a
 * one-agent cs_belief_actions.  DEFINED by local_belief.local_belief_actions_torch (stock torch ops, integer after one
 * quantisation); the kernel reproduces grids, prev, heard and actions bit for bit.
 *   state_dev  float [B][state_width]             grids_dev  int32 [B][n_agents][side * side], in / out
 *   prev_dev   int32 [B][8][2], in / out          heard_dev  int32 [B][8], in / out      actions_dev  int64 [B][n_agents], out */
typedef struct cs_local_belief_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t keep;         /* rint((1 - detect_prob) * 65536), 0..65536 */
    int32_t lookahead;    /* distance of the look-ahead point in cells, 0..side */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t mode;         /* the motion model: CS_MOTION_WALK or CS_MOTION_EVADE */
    int32_t moved;        /* 1: the targets moved since the previous call (predict first); 0: they did not */
    int32_t sense16;      /* rint(16 sense), 0..2048 (evade only) */
    int32_t dx[16];       /* rint(16 speed cos(2 pi k / 16)), -1024..1024 */
    int32_t dy[16];       /* rint(16 speed sin(2 pi k / 16)), -1024..1024 */
    int32_t comm_range;   /* communication range in whole cells, 0..128, or -1: unlimited */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_local_belief_params;

/* One launch on `stream`, one workgroup per env, atomics on LDS only (integer: the result does not depend on their order), no
 * synchronisation.  CS_E_CONFIG (before any launch) for a field out of range, a non-zero `reserved`, a NULL or misaligned
 * pointer or B < 1.  The message is cs_episodes_last_error()'s. */
int cs_local_belief_actions(const cs_local_belief_params *p, const float *state_dev, int B, int32_t *grids_dev, int32_t *prev_dev,
                            int32_t *heard_dev, int64_t *actions_dev, void *stream);

/* ---- receding-horizon planner over a base policy's grid, one launch per decision -------------
 * cs_coverage_actions and cs_belief_actions score three look-ahead points whose footprints overlap almost entirely: mass abeam of
 * an agent or behind it scores 0 on all three and the agent flies straight on.  This planner reads the grid either of them left
 * (int32 [side * side], row-major [ix * side + iy]; READ ONLY, every cell as clamp(cell, 0, 2^19), so a whole map sums to at most
 * 2^31) and, per env, lets the agents decide in index order on a working copy W: the 3^depth sequences of `depth` segments, each
 * "hold action a for `stride` steps" (one step: h = (h + {0, 1, 35}[a]) % 36, x = clamp(x + ((16 CT[h]) >> 14), 0, 16 side), y
 * likewise), are scored by the sum over their segment end points of (the mass of W within 16 view_range sub-units of the point and
 * of no earlier point of the sequence) * w_d, w_0 = 256, w_d = (w_{d-1} discount) >> 8; the lowest sequence index of the largest
 * score wins (the index: `depth` base-3 digits, the first segment the most significant), the action is its first digit, and W is
 * zeroed on that sequence's discs before the next agent decides.  DEFINED by plan.plan_actions_torch (stock torch ops, integer
 * after one quantisation); the kernel reproduces actions, plans and scores element for element.
 *   state_dev  float [B][state_width] (the first 4 n_agents floats of a get_state() row are read)
 *   grid_dev   int32 [B][side * side], in     actions_dev, plans_dev, scores_dev  int64 [B][n_agents], out: the action, the
 *   winning sequence index and its score (at most 2^39) */
typedef struct cs_plan_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t depth;        /* segments per sequence, 1..5 */
    int32_t stride;       /* env steps per segment, 1..8 */
    int32_t discount;     /* Q8 weight ratio of successive segments, 0..256 */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_plan_params;

/* One launch on `stream`, one workgroup per env, no atomics, no synchronisation.  CS_E_CONFIG (before any launch) for a field out
 * of range, a non-zero `reserved`, a NULL or misaligned pointer or B < 1.  The message is cs_episodes_last_error()'s. */
int cs_plan_actions(const cs_plan_params *p, const float *state_dev, int B, const int32_t *grid_dev, int64_t *actions_dev,
                    int64_t *plans_dev, int64_t *scores_dev, void *stream);

/* ---- the density predicted along the planning horizon, and the planner scored on it ----------
 * cs_plan_actions scores every segment of a sequence on the density of NOW; moving targets leave it within a few steps.
 * cs_belief_forecast runs cs_belief_actions' prediction step forward with the agents held at pos: level d of `stack` is the
 * grid (every cell read as clamp(cell, 0, 2^19)) after moves[0] + .. + moves[d] prediction steps, each capped at 2^19; a level
 * with moves[d] == 0 is a copy of the level before it (of the clamped grid for d = 0).  cs_plan_forecast_actions is
 * cs_plan_actions with `depth` levels: the gain of a segment end point d is summed over level d, and the winner's discs are
 * zeroed in every level.  DEFINED by forecast.forecast_torch and forecast.plan_forecast_actions_torch (stock torch ops, all
 * integer); the kernels reproduce them element for element.  A stack of identical levels gives cs_plan_actions' outputs.
 *   grid_dev   int32 [B][side * side], in     pos_dev  int32 [B][8][2], in (cs_belief_actions' prev, read clamped to +-2^15)
 *   stack_dev  int32 [B][levels][side * side], out of cs_belief_forecast, in (READ ONLY) of cs_plan_forecast_actions, whose
 *   `depth` is the number of levels; state_dev, actions_dev, plans_dev, scores_dev as cs_plan_actions' */
typedef struct cs_forecast_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t levels;       /* levels of the stack, 1..5 */
    int32_t mode;         /* the motion model: CS_MOTION_WALK or CS_MOTION_EVADE */
    int32_t sense16;      /* rint(16 sense), 0..2048 (evade only) */
    int32_t dx[16];       /* rint(16 speed cos(2 pi k / 16)), -1024..1024 */
    int32_t dy[16];       /* rint(16 speed sin(2 pi k / 16)), -1024..1024 */
    int32_t moves[5];     /* prediction steps from level d - 1 to level d, 0..8; 0 for d >= levels */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_forecast_params;

/* One launch each on `stream`, one workgroup per env, atomics on LDS only (cs_belief_forecast; integer: the result does not
 * depend on their order), no synchronisation.  cs_plan_forecast_actions takes 3.3 KB + 4 depth side^2 bytes of LDS (85 KB at
 * side 64 and depth 5).  CS_E_CONFIG (before any launch) for a field out of range, a non-zero `reserved`, a NULL or misaligned
 * pointer or B < 1.  The message is cs_episodes_last_error()'s. */
int cs_belief_forecast(const cs_forecast_params *p, const int32_t *grid_dev, const int32_t *pos_dev, int B, int32_t *stack_dev,
                       void *stream);
int cs_plan_forecast_actions(const cs_plan_params *p, const float *state_dev, int B, const int32_t *stack_dev, int64_t *actions_dev,
                             int64_t *plans_dev, int64_t *scores_dev, void *stream);

/* ---- an expert relabels a recorded batch of episodes, one launch per batch -------------------
 * Imitation learning (DAgger) asks what cs_coverage_actions or cs_belief_actions WOULD have done in every state another policy
 * reached.  Those experts decide from (state row, t) and their own grid alone, so walking the recorded rows s[e][0..T-1] of every
 * episode in order, from a fresh grid (65536 everywhere, stored positions 0), gives what shadowing the flight would have given.
 * Row t of a belief expert is cs_belief_actions with moved = (moving && t > 0 && (t - 1) % every == 0); row t of a coverage expert is
 * cs_coverage_actions.  Only the rows t < lens[e] are walked (lens[e] is read clamped to 0..T): the rows behind them are never read,
 * their labels are 0, and the episode's grid and positions stay as its last live row left them.  DEFINED by
 * imitate.label_episodes_torch (a loop over the two definitions); the kernel reproduces labels, grid_out and prev_out element for
 * element, with the expert's grid in LDS from the first row to the last.
 *   s_dev       float [E][T][state_width], in (the first 4 n_agents floats of a row are read)      lens_dev  int32 [E], in
 *   labels_dev  int64 [E][T][n_agents], out    grid_out_dev  int32 [E][side * side], out, or NULL
 *   prev_out_dev  int32 [E][8][2], out, or NULL; belief only (slots >= n_agents are written as 0) */
typedef struct cs_label_params {
    int32_t expert;       /* 0: cs_coverage_actions' policy, 1: cs_belief_actions' */
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t keep;         /* rint((1 - detect_prob) * 65536), 0..65536 */
    int32_t regrow;       /* regrowth shift, 1..16 (coverage; checked, then unused, for belief) */
    int32_t lookahead;    /* distance of the look-ahead point in cells, 0..side */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t mode;         /* belief: the motion model, CS_MOTION_WALK or CS_MOTION_EVADE */
    int32_t sense16;      /* belief: rint(16 sense), 0..2048 (evade only) */
    int32_t every;        /* belief: env steps between two moves of the targets, >= 1 */
    int32_t moving;       /* belief: 1 if the targets move at all (speed > 0), else 0 */
    int32_t dx[16];       /* belief: rint(16 speed cos(2 pi k / 16)), -1024..1024 */
    int32_t dy[16];       /* belief: rint(16 speed sin(2 pi k / 16)), -1024..1024 */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_label_params;

/* One launch on `stream`, one workgroup per episode, atomics on LDS only (integer: the result does not depend on their order), no
 * synchronisation.  CS_E_CONFIG (before any launch) for a field out of range, a non-zero `reserved`, a NULL or misaligned pointer
 * (grid_out_dev and prev_out_dev may be NULL; prev_out_dev must be NULL for the coverage expert), E < 1 or T < 1.  The message is
 * cs_episodes_last_error()'s. */
int cs_label_episodes(const cs_label_params *p, const float *s_dev, int E, int T, const int32_t *lens_dev, int64_t *labels_dev,
                      int32_t *grid_out_dev, int32_t *prev_out_dev, void *stream);

/* ---- grid observations: sixteen floats per agent from the grid of a coverage or belief policy ---
 * The agent network observes (x, y, cos, sin); the search policies decide from their grid.  These two calls summarise the grid
 * for the network: per agent, probe k = 8 ring + b (ring 0..1, b 0..7) lies {1, 3}[ring] * lookahead cells along the heading turned
 * by {0, 1, 35, 4, 32, 9, 27, 18}[b] * pi / 18, clamped to the map as cs_coverage_actions' look-ahead points are (probes 0, 1, 2 ARE
 * those points); sum_k is the sum of clamp(cell, 0, 2^19) over the cells whose centre lies within 16 view_range sub-units of the
 * probe, and the feature is float(sum_k >> 8) * 2^-15 -- exact: sum_k <= 2^31.  Every agent reads the same grid (no claims).
 * DEFINED by gridobs.grid_features_torch and gridobs.feature_episodes_torch (stock torch ops, integer after one quantisation);
 * the kernels reproduce them bit for bit.
 *   cs_grid_features     per decision, on the grid cs_coverage_actions or cs_belief_actions left after its call on the same state:
 *     state_dev  float [B][state_width], in     grid_dev  int32 [B][side * side], in (READ ONLY)     feat_dev  float [B][n_agents][16], out
 *   cs_feature_episodes  for a recorded batch: cs_label_episodes' walk (same params, same s_dev / lens_dev / outputs) that also
 *     writes the features of the grid as every live row's step left it:
 *     feat_dev  float [E][T][n_agents][16], out (rows t >= lens[e]: 0)     labels_dev  int64 [E][T][n_agents], out, or NULL: the
 *     choose step is skipped altogether     grid_out_dev, prev_out_dev  as cs_label_episodes', or NULL */
typedef struct cs_grid_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t lookahead;    /* distance of the inner ring in cells, 0..side */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_grid_params;

/* One launch each on `stream`, one workgroup per env / per episode, no global atomics (cs_feature_episodes: LDS atomics as
 * cs_label_episodes), no synchronisation.  CS_E_CONFIG (before any launch) for a field out of range, a non-zero `reserved`, a NULL or
 * misaligned pointer (labels_dev, grid_out_dev and prev_out_dev may be NULL; prev_out_dev must be NULL for the coverage filter), B <
 * 1, E < 1 or T < 1.  The message is cs_episodes_last_error()'s. */
int cs_grid_features(const cs_grid_params *p, const float *state_dev, int B, const int32_t *grid_dev, float *feat_dev, void *stream);
int cs_feature_episodes(const cs_label_params *p, const float *s_dev, int E, int T, const int32_t *lens_dev, float *feat_dev,
                        int64_t *labels_dev, int32_t *grid_out_dev, int32_t *prev_out_dev, void *stream);

/* ---- grid observations of PRIVATE grids: sixteen floats per agent from its own grid under a communication range (DESIGN.md
 * section 27) ------------------------------------------------------------------------------------------------------------------
 * cs_grid_features reads the one grid of an env for every agent.  cs_local_coverage_actions and cs_local_belief_actions keep one
 * grid per AGENT; here agent i's sixteen probes (the same probe points, sums, shift and scale) read grids[b][i] alone.
 * DEFINED by localobs.local_grid_features_torch and localobs.local_feature_episodes_torch (stock torch ops, integer after one
 * quantisation); the kernels reproduce them bit for bit.
 *   cs_local_grid_features     per decision, on the grids cs_local_coverage_actions or cs_local_belief_actions left after its call
 *     on the same state:
 *     state_dev  float [B][state_width], in     grids_dev  int32 [B][n_agents][side * side], in (READ ONLY)
 *     feat_dev   float [B][n_agents][16], out
 *   cs_local_feature_episodes  for a recorded batch: row t of a coverage filter (expert 0) is cs_local_coverage_actions, row t of a
 *     belief filter (expert 1) is cs_local_belief_actions with moved = (moving && t > 0 && (t - 1) % every == 0), from n fresh grids
 *     (65536 everywhere, stored positions and link masks 0), followed by cs_local_grid_features on the grids as the row left them.
 *     Only the rows t < lens[e] are walked (lens[e] is read clamped to 0..T).
 *     s_dev, lens_dev  as cs_label_episodes'     feat_dev  float [E][T][n_agents][16], out (rows t >= lens[e]: 0)
 *     labels_dev  int64 [E][T][n_agents], out (rows t >= lens[e]: 0), or NULL: the choose step is skipped altogether
 *     grids_dev   int32 [E][n_agents][side * side], REQUIRED: the kernel's workspace (it fills it itself; the content on entry does
 *                 not matter), and on return every agent's grid after the episode's last live row
 *     prev_dev    int32 [E][8][2], out, or NULL; heard_dev  int32 [E][8], out, or NULL; both belief only (slots >= n_agents: 0) */
typedef struct cs_local_label_params {
    int32_t expert;       /* 0: cs_local_coverage_actions' policy, 1: cs_local_belief_actions' */
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t keep;         /* rint((1 - detect_prob) * 65536), 0..65536 */
    int32_t regrow;       /* regrowth shift, 1..16 (coverage; checked, then unused, for belief) */
    int32_t lookahead;    /* distance of the look-ahead point and of the inner probe ring in cells, 0..side */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t mode;         /* belief: the motion model, CS_MOTION_WALK or CS_MOTION_EVADE */
    int32_t sense16;      /* belief: rint(16 sense), 0..2048 (evade only) */
    int32_t every;        /* belief: env steps between two moves of the targets, >= 1 */
    int32_t moving;       /* belief: 1 if the targets move at all (speed > 0), else 0 */
    int32_t dx[16];       /* belief: rint(16 speed cos(2 pi k / 16)), -1024..1024 */
    int32_t dy[16];       /* belief: rint(16 speed sin(2 pi k / 16)), -1024..1024 */
    int32_t comm_range;   /* communication range in whole cells, 0..128, or -1: unlimited */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_local_label_params;

/* One launch each on `stream`, one workgroup per env / per episode, no global atomics (cs_local_feature_episodes: LDS atomics as
 * cs_local_belief_actions), no synchronisation.  CS_E_CONFIG (before any launch) for a field out of range (expert included), a
 * non-zero `reserved`, a NULL or misaligned required pointer (labels_dev, prev_dev and heard_dev may be NULL; prev_dev and heard_dev
 * must be NULL for the coverage filter), B < 1, E < 1 or T < 1.  Both decide their 16-byte paths themselves.  The message is
 * cs_episodes_last_error()'s. */
int cs_local_grid_features(const cs_grid_params *p, const float *state_dev, int B, const int32_t *grids_dev, float *feat_dev,
                           void *stream);
int cs_local_feature_episodes(const cs_local_label_params *p, const float *s_dev, const int32_t *lens_dev, int E, int T, float *feat_dev,
                              int64_t *labels_dev, int32_t *grids_dev, int32_t *prev_dev, int32_t *heard_dev, void *stream);

/* ---- the receding-horizon planner on PRIVATE grids under a communication range, one launch per decision ----
 * cs_plan_actions reads one grid per env and lets every agent see every earlier agent's claim.  Here agent i plans on its own grid,
 * grids[b][i] (what cs_local_coverage_actions or cs_local_belief_actions left; READ ONLY, every cell as clamp(cell, 0, 2^19)), less
 * the discs of the winning sequences of the agents j < i that it is linked to: cs_local_coverage_actions' link test on the current
 * positions (i == j, or comm_range < 0, or (X_i - X_j)^2 + (Y_i - Y_j)^2 < (16 comm_range)^2 in sub-units; strict, 64-bit).  The
 * sequences, their end points, the gains less the ancestors' discs, the weights, the score, the tie rule and the action are
 * cs_plan_actions'.  With comm_range -1 and equal grids this IS cs_plan_actions; with comm_range 0 every agent is a one-agent
 * cs_plan_actions on its own grid.  DEFINED by local_plan.local_plan_actions_torch (stock torch ops, integer after one
 * quantisation); the kernel reproduces actions, plans and scores bit for bit.
 *   state_dev  float [B][state_width]       grids_dev  int32 [B][n_agents][side * side], in
 *   actions_dev, plans_dev, scores_dev  int64 [B][n_agents], out, as cs_plan_actions' */
typedef struct cs_local_plan_params {
    int32_t n_agents;     /* 1..8 */
    int32_t side;         /* map_size: cells per side, 1..CS_MAX_MAP */
    int32_t view_range;   /* sensor radius in cells, 0..CS_MAX_MAP */
    int32_t depth;        /* segments per sequence, 1..5 */
    int32_t stride;       /* env steps per segment, 1..8 */
    int32_t discount;     /* Q8 weight ratio of successive segments, 0..256 */
    int32_t state_width;  /* floats per state row, >= 4 n_agents */
    int32_t comm_range;   /* communication range in whole cells, 0..128, or -1: unlimited */
    int32_t reserved;     /* must be 0 (CS_E_CONFIG otherwise) */
} cs_local_plan_params;

/* One launch on `stream`, one workgroup per env, no atomics, no synchronisation.  CS_E_CONFIG (before any launch) for a field out
 * of range, a non-zero `reserved`, a NULL or misaligned pointer or B < 1.  It decides its 16-byte path itself.  The message is
 * cs_episodes_last_error()'s. */
int cs_local_plan_actions(const cs_local_plan_params *p, const float *state_dev, int B, const int32_t *grids_dev, int64_t *actions_dev,
                          int64_t *plans_dev, int64_t *scores_dev, void *stream);

/* ---- the forecast planner on PRIVATE grids under a communication range ------------------------------------
 * cs_belief_forecast predicts ONE grid per env with every agent held in place.  cs_local_belief_forecast predicts agent i's own grid,
 * grids[b][i], with the agents of heard[b][i] alone held at their prev positions: the word is read as cs_local_belief_actions reads
 * it ((heard & ((1 << n_agents) - 1)) | (1 << i)), the heard agents are listed in index order, and levels, moves, the clamp and the
 * cap are cs_belief_forecast's.  After a cs_local_belief_actions call prev holds the current positions and heard the links of that
 * call.  In walk mode the mask plays no part.  cs_local_plan_forecast_actions is cs_local_plan_actions with `depth` levels per agent:
 * the gain of a segment end point d is summed over level d of agent i's stack, and the claims of the linked agents j < i are zeroed in
 * every level.  DEFINED by local_forecast.local_forecast_torch and local_forecast.local_plan_forecast_actions_torch (stock torch ops,
 * integer after one quantisation); the kernels reproduce them bit for bit.  Both reuse an existing params struct.
 *   grids_dev   int32 [B][n_agents][side * side], in      prev_dev  int32 [B][8][2], in      heard_dev  int32 [B][8], in
 *   stacks_dev  int32 [B][n_agents][levels][side * side], out of cs_local_belief_forecast, in (READ ONLY) of
 *   cs_local_plan_forecast_actions, whose `depth` is the number of levels; state_dev, actions_dev, plans_dev, scores_dev as
 *   cs_local_plan_actions'
 * One launch each on `stream`: cs_local_belief_forecast one workgroup per (env, agent) with atomics on LDS only (integer: the result
 * does not depend on their order), cs_local_plan_forecast_actions one workgroup per env with 3.5 KB + 4 depth side^2 bytes of LDS
 * (85.4 KB at side 64 and depth 5; CS_E_LAUNCH if the device does not grant it).  No synchronisation.  CS_E_CONFIG (before any
 * launch) for a field out of range, a non-zero `reserved`, a NULL or misaligned pointer or B < 1.  The message is
 * cs_episodes_last_error()'s. */
int cs_local_belief_forecast(const cs_forecast_params *p, const int32_t *grids_dev, const int32_t *prev_dev, const int32_t *heard_dev,
                             int B, int32_t *stacks_dev, void *stream);
int cs_local_plan_forecast_actions(const cs_local_plan_params *p, const float *state_dev, int B, const int32_t *stacks_dev,
                                   int64_t *actions_dev, int64_t *plans_dev, int64_t *scores_dev, void *stream);

/* ---- QMIX learner: the GRU recurrence of the agent network over T steps, forward and backward ---------------------
 * Replaces the per-transition unroll of policy/qmix.py:160-182 (get_q_values) over network/base_net.py:40-46
 * (GRUCell(64)) and autograd's walk back through it: ONE launch for all T steps of all rows, whatever T is.  The batched
 * parts (fc1, the input projection gi = W_ih x + b_ih, fc2, the mixer, dW_hh, db_hh) stay with the caller.  Gate rows of
 * the 192-wide tensors are ordered [r | z | n] (torch.nn.GRUCell); all tensors are float32, contiguous, on the device;
 * rows = E * n_agents, row order free (rows never mix).  The products run on the split-fp16 matrix path of
 * cs_policy_forward (~2e-5 against fp32 torch); the backward scales each group of 16 rows by a power of two so that its
 * gradients keep full precision whatever their magnitude.  Results do not depend on the launch geometry: bit-identical
 * from run to run.
 *
 * Forward.  gi [T][rows][192]; w_hh [192][64], b_hh [192] (rnn.weight_hh / rnn.bias_hh as they are); h0 [rows][64] or
 * NULL (zeros, init_hidden of policy/qmix.py:184-187) -> h_out [T][rows][64] = h_1 .. h_T; saved_out [T][rows][4][64] =
 * (r, z, n, gh_n) of every step for cs_gru_seq_backward, or NULL (no-grad forward: the target network). */
int cs_gru_seq_forward(const float *w_hh, const float *b_hh, const float *gi, const float *h0, int T, int rows,
                       float *h_out, float *saved_out, void *stream);
/* Backward.  dh_seq [T][rows][64] = dloss/dh_t from the layers above (fc2) for every t; h_seq, h0, saved as produced by
 * the forward (h0 NULL = zeros) -> dgi_out [T][rows][192] = dloss/dgi_t, dgh_out [T][rows][192] = dloss/dgh_t (gh = W_hh h +
 * b_hh), dh0_out [rows][64] = dloss/dh0 or NULL.  dW_hh = sum_t dgh_t^T h_{t-1} and db_hh = sum_t dgh_t are left to one
 * matrix product / sum over the T * rows rows. */
int cs_gru_seq_backward(const float *w_hh, const float *dh_seq, const float *h_seq, const float *h0,
                        const float *saved, int T, int rows, float *dgi_out, float *dgh_out,
                        float *dh0_out, void *stream);
/* DOP / REINFORCE learners: the backward recursion over t of the returns, ONE launch for all E episodes and T steps.
 * r, terminated, padded [E][T] (the batch's [E][T][1] float32 tensors); q [E][T] = q_total_target of the target mixer, or
 * NULL.  With m = 1 - padded, c = 1 - terminated:
 *   q == NULL: out = REINFORCE's discounted return (policy/reinforce.py:101-110)
 *              R[T-1] = r m,  R[t] = (r[t] + gamma R[t+1] c[t]) m[t]
 *   q != NULL: out = DOP's TD(lambda) target (policy/dop.py:192-232, its O(T^2) n-step sum as a recursion)
 *              L[T-1] = (r + gamma q c) m,  L[t] = (r[t] + gamma ((1 - lambda) c[t] q[t] + lambda L[t+1])) m[t]
 * fp32 in the evaluation order stated in csrc/returns.h (no fused multiply-adds: a float32 restatement of that order is
 * bit-identical); no atomics, so reruns are bit-identical.  lambda is ignored when q is NULL. */
int cs_episode_returns(const float *r, const float *terminated, const float *padded, const float *q, int E, int T,
                       float gamma, float lambda, float *out, void *stream);
/* PPO learner (learner.PPOLearner): generalised advantage estimation, ONE launch for all E episodes and T steps.
 * r, terminated, padded, v = V(s), v_next = V(s_next) [E][T] float32 -> adv_out, ret_out [E][T].  With m = 1 - padded,
 * c = 1 - terminated, gl = gamma * lambda, in fp32 in this order (no fused multiply-adds: a float32 restatement is
 * bit-identical; csrc/ppo.h):
 *   delta = (r + (gamma * v_next) * c) - v
 *   A[T-1] = delta * m,  A[t] = (delta + (gl * A[t+1]) * c) * m,  ret = (A + v) * m
 * With v = v_next = 0 and lambda = 1, adv_out equals cs_episode_returns' REINFORCE return bit for bit.  Padded steps are
 * exactly zero (finite inputs).  No atomics: reruns are bit-identical. */
int cs_gae(const float *r, const float *terminated, const float *padded, const float *v, const float *v_next, int E, int T,
           float gamma, float lambda, float *adv_out, float *ret_out, void *stream);
/* PPO's clipped surrogate with an entropy bonus, its statistics and its gradient with respect to the logits, in one pass over
 * the rows = E * T * n_agents rows (row rho belongs to step rho / n_agents).  logits, avail [rows][n_actions] float32 (2 to 8
 * actions), u [rows] int64, old_logp [rows] or NULL, adv, mask [rows / n_agents].  epsilon (the exploration mix of the
 * action probabilities) is read from epsilon_dev[0] when that is set, else from `epsilon`; inv_count_dev[0] =
 * 1 / (n_agents * sum(mask)), a device scalar.  Per row with mask != 0: p = the reference actors' action probabilities
 * (softmax, epsilon mix over the available actions, unavailable ones zeroed, renormalised), logp = log p[u],
 * ratio = exp(logp - old_logp), surr = min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv), H = -sum p log p.
 *   old_logp == NULL: only logp_out [rows] is written (the no-grad pass; adv, inv_count_dev and the outputs below unused).
 *   old_logp != NULL: dlogits_out [rows][n_actions] = d(inv_count * sum mask (-surr - ent_coef H)) / dlogits, the gradient
 *     passing where the unclipped term is the active one (both clip boundaries included: torch.clamp / torch.minimum);
 *     stats_out [4] = (policy loss = -mean surr, mean H, fraction of rows with ratio outside the clip range,
 *     mean(old_logp - logp)), means over the live rows; logp_out [rows] or NULL.
 * Rows with mask == 0 give zeros everywhere, whatever their other inputs hold.  scratch_dev: scratch_floats >=
 * 4 * ceil(rows / CS_PPO_BLOCK) floats (one partial per block; a second one-block launch adds them in a fixed order).  No
 * atomics: reruns are bit-identical. */
#define CS_PPO_BLOCK 256
int cs_ppo_loss(const float *logits, const float *avail, const int64_t *u, const float *old_logp, const float *adv,
                const float *mask, int64_t rows, int n_agents, int n_actions, float clip, float ent_coef, float epsilon,
                const float *epsilon_dev, const float *inv_count_dev, float *dlogits_out, float *logp_out, float *stats_out,
                float *scratch_dev, int64_t scratch_floats, void *stream);
/* Imitation learner (imitate.ImitationLearner): the masked cross-entropy between the actor's action probabilities and an expert's
 * labels, its statistics and its gradient with respect to the logits, in one pass over the rows = E * T * n_agents rows (row rho
 * belongs to step rho / n_agents).  logits, avail [rows][n_actions] float32 (2 to 8 actions), labels [rows] int64, mask
 * [rows / n_agents]; inv_count_dev[0] = 1 / (n_agents * sum(mask)), a device scalar.  Per row with mask != 0: p = the reference
 * actors' action probabilities with epsilon 0 (softmax, unavailable actions zeroed, renormalised), ce = -log p[label].
 *   dlogits_out [rows][n_actions] = d(inv_count * sum mask ce) / dlogits = mask inv_count (p - onehot(label))
 *   stats_out [3] = (loss = mean ce, agreement = mean [argmax p == label], the lowest index on ties, mean entropy -sum p log p),
 *     means over the live rows.
 * A live row whose label is unavailable (or outside 0..n_actions - 1) adds no loss and no gradient and counts as a miss.  Rows with
 * mask == 0 give zeros everywhere, whatever their other inputs hold.  scratch_dev: scratch_floats >= 3 * ceil(rows /
 * CS_PPO_BLOCK) floats (one partial per block; a second one-block launch adds them in a fixed order).  No atomics: reruns are
 * bit-identical.  CS_E_ARG (before any launch) for a NULL pointer or a count out of range; the message is cs_learn_last_error()'s. */
int cs_bc_loss(const float *logits, const float *avail, const int64_t *labels, const float *mask, int64_t rows, int n_agents,
               int n_actions, const float *inv_count_dev, float *dlogits_out, float *stats_out, float *scratch_dev,
               int64_t scratch_floats, void *stream);
const char *cs_learn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
