/*
 * mse.h -- C ABI of libmse_hip.so: the MI355X-native batched step() engine for the three
 * MARL-SortingEnv environments.
 *
 * The reference has no FFI: its boundary for this path is the Python Gymnasium protocol of
 * Env_1_Sorting / Env_2_Pressing / Env_3_Monolith (one env instance, NumPy on the host).  Each
 * entry point below names the reference interface it replaces (path:line in the reference
 * checkout).  N independent env instances live in one handle, one env per GPU lane, state as
 * struct-of-arrays planes in HBM that the library owns; every I/O buffer is CALLER-owned DEVICE
 * memory (contiguous, row-major, 16-byte aligned), e.g. a PyTorch-ROCm tensor's data_ptr().
 *
 * Conventions
 *   - every function returns 0 (MSE_OK) or a negative mse_status; nothing throws across the ABI;
 *     mse_last_error() gives the message of the calling thread's last failure;
 *   - all device work is enqueued on the caller's HIP stream (`stream` is a hipStream_t passed as
 *     void*, NULL = the default stream); no hidden synchronisation, graph-capture safe
 *     (mse_step / mse_rollout / mse_reset / mse_action_masks allocate nothing and never sync);
 *   - a handle is not thread-safe; different handles are independent;
 *   - there is NO CPU fallback: the library needs a gfx950 device and fails loudly without one.
 */
#ifndef MSE_H
#define MSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSE_VERSION 200 /* 0.2.0 */

typedef enum mse_status {
    MSE_OK = 0,
    MSE_ERR_INVALID_ARGUMENT = -1,
    MSE_ERR_UNSUPPORTED_CONFIG = -2,
    MSE_ERR_NO_DEVICE = -3,
    MSE_ERR_HIP = -4,
    MSE_ERR_NOT_RESET = -5,
    MSE_ERR_ALIGNMENT = -6
} mse_status;

/* env_1_sort.py:26 "sort", env_2_press.py:26 "press", env_monolith.py:28 "mono" */
typedef enum mse_env_kind { MSE_ENV_SORT = 1, MSE_ENV_PRESS = 2, MSE_ENV_MONO = 3 } mse_env_kind;

/* per-call step flags = the reference's step() keyword arguments
 * (env_monolith.py:109, env_2_press.py:88, env_1_sort.py:97) */
#define MSE_STEP_UNMASKED       1u /* use_action_masking=False: validate + sanitise the press action */
#define MSE_STEP_CHECK_OVERFLOW 2u /* check_overflow=True: overflow terminates with the -10 penalty  */
/* mse_rollout only: act with the reference's rule-based policy (mode='rule_based', env_monolith.py:166-184:
 * sorting_rules() env_super.py:469-482 + check_container_level() :689-720) instead of the random one */
#define MSE_ROLLOUT_RULE_BASED  4u
/* with MSE_STEP_UNMASKED on Env_3: test the press action's validity AFTER sort_material instead of at decode time -
 * what Env_3_Monolith.step(action=None, mode='random', use_action_masking=False) does (env_monolith.py:245-253:
 * sanitize_press_action runs in the "apply" section; an invalid action still skips press_action_rules) */
#define MSE_STEP_SANITIZE_LATE  8u
/* mse_model_actions only: leave the sorting / the pressing decision to an agent (no draw, that part is 0) */
#define MSE_MODEL_NO_SORT_DRAW  16u
#define MSE_MODEL_NO_PRESS_DRAW 32u

/* POD copy of the reference's config.yml plus the env constructor arguments
 * (env_super.py:25-137 reads the same keys; env_monolith.py:22-23 ctor). */
typedef struct mse_config {
    uint32_t struct_size;          /* = sizeof(mse_config); ABI check */
    int32_t  env_kind;             /* mse_env_kind */
    int32_t  max_steps;            /* ctor max_steps (<= 65535) */
    int32_t  auto_reset;           /* 1: a terminated env is reset inside the same step (VecEnv semantics) */
    int32_t  track_bales;          /* 1: keep the O(1) bale ledger summary (env_super.py:661-687) */
    int32_t  literal_choice;       /* 1: always evaluate Generator.choice(4,p) in literal fp64 (test switch);
                                      0: exact integer decision with literal fallback near ties */
    /* simulation (config.yml:4-9) */
    int32_t  input_batch_size;     /* <= 255.  If floor(ratio * batch) leaves units over (e.g. 90), the generator's
                                      random remainder + shuffle draws run on the device ("general generator mode",
                                      utils/input_generator.py:46-61) and the one-lane kernels serve the handle */
    int32_t  steps_per_pattern;    /* informational: reset() rebuilds the generator with its default 20
                                      (env_super.py:375), so 20 is what every episode uses */
    /* sorting_station (config.yml:12-18) */
    double   baseline_accuracy[4];
    double   boost;
    double   noise;                /* ctor noise_sorting (env_super.py:71) */
    int32_t  stage_capacity;
    /* pressing_station (config.yml:21-32) */
    int32_t  press_time[2];        /* <= 255 */
    int32_t  container_capacity;
    int32_t  bale_standard_size;   /* ctor balesize (env_super.py:87) */
    double   bale_remainder_threshold;
    double   quality_threshold[4];
    double   quality_threshold_r2[4]; /* python round(threshold, 2): purity of an EMPTY container
                                         (env_super.py:786-789) */
    /* rewards (config.yml:35-59) */
    double   purity_threshold_theta;
    double   tanh_temperature;
    double   overflow_penalty_catastrophic;
    double   overflow_penalty_severe;
    double   overflow_penalty_mild;
    double   bale_efficiency_factor;
    double   max_state_reward;
    double   overflow_termination_penalty;
    /* seasonal patterns 1 and 2, order A,B,C,D (utils/input_generator.py:17-20) */
    double   pattern_ratio[2][4];
    /* mse_rollout kernel choice: 0 = by size (while the batch fits the chip in one round of 256-env workgroups,
       n <= 256 x CUs - or fills most of a second one, 320 x CUs < n <= 512 x CUs -, the multi-role kernels:
       dynamics + observer waves, plus RNG waves when the config's draws per step fit the ring; otherwise one lane
       per env), 1 = dynamics + observer waves, 2 = one lane per env, 3 = dynamics + observer + RNG waves.
       mse_rollout_policy reads the same field: up to 256 envs x CUs (f16x3 products, no in-loop sorting policy) it
       runs actor + critic + RNG waves per 64 envs (0, when the draws fit the ring), actor + critic waves (1, or 0 when
       they do not) or one wave per 32 envs doing everything (2); above that size 64-env waves whatever the value.
       Results are identical. */
    int32_t  rollout_pipeline;
    int32_t  reserved0;
} mse_config;

typedef struct mse_env mse_env; /* opaque handle: N envs on one device */

/* library */
int         mse_version(void);
const char *mse_last_error(void);
const char *mse_status_string(int status);

/* Fills *cfg with config.yml's values and the env classes' ctor defaults
 * (max_steps=50, noise 0.05, balesize 200: env_monolith.py:22-23). */
int mse_config_default(mse_config *cfg);

/* Replaces Env_*.__init__ (env_monolith.py:22-36, env_super.py:25-137) for n_envs instances on
 * HIP device `device_id`.  Allocates the state planes; the envs hold no valid episode until
 * mse_reset() with seeds has run once (mse_step before that fails with MSE_ERR_NOT_RESET). */
int mse_create(mse_env **out, const mse_config *cfg, int64_t n_envs, int device_id);
/* Same, for one shard of a larger job: env i of this handle is global env index_offset + i.
 * The global index only feeds the random-policy stream, so a sharded run samples the same
 * actions as a single-handle run (env-index sharding). */
int mse_create_indexed(mse_env **out, const mse_config *cfg, int64_t n_envs, int device_id, int64_t index_offset);
int mse_destroy(mse_env *env);

int64_t mse_num_envs(const mse_env *env);
int     mse_obs_dim(const mse_env *env);      /* 13 / 16 / 29: observation_space (env_1_sort.py:71, env_2_press.py:62, env_monolith.py:72) */
int     mse_num_actions(const mse_env *env);  /* 2 / 11 / 22: action_space      (env_1_sort.py:72, env_2_press.py:64, env_monolith.py:79) */

/* Replaces Env_*.reset(seed=...) (env_super.py:365-420 and the variants' overrides
 * env_1_sort.py:81-85, env_2_press.py:73-75, env_monolith.py:91-93).
 *   seeds_dev  u64[N] or NULL.  Given: reset(seed=seeds[i]) - re-seeds the env's streams at
 *              seed+3/+4/+99 and the generator at seed, all on the device (NumPy SeedSequence +
 *              PCG64 restated).  NULL: reset(seed=None) - streams continue; the generator's
 *              pattern order follows the build's deterministic rule (DESIGN.md "unseeded reset").
 *   which_dev  u8[N] or NULL: only envs with which[i] != 0 are reset (NULL = all).
 *   obs_out    f32[N, D] or NULL;  mask_out u8[N, A] or NULL  (rows of envs not reset are
 *              rewritten with their current observation / mask). */
int mse_reset(mse_env *env, const uint64_t *seeds_dev, const uint8_t *which_dev,
              float *obs_out, uint8_t *mask_out, void *stream);

/* Replaces Env_*.step(action, use_action_masking, check_overflow)
 * (env_1_sort.py:97-154, env_2_press.py:88-165, env_monolith.py:109-284) for all N envs.
 *   action_dev     i32[N]: sort: mode 0|1; press: 0..10; mono: 0..21 (mode*11 + press action).
 *                  Out-of-range values are counted (mse_error_count) and treated as action 0.
 *   sort_mode_dev  i32[N] or NULL, Env_2 only: the sorting agent's decision
 *                  (env_2_press.py:101-104); NULL = the rule-based fallback sorting_rules()
 *                  (env_super.py:469-482).
 *   obs_out        f32[N, D]    next observation (after auto-reset: the reset observation)
 *   reward_out     f32[N]       or NULL
 *   reward64_out   f64[N]       or NULL (the reference returns a python float = f64)
 *   done_out       u8[N]        terminated flag (truncated is always False in the reference)
 *   mask_out       u8[N, A]     or NULL: action_masks() of the state the NEXT action sees
 *   terminal_obs_out f32[N, D]  or NULL: with auto_reset, the last observation of a finished
 *                  episode (rows of envs that did not finish are left untouched). */
int mse_step(mse_env *env, const int32_t *action_dev, const int32_t *sort_mode_dev, uint32_t flags,
             float *obs_out, float *reward_out, double *reward64_out, uint8_t *done_out,
             uint8_t *mask_out, float *terminal_obs_out, void *stream);

/* Replaces Env_*.action_masks() (env_monolith.py:81-85 -> env_super.py:887-898,
 * env_2_press.py:66-67 -> env_super.py:869-885, env_1_sort.py:74-76). mask_out u8[N, A]. */
int mse_action_masks(mse_env *env, uint8_t *mask_out, void *stream);

/* The observation Env_2_Pressing.step hands its sorting agent (env_2_press.py:95-104: get_sort_obs() after the
 * coming step's flow update, before the sensor setting), for every env: obs13_out f32[N, 13].  A preview - the
 * state is not changed; feed the agent's decisions to the next mse_step / mse_rollout as sort_mode_dev.
 * Defined for every env kind (the sorting view of the state one flow update ahead). */
int mse_sort_agent_obs(mse_env *env, float *obs13_out, void *stream);
/* The same preview for a pressing agent: get_press_obs() after the coming step's flow update, which is what
 * Env_3_Monolith.step(mode='model') hands its press_agent (env_monolith.py:198-210).  obs16_out f32[N, 16]. */
int mse_press_agent_obs(mse_env *env, float *obs16_out, void *stream);
/* What Env_3_Monolith.step hands a stored mono_agent (env_monolith.py:144-150: get_obs() after the step's flow update =
 * get_sort_obs() || get_press_obs()): obs29_out f32[N, 29], [:, :13] the bits of mse_sort_agent_obs and [:, 13:] the bits
 * of mse_press_agent_obs of the same state, from one kernel over one flow-updated copy of the env.  Env_3 only
 * (MSE_ERR_INVALID_ARGUMENT otherwise); general generator mode is served as the two previews serve it.  A preview: nothing
 * is stored to the state. */
int mse_mono_agent_obs(mse_env *env, float *obs29_out, void *stream);

/* K fused steps with the on-device random policy (the reference's mode='random', env_monolith.py:152-164, with a
 * counter-based policy stream instead of the global np.random): uniform over the set bits of action_masks(), or -
 * with MSE_STEP_UNMASKED - over the whole action space, the step sanitising what it gets (add MSE_STEP_SANITIZE_LATE
 * on Env_3 for the reference's exact mode='random' sequencing).  State stays in registers across the K steps.
 * Outputs are step-major: actions_out i32[K,N], obs_out f32[K,N,D], reward_out f32[K,N],
 * done_out u8[K,N], mask_out u8[K,N,A]; any of them may be NULL.  Needs auto_reset=1.
 *   sort_mode_dev i32[N] or NULL: Env_2's frozen per-env sorting decision (NULL = rule). */
int mse_rollout(mse_env *env, int32_t k_steps, uint64_t policy_seed, const int32_t *sort_mode_dev,
                uint32_t flags, int32_t *actions_out, float *obs_out, float *reward_out,
                uint8_t *done_out, uint8_t *mask_out, void *stream);

/* Samples one masked-uniform action per env from the CURRENT state (same policy stream as
 * mse_rollout); action_out i32[N]. */
int mse_sample_actions(mse_env *env, uint64_t policy_seed, int32_t *action_out, void *stream);

/* The reference's rule-based action per env for the CURRENT state (env_monolith.py:166-184). */
int mse_rule_actions(mse_env *env, int32_t *action_out, void *stream);

/* State export / import in a fixed record layout (tests, checkpoint/resume, dashboard trace):
 *   ints  i64[N, MSE_SNAP_INTS]  (column map: MSE_SNAP_* below)
 *   dbls  f64[N, 4]              accuracy_belt
 *   rng   u64[N, 30]             {state_hi,state_lo,inc_hi,inc_lo,has_uint32,uinteger} x
 *                                {rng (seed+99), rng_noise (seed+4), rng_pressing (seed+3), rng_sorting (seed+2),
 *                                 the input generator's private default_rng(seed) (utils/input_generator.py:28; it only
 *                                 advances in general generator mode, i.e. when floor(ratio * batch) leaves units over)}
 * Replaces reading/writing the attributes of Env_Super (env_super.py:52-137). */
#define MSE_SNAP_INTS 71
#define MSE_SNAP_RNG_WORDS 30
int mse_get_state(mse_env *env, int64_t *ints_out, double *dbls_out, uint64_t *rng_out, void *stream);
int mse_set_state(mse_env *env, const int64_t *ints_in, const double *dbls_in, const uint64_t *rng_in, void *stream);

/* Env_3_Monolith.step(action=None, mode='model') with no agents assigned (env_monolith.py:186-221): per env the
 * sorting decision rng_sorting.choice([0, 1]) (:195) and the press action rng_pressing.choice(flatnonzero(
 * press_action_masks())) (:214-217), or rng_pressing.choice(11) with MSE_STEP_UNMASKED (:219), NumPy-exact (buffered
 * Lemire draws on the env's own PCG64 streams, which advance).  action_out i32[N] = mode * 11 + press action; step
 * it with mse_step and flags WITHOUT MSE_STEP_UNMASKED: the reference applies a mode='model' action through
 * press_action_rules without sanitising it (env_monolith.py:254-257).  flags: MSE_STEP_UNMASKED,
 * MSE_MODEL_NO_SORT_DRAW, MSE_MODEL_NO_PRESS_DRAW (an assigned agent decides that part).  Env_3 handles only. */
int mse_model_actions(mse_env *env, uint32_t flags, int32_t *action_out, void *stream);

/* K fused steps of Env_3_Monolith.step(action=None, mode='model') (env_monolith.py:186-221), agents assigned or not:
 * per step k and env i the sorting part is the argmax of sort_agent's actor (13 -> 2) on get_sort_obs() after the
 * step's flow update (what mse_sort_agent_obs previews), or - sort_agent NULL - rng_sorting.choice([0, 1]); the press
 * part the argmax of press_agent's actor (16 -> 11) on get_press_obs() after the flow update (mse_press_agent_obs),
 * with MSE_MODEL_PRESS_AGENT_MASKED over press_action_masks() (illegal actions at logit -1e8, as mse_policy_forward),
 * or - press_agent NULL - the draw of mse_model_actions (rng_pressing.choice(flatnonzero(press_action_masks())), or
 * choice(11) with MSE_STEP_UNMASKED).  Argmax ties go to the first maximum (mse_policy_forward, deterministic=1).  The
 * flat action mode * 11 + press is then stepped as mse_step steps it without MSE_STEP_UNMASKED (no sanitising,
 * env_monolith.py:254-257), MSE_STEP_CHECK_OVERFLOW honoured, auto-reset on termination.  Bit-identical to K rounds of
 * mse_sort_agent_obs / mse_press_agent_obs, mse_policy_forward(deterministic=1), mse_model_actions(MSE_MODEL_NO_*_DRAW
 * for the agents' parts) and mse_step: rng_sorting / rng_pressing advance as there, the policy step counter by K.
 * Outputs are step-major, any may be NULL: actions_out i32[K,N], obs_out f32[K,N,29] (after any auto-reset),
 * reward_out f32[K,N], done_out u8[K,N], mask_out u8[K,N,22] (the post-step rows, as mse_rollout), and the agents'
 * views before the decision, written whether or not that agent is present: sort_obs_out f32[K,N,13],
 * press_obs_out f32[K,N,16].  flags: MSE_STEP_UNMASKED (use_action_masking=False: the fallback press draw),
 * MSE_STEP_CHECK_OVERFLOW, MSE_MODEL_PRESS_AGENT_MASKED.  Env_3 handles with auto_reset=1; agents in the f16x3 form
 * (mse_policy_set_precision) on the env's device; not with literal_choice or in general generator mode
 * (MSE_ERR_UNSUPPORTED_CONFIG: alternate the calls above instead). */
#define MSE_MODEL_PRESS_AGENT_MASKED 64u /* the press agent is maskable and masking is on: argmax over press_action_masks() */
struct mse_policy; /* a packed policy: mse_policy_create below */
int mse_rollout_model(mse_env *env, struct mse_policy *sort_agent, struct mse_policy *press_agent, int32_t k_steps, uint32_t flags,
                      int32_t *actions_out, float *obs_out, float *reward_out, uint8_t *done_out, uint8_t *mask_out,
                      float *sort_obs_out, float *press_obs_out, void *stream);

/* Opt-in trace of ONE env: what the reference appends per step to its Python ledgers - reward_data
 * (env_super.py:402-408, 928-946), press_actions_per_timestep (:631-637, 730-736; env_monolith.py:136;
 * env_2_press.py:131) and the press_bale calls behind bale_count (:661-687) - which the dashboard reads
 * (utils/plotting.py:32-48).  Between mse_trace_begin and mse_trace_end every mse_step appends one record
 * f64[MSE_TRACE_COLS] for env `env_index` to records_dev (caller-owned device memory, `capacity` records; a step
 * beyond the capacity fails with MSE_ERR_INVALID_ARGUMENT; mse_rollout is refused while a trace is attached).
 * The values are those of the state _log_step_data sees: after the step, before any auto-reset.  Unbounded
 * per-env ledgers are not kept for all N lanes (DESIGN.md "Not carried per lane"); this is the one-env form. */
#define MSE_TRACE_COLS       40
#define MSE_TRACE_ACTION      0 /* the flat action the step applied (Env_1: the sensor mode)                     */
#define MSE_TRACE_R_SORT      1 /* _log_step_data(r_sort, r_press): env_1_sort.py:141,151; env_2_press.py:152,162; */
#define MSE_TRACE_R_PRESS     2 /*                                  env_monolith.py:271,282                         */
#define MSE_TRACE_SETTING     3 /* sensor_current_setting                                                         */
#define MSE_TRACE_BELT        4 /* [4] current_material_belt (Belt_Occupancy, Belt_Proportions derive from it)    */
#define MSE_TRACE_CONT_TRUE   8 /* [4] container A..D true                                                        */
#define MSE_TRACE_CONT_FALSE 12 /* [4] container A..D false                                                       */
#define MSE_TRACE_CONT_E     16
#define MSE_TRACE_N_LOG      17 /* entries appended to press_actions_per_timestep this step (0..2)                */
#define MSE_TRACE_LOG        18 /* [2][2] {code, material}: code 0 no-op, 1|2 press started, 111|222 busy/invalid */
#define MSE_TRACE_N_BALE     22 /* press_bale calls this step (0..2)                                              */
#define MSE_TRACE_BALE       23 /* [2][3] {material 0..4, amount n, int(q*100)} in the reference's call order      */
#define MSE_TRACE_DONE       29
#define MSE_TRACE_STEP       30 /* current_step after the step                                                    */
#define MSE_TRACE_INTERNAL   31 /* Env_1: the press action sampled inside the env (env_1_sort.py:125)             */
#define MSE_TRACE_REWARD     32 /* the step's reward (f64)                                                        */
#define MSE_TRACE_ACC_BELT   33 /* [4] accuracy_belt after the step (the next step's accuracy_sorter)             */
#define MSE_TRACE_OVERFLOW   37 /* check_overflow terminated the episode: 1 + index of the first material A..E whose
                                   level exceeds the capacity (detect_overflow, env_super.py:900-905: the reference's
                                   info["overflow_material"]), else 0                                                */
int mse_trace_begin(mse_env *env, int64_t env_index, double *records_dev, int64_t capacity);
int mse_trace_end(mse_env *env, int64_t *n_records_out);

/* The same trace for EVERY env: records_dev is f64[capacity, MSE_TRACE_COLS, N], one plane of N doubles per column per
 * step, so the store of one column by a wave is 64 consecutive doubles.  From the call on every mse_step stores the
 * record of every env into step slot n_records (the values and their moment are those of the one-env trace; columns 38
 * and 39 are not written), until mse_trace_end, which ends either kind of trace.  A step beyond `capacity` and any
 * mse_rollout* while the trace is attached are refused exactly as with mse_trace_begin; beginning either kind of
 * trace replaces the one attached.  The records are what mse_plant_scan (below) folds into per-episode rows. */
int mse_trace_begin_all(mse_env *env, double *records_dev, int64_t capacity);

/* The step counter t of the on-device policy stream (word = f(policy seed, global env index, t); every mse_step
 * advances it by 1, every mse_rollout by k_steps).  It is host-side handle state, not part of the state record:
 * a checkpoint that must reproduce an on-device-policy rollout saves it with mse_get_state's record and restores
 * it after mse_set_state. */
int mse_get_policy_step(const mse_env *env, uint64_t *t_out);
int mse_set_policy_step(mse_env *env, uint64_t t);

/* Number of out-of-range actions (mse_step) and of unreachable values handed to mse_set_state (stage vectors that
 * are no generator output, accuracies outside [clip(baseline [+ boost] - noise), 1]) seen so far; synchronises
 * the device. */
int mse_error_count(mse_env *env, uint64_t *count_out);

/* Algorithmic HBM bytes per env-step used for the roofline figure. */
int mse_algorithmic_bytes_per_step(const mse_env *env);

/* Build constant: a `choice` draw whose 32-bit fraction view f satisfies f + 160 < window (32-bit wrap-around: f below
 * window - 160, or within 160 of 2^32) is decided by the literal fp64 cdf instead of the exact integer comparison
 * (DESIGN.md "choice"; the derivation of the margin is in csrc/mse_device.h).  162 in the shipped library; the
 * test-only build libmse_hip_widetie.so reports 0x08000000. */
uint32_t mse_tie_window(void);

/* ---- the policy on the caller's side of step() -----------------------------------------------
 * Batched forward of the reference's actor-critic MLP (src/training.py:115: net_arch=dict(pi=[32,32], vf=[32,32]),
 * tanh; MaskableActorCriticPolicy) with masked categorical sampling, on the f32 matrix cores.
 * weights_host: mse_policy_num_weights(D, A) floats, torch.nn.Linear layout ([out, in] row-major), in this order:
 *   pi_w1[32*D] pi_b1[32] pi_w2[32*32] pi_b2[32] act_w[A*32] act_b[A]   (mlp_extractor.policy_net.0/.2, action_net)
 *   vf_w1[32*D] vf_b1[32] vf_w2[32*32] vf_b2[32] val_w[32]   val_b[1]   (mlp_extractor.value_net.0/.2, value_net)
 * mse_policy_forward: obs_dev f32[N, D]; mask_dev u8[N, A] or NULL (invalid actions get logit -1e8, as
 * sb3_contrib's MaskableCategorical); deterministic != 0: argmax, else inverse-cdf sampling with the engine's
 * counter-based stream (seed, global env index = index_offset + i, t).  Outputs (each may be NULL):
 * action i32[N], log-probability f32[N], value f32[N], masked logits f32[N, A]. */
typedef struct mse_policy mse_policy;
int64_t mse_policy_num_weights(int obs_dim, int n_actions);
int mse_policy_create(mse_policy **out, int obs_dim, int n_actions, const float *weights_host, int device_id);
int mse_policy_destroy(mse_policy *policy);
/* Arithmetic of the matrix products: 1 = exact f32 (v_mfma_f32_32x32x2_f32, an fmaf chain); 2 = "f16x3": every f32
 * operand split into two f16 parts carrying 22 bits, three f16 MFMAs per product with f32 accumulation (logits within
 * ~1e-6 of the exact form, 5x the matrix rate; needs every folded weight below 65 504); 0 = f16x3 when the weights
 * allow it, else f32 (the default).  mse_policy_precision reports which one is in effect (1 | 2). */
int mse_policy_set_precision(mse_policy *policy, int mode);
int mse_policy_precision(const mse_policy *policy);
int mse_policy_forward(mse_policy *policy, int64_t n, int64_t index_offset, const float *obs_dev, const uint8_t *mask_dev,
                       uint64_t seed, uint64_t t, int deterministic, int32_t *action_out, float *logp_out,
                       float *value_out, float *logits_out, void *stream);

/* ---- SURVEY 8f ranks 1 + 2 fused: K steps of policy forward + env transition in ONE launch -------------------------
 * The consumer loop of the reference's training (SB3's collect_rollouts inside model.learn, src/training.py:191, with
 * the policy of src/training.py:115-131): per step k and env i
 *     observation / action mask / episode-start flag of the state the action is taken from   (obs_out f32[K,N,D],
 *                                                       mask_out u8[K,N,A], episode_start_out u8[K,N])
 *     action, log-probability, value = policy(observation, mask)   (sampled with the engine's stream at step counter
 *                                                       t + k, or argmax with deterministic != 0: actions_out i32[K,N],
 *                                                       logp_out f32[K,N], value_out f32[K,N])
 *     reward of the transition under that action, auto-reset on termination                  (reward_out f32[K,N])
 * i.e. the rows of SB3's MaskableRolloutBuffer, plus last_value_out f32[N] (the value of the state after the last
 * step, the bootstrap of compute_returns_and_advantage) and last_done_out u8[N].  Any output may be NULL.  The
 * observation never leaves the wave's registers between env_step and the policy's MFMA chain.  Bit-identical to
 * alternating mse_policy_forward and mse_step with the same seed and step counter.
 *   sort_policy   Env_2 only, or NULL: a second network (13 -> 2) standing where the reference expects the pre-trained
 *                 sorting agent (env_2_press.py:101-104: sort_agent.predict(get_sort_obs() after the step's flow update,
 *                 deterministic=True)): its actor is evaluated inside the loop, argmax (f16x3 form of both networks);
 *   sort_mode_dev i32[N] or NULL: else Env_2's per-env sorting decision (both NULL = sorting_rules()).
 *   flags: MSE_STEP_UNMASKED, MSE_STEP_CHECK_OVERFLOW.  Needs auto_reset=1; advances the policy step counter by K. */
int mse_rollout_policy(mse_env *env, mse_policy *policy, mse_policy *sort_policy, int32_t k_steps, uint64_t seed, int deterministic,
                       const int32_t *sort_mode_dev, uint32_t flags, float *obs_out, uint8_t *mask_out,
                       int32_t *actions_out, float *logp_out, float *value_out, float *reward_out,
                       uint8_t *episode_start_out, float *last_value_out, uint8_t *last_done_out, void *stream);

/* ---- The modular pair trained in the env it is deployed in: K steps of Env_3_Monolith in ONE launch with the sorting
 * agent (13 -> 2) and the pressing agent (16 -> 11) acting side by side, each recorded as its own learner needs it.
 * Per step k and env i:
 *   1. previews: a copy of the env takes the step's flow update; sort_obs = get_sort_obs() and press_obs =
 *      get_press_obs() of the copy (mse_sort_agent_obs / mse_press_agent_obs); press_action_masks() is taken from the
 *      state the decision is made in;
 *   2. sorting agent: action, log-probability, value = policy(sort_obs), every action legal, drawn with the word of
 *      (sort_seed, global env index, t + k);
 *   3. pressing agent: the same on press_obs with the word of (press_seed, global env index, t + k), over
 *      press_action_masks() with MSE_MODEL_PRESS_AGENT_MASKED, else over all 11 actions;
 *   4. MSE_MODULAR_SORT_DETERMINISTIC / MSE_MODULAR_PRESS_DETERMINISTIC: that agent takes the argmax
 *      (predict(deterministic=True)); its log-probability and value are written all the same;
 *   5. the flat action 11 sort + press is stepped as mse_step steps it without MSE_STEP_UNMASKED (no sanitising,
 *      env_monolith.py:254-257), MSE_STEP_CHECK_OVERFLOW honoured, auto-reset on termination.
 * Outputs (mse_modular_buffers, step-major, any pointer may be NULL): the rows the decisions were taken from -
 * sort_obs f32[K,N,13], press_obs f32[K,N,16], press_masks u8[K,N,11] (always press_action_masks(), whatever the
 * agent was shown), episode_starts u8[K,N] -, sort_actions / press_actions i32[K,N], sort_log_probs / press_log_probs /
 * sort_values / press_values f32[K,N], rewards f32[K,N] (the step's reward) and its two parts rewards_sort /
 * rewards_press f32[K,N] (the arguments of _log_step_data, env_monolith.py:271,282: reward / 2 each on an overflow
 * termination), and after the last step sort_last_values / press_last_values f32[N] (each critic on its preview of the
 * state the rollout ends in) and last_dones u8[N].
 * Bit-identical to K rounds of mse_sort_agent_obs, mse_press_agent_obs, two mse_policy_forward calls (the seeds above,
 * t = the handle's policy step counter, index_offset = the env's) and mse_step: the same actions, log-probabilities,
 * values, observations, rewards, flags and final state.  Advances the policy step counter by K; the env's rng_sorting /
 * rng_pressing streams are neither read nor written (there are no fallback draws).
 * Refusals: MSE_ERR_INVALID_ARGUMENT - a NULL agent, agent dimensions other than 13 -> 2 / 16 -> 11, sort_seed ==
 * press_seed (the two agents would draw from one word), k_steps < 1, a flag other than the four above
 * (MSE_STEP_UNMASKED included), a handle that is not Env_3 or lacks auto_reset=1, an attached trace;
 * MSE_ERR_UNSUPPORTED_CONFIG - an agent not in the f16x3 form, literal_choice, general generator mode, tables that do
 * not fit the kernel's LDS image. */
#define MSE_MODULAR_SORT_DETERMINISTIC  128u
#define MSE_MODULAR_PRESS_DETERMINISTIC 256u
typedef struct mse_modular_buffers {
    uint32_t struct_size; /* = sizeof(mse_modular_buffers); ABI check */
    uint32_t reserved0;
    float   *sort_obs;
    float   *press_obs;
    uint8_t *press_masks;
    uint8_t *episode_starts;
    int32_t *sort_actions;
    int32_t *press_actions;
    float   *sort_log_probs;
    float   *press_log_probs;
    float   *sort_values;
    float   *press_values;
    float   *rewards;
    float   *rewards_sort;
    float   *rewards_press;
    float   *sort_last_values;
    float   *press_last_values;
    uint8_t *last_dones;
} mse_modular_buffers;
int mse_rollout_modular(mse_env *env, mse_policy *sort_agent, mse_policy *press_agent, int32_t k_steps, uint64_t sort_seed,
                        uint64_t press_seed, uint32_t flags, const mse_modular_buffers *out, void *stream);
/* The status mse_rollout_modular would return for these arguments (MSE_OK or one of the refusals above, with its
 * message in mse_last_error), without launching anything or touching the handle: what a caller that alternates the
 * single calls itself asks first, so that it serves exactly the handles the kernel serves. */
int mse_rollout_modular_check(mse_env *env, mse_policy *sort_agent, mse_policy *press_agent, int32_t k_steps,
                              uint64_t sort_seed, uint64_t press_seed, uint32_t flags);

/* ---- mse_rollout_modular with the rule-based controller in the same launch: its label of every recorded state in the two
 * agents' halves, and the DAgger mixture of mse_rollout_demo deciding per env and step who steps.  Per step k and env i:
 *   1. mse_rollout_modular's steps 1-4, unchanged: previews, press_action_masks(), the rows, both agents' action,
 *      log-probability and value.  sort_actions / press_actions are the agents' own draws whoever steps, so they match
 *      the recorded log-probabilities;
 *   2. the label: the flat rule-based action of the state before the step, exactly what mse_rule_actions returns for it
 *      (mse_rollout_demo's label); no stream is read or advanced.  sort_expert_actions[k,i] = label / 11,
 *      press_expert_actions[k,i] = label % 11;
 *   3. who steps: mse_rollout_demo's step 4 with the word of (mix_seed, global env index, t + k) - the expert iff
 *      (w >> 8) < expert_threshold, an integer in [0, 2^24]; mse_demo_who_steps_host is the same rule on the host.  One
 *      decision covers both halves: the stepped flat action is the label, or 11 sort + press;
 *   4. stepped_actions i32[K,N] (that flat action), expert_stepped u8[K,N] (1: the label was stepped); the action is
 *      stepped as mse_step steps it without MSE_STEP_UNMASKED, MSE_STEP_CHECK_OVERFLOW honoured, auto-reset on termination;
 *   5. rewards, reward parts, bootstrap values, last_dones and the state write-back as in mse_rollout_modular.
 * Any pointer inside either struct may be NULL.  The flags are mse_rollout_modular's four.
 * CONTRACT: with expert_threshold = 0 every mse_modular_buffers output, the written-back state and the policy step counter
 * are bit-identical to mse_rollout_modular on the same handle.  For every threshold the env's rng_sorting / rng_pressing
 * planes are neither read nor written, and the policy step counter advances by K.
 * The shape is mse_rollout_modular's (both wave forms; no roles shape).
 * Refusals, in this order: mse_rollout_modular's, in its own order; expert_threshold > 2^24; mix_seed equal to sort_seed
 * or press_seed, whatever the threshold; out or labels NULL, or a struct_size mismatch (all MSE_ERR_INVALID_ARGUMENT).  A
 * refused call writes nothing and leaves the step counter unchanged. */
typedef struct mse_modular_label_buffers {
    uint32_t struct_size; /* = sizeof(mse_modular_label_buffers); ABI check */
    uint32_t reserved0;
    int32_t *sort_expert_actions;  /* i32[K,N] */
    int32_t *press_expert_actions; /* i32[K,N] */
    int32_t *stepped_actions;      /* i32[K,N], flat */
    uint8_t *expert_stepped;       /* u8[K,N] */
} mse_modular_label_buffers;
int mse_rollout_modular_labelled(mse_env *env, mse_policy *sort_agent, mse_policy *press_agent, int32_t k_steps,
                                 uint64_t sort_seed, uint64_t press_seed, uint64_t mix_seed, uint32_t expert_threshold,
                                 uint32_t flags, const mse_modular_buffers *out, const mse_modular_label_buffers *labels,
                                 void *stream);
/* The status mse_rollout_modular_labelled would return for these arguments, its checks on out / labels left out; no launch */
int mse_rollout_modular_labelled_check(mse_env *env, mse_policy *sort_agent, mse_policy *press_agent, int32_t k_steps,
                                       uint64_t sort_seed, uint64_t press_seed, uint64_t mix_seed, uint32_t expert_threshold,
                                       uint32_t flags);

/* ---- Demonstrations on the states a student visits (DAgger): K steps in ONE launch in which the rule-based controller
 * labels every visited state and, per env and step, either its action or a student policy's is stepped.
 * Per step k and env i, in this order:
 *   1. the rows the decision is taken from: observations f32[K,N,D], action_masks u8[K,N,A] (action_masks() of that
 *      state) and episode_starts u8[K,N] (current_step == 0);
 *   2. the label: the flat rule-based action for that state, exactly what mse_rule_actions returns for it; it consumes
 *      no draw from any stream                                                                       (labels i32[K,N]);
 *   3. the student's action = policy(observation) over the mask bits, drawn with the word of (seed, global env index,
 *      t + k); with MSE_DEMO_ACTOR_DETERMINISTIC the argmax;
 *   4. who steps: w = the policy stream's word of (mix_seed, global env index, t + k) (csrc/mse_policy_stream.h: the
 *      word at t + k under the key of mix_seed and the index); the expert's action is
 *      stepped iff (w >> 8) < expert_threshold, else the student's.  expert_threshold is an integer in [0, 2^24]:
 *      0 = the student always steps, 2^24 = the expert always steps; integers are compared, nothing is rounded
 *      (mse_demo_who_steps_host is the same rule on the host);
 *   5. that action is stepped as mse_step steps it without MSE_STEP_UNMASKED, MSE_STEP_CHECK_OVERFLOW honoured,
 *      auto-reset on termination; Env_2's sorting decision is sorting_rules();
 *   6. stepped_actions i32[K,N], expert_stepped u8[K,N] (1: the expert's action was stepped), rewards f32[K,N], and
 *      after the last step last_dones u8[N].
 * actor == NULL: there is no student (no network, no matrix-core work); the expert always steps, expert_stepped is all
 * ones, and seed / mix_seed / expert_threshold select nothing (the threshold is still range-checked).
 * Any output pointer may be NULL.  The state is written back once; the policy step counter advances by K.  Serves the
 * three env kinds with a policy of the env's own dimensions (13 -> 2, 16 -> 11, 29 -> 22) in both precision forms (the
 * exact-f32 form in the 64-env shape, as in mse_rollout_policy's plain kernel).
 * Bit-identical to K rounds of: read the observation and mask; mse_rule_actions; mse_policy_forward(seed, t = the
 * handle's policy step counter, index_offset = the env's); the who-steps rule above; mse_step - in actions, labels,
 * rows, rewards, flags, final mse_get_state record and step counter.
 * Refusals, made before any device call, in this order: MSE_ERR_INVALID_ARGUMENT - a NULL env or out; a wrong
 * struct_size; k_steps < 1; actor dimensions other than the env's, or an actor on another device; expert_threshold >
 * 2^24; mix_seed == seed with a non-NULL actor (who steps and what the student draws would come from one word); a flag
 * other than MSE_STEP_CHECK_OVERFLOW / MSE_DEMO_ACTOR_DETERMINISTIC (MSE_STEP_UNMASKED included); a handle without
 * auto_reset=1 or not yet reset; an attached trace; observations / action_masks not 16-byte aligned.
 * MSE_ERR_UNSUPPORTED_CONFIG - literal_choice, general generator mode, tables that do not fit the kernel's LDS image.
 * Every one of them, this entry point's own statuses: a handle not yet reset and a misaligned row buffer are invalid
 * arguments here. */
#define MSE_DEMO_ACTOR_DETERMINISTIC 512u
typedef struct mse_demo_buffers {
    uint32_t struct_size; /* = sizeof(mse_demo_buffers); ABI check */
    uint32_t reserved0;
    float   *observations;
    uint8_t *action_masks;
    uint8_t *episode_starts;
    int32_t *labels;
    int32_t *stepped_actions;
    uint8_t *expert_stepped;
    float   *rewards;
    uint8_t *last_dones;
} mse_demo_buffers;
int mse_rollout_demo(mse_env *env, mse_policy *actor, int32_t k_steps, uint64_t seed, uint64_t mix_seed,
                     uint32_t expert_threshold, uint32_t flags, const mse_demo_buffers *out, void *stream);
/* mse_rollout_policy with the rule-based controller's label of every recorded row, in the same launch: the rollout that PPO
 * with an imitation term trains on (mse_ppo_bc_loss_grad).  The arguments are mse_rollout_policy's without the sorting policy,
 * then
 *   expert_actions_out  i32[K, N]: per step, what mse_rule_actions returns for the state the recorded row shows (the state
 *                       before the step) - mse_rollout_demo's label expression; no stream is read or advanced for it
 * Every other output, the written-back state and the policy step counter are bit-identical to mse_rollout_policy with
 * sort_policy = NULL on the same handle.  Two limits: there is no in-loop sorting policy (alternate mse_policy_forward,
 * mse_rule_actions and mse_step for that: Python's PolicyRolloutCollector(sort_policy=, expert_labels=True)), and there is no
 * roles shape - the plain kernel (one wave owns 32 or 64 envs, one network, f16x3 in either wave shape, exact f32 in the
 * 64-env shape) runs at every size, as in mse_rollout_demo, whatever rollout_pipeline says.
 * Refusals: mse_rollout_policy's, in its order (NULL env / policy, before reset, k_steps < 1, auto_reset = 0, an attached
 * trace, unknown flags, mismatched dimensions or devices, unaligned obs_out / mask_out, a config off the integer path, tables
 * that do not fit the kernel's LDS image), then expert_actions_out == NULL (MSE_ERR_INVALID_ARGUMENT).  Nothing is written
 * and the step counter stays when a call is refused. */
int mse_rollout_policy_labelled(mse_env *env, mse_policy *policy, int32_t k_steps, uint64_t seed, int deterministic,
                                const int32_t *sort_mode_dev, uint32_t flags, float *obs_out, uint8_t *mask_out,
                                int32_t *actions_out, float *logp_out, float *value_out, float *reward_out,
                                uint8_t *episode_start_out, float *last_value_out, uint8_t *last_done_out,
                                int32_t *expert_actions_out, void *stream);
/* The status mse_rollout_policy_labelled would return for these arguments, its checks on the outputs left out; no launch */
int mse_rollout_policy_labelled_check(mse_env *env, mse_policy *policy, int32_t k_steps, uint64_t seed, int deterministic,
                                      const int32_t *sort_mode_dev, uint32_t flags);

/* The status mse_rollout_demo would return for these arguments, its checks on `out` left out (MSE_OK or one of the
 * refusals above, with its message in mse_last_error), without launching anything or touching the handle. */
int mse_rollout_demo_check(mse_env *env, mse_policy *actor, int32_t k_steps, uint64_t seed, uint64_t mix_seed,
                           uint32_t expert_threshold, uint32_t flags);
/* Step 4 on the host, no device needed: out[j] = 1 iff the expert steps env index_offset + j at step counter t. */
int mse_demo_who_steps_host(int64_t n, int64_t index_offset, uint64_t mix_seed, uint64_t t, uint32_t expert_threshold,
                            uint8_t *out);

/* ---- The mono policy on the in-step view (env_monolith.py:144-150, a stored mono_agent): K steps of Env_3 in ONE launch
 * with one 29 -> 22 network that is shown, like the modular agents, the observation AFTER the step's flow update, with the
 * rule-based controller's label and mse_rollout_demo's mixture in the same launch.  Per step k and env i:
 *   1. the preview: a copy of the env takes the step's flow update; observations[k,i,:] f32[K,N,29] is get_sort_obs() ||
 *      get_press_obs() of the copy (the container purities come from the current state, as in mse_rollout_modular) - the
 *      row mse_mono_agent_obs returns; action_masks[k,i,:] u8[K,N,22] is action_masks() of the state the decision is
 *      taken in; episode_starts[k,i] is current_step == 0;
 *   2. the policy: actions i32[K,N], log_probs f32[K,N], values f32[K,N] = policy(row) over the mask bits, drawn with the
 *      word of (seed, index_offset + i, t + k); with MSE_PREVIEW_DETERMINISTIC the argmax;
 *   3. the label: expert_actions i32[K,N], exactly what mse_rule_actions returns for the state; no stream is read;
 *   4. who steps: mse_rollout_demo's step 4 with the word of (mix_seed, index_offset + i, t + k) against expert_threshold
 *      in [0, 2^24] (mse_demo_who_steps_host on the host).  stepped_actions i32[K,N] is the flat action that was stepped,
 *      expert_stepped u8[K,N] marks where it was the label; actions stays the policy's own draw whoever steps;
 *   5. the step: as mse_step steps the action without MSE_STEP_UNMASKED (Path 2 predicts under the mask and applies the
 *      action unsanitised, :148, :254-259), MSE_STEP_CHECK_OVERFLOW honoured, auto-reset on termination; rewards f32[K,N].
 * After the last step: last_values f32[N] is the critic on the preview of the final state, last_dones u8[N]; the state is
 * written back once and the policy step counter advances by K.  rng_sorting / rng_pressing are neither read nor written.
 * Every pointer in the struct may be NULL.
 * CONTRACTS: (a) bit-identical to K rounds of mse_mono_agent_obs, mse_action_masks, mse_rule_actions, mse_policy_forward
 * (seed, t = the handle's policy step counter, index_offset = the env's), the who-steps rule on the host and mse_step - in
 * every buffer, the final mse_get_state record and the step counter.  (b) With expert_threshold = 0 every non-label
 * output, the state and the counter hold the same bits whether or not expert_actions / stepped_actions / expert_stepped
 * are given.  (c) With expert_threshold = 2^24, rewards, stepped_actions and the final mse_get_state record equal those of
 * mse_rollout with MSE_ROLLOUT_RULE_BASED on a twin handle.
 * Shape: mse_rollout_policy's plain kernel with one network at every size - 32-env waves up to 256 x CUs envs in the f16x3
 * form, 64-env waves beyond, the exact-f32 form in the 64-env shape.  There is no roles shape, whatever rollout_pipeline
 * says (as mse_rollout_demo and mse_rollout_policy_labelled).
 * Refusals, made before any device call, in this order.  MSE_ERR_INVALID_ARGUMENT: a NULL env, policy or out; a wrong
 * struct_size; k_steps < 1; a handle that is not Env_3; policy dimensions other than 29 -> 22; a policy on another device;
 * expert_threshold > 2^24; mix_seed == seed; a flag other than MSE_STEP_CHECK_OVERFLOW / MSE_PREVIEW_DETERMINISTIC
 * (MSE_STEP_UNMASKED included); a handle without auto_reset = 1; a handle not yet reset; an attached trace; observations
 * / action_masks not 16-byte aligned.  MSE_ERR_UNSUPPORTED_CONFIG: literal_choice; general generator mode; tables that
 * do not fit the kernel's LDS image.  A refused call writes nothing and leaves the step counter unchanged. */
#define MSE_PREVIEW_DETERMINISTIC 1024u
typedef struct mse_preview_buffers {
    uint32_t struct_size; /* = sizeof(mse_preview_buffers); ABI check */
    uint32_t reserved0;
    float   *observations;    /* f32[K,N,29] */
    uint8_t *action_masks;    /* u8[K,N,22] */
    uint8_t *episode_starts;  /* u8[K,N] */
    int32_t *actions;         /* i32[K,N] */
    float   *log_probs;       /* f32[K,N] */
    float   *values;          /* f32[K,N] */
    float   *rewards;         /* f32[K,N] */
    int32_t *expert_actions;  /* i32[K,N] */
    int32_t *stepped_actions; /* i32[K,N] */
    uint8_t *expert_stepped;  /* u8[K,N] */
    float   *last_values;     /* f32[N] */
    uint8_t *last_dones;      /* u8[N] */
} mse_preview_buffers;
int mse_rollout_policy_preview(mse_env *env, mse_policy *policy, int32_t k_steps, uint64_t seed, uint64_t mix_seed,
                               uint32_t expert_threshold, uint32_t flags, const mse_preview_buffers *out, void *stream);
/* The status mse_rollout_policy_preview would return for these arguments, its checks on `out` left out; no launch */
int mse_rollout_policy_preview_check(mse_env *env, mse_policy *policy, int32_t k_steps, uint64_t seed, uint64_t mix_seed,
                                     uint32_t expert_threshold, uint32_t flags);

/* Replaces the device image of `policy` with new weights (same flat order as mse_policy_create), repacked by the same
 * host routine, including the f16 range check: a policy in the "auto" form moves to f32 when a folded weight leaves
 * f16's range and back when all fit again; one pinned to f16x3 refuses such weights (MSE_ERR_UNSUPPORTED_CONFIG, image
 * unchanged).  A BLOCKING host-to-device copy.  Ordering rule: no launch that reads this policy may be in flight on
 * any stream when it is called; launches enqueued afterwards see the new weights. */
int mse_policy_set_weights(mse_policy *policy, const float *weights_host);

/* The same replacement without the host: the repack runs on the device (csrc/mse_policy_pack.h specifies the image
 * completely and is the one arithmetic both packers run, float64 operations in the same order, so the device image
 * equals mse_policy_set_weights' byte for byte).  The handle also keeps a device copy of the flat weights its image was
 * packed from; mse_policy_create and mse_policy_set_weights keep it current too.
 *
 * mse_policy_set_weights_device: weights_dev f32[W] in device memory, flat order.  ONE launch of one workgroup on
 * `stream`; never synchronises, never allocates.  Ordering rule: launches enqueued on that stream afterwards see the new
 * weights; for every other stream the rule of mse_policy_set_weights stands.  The f16 range check happens inside the
 * launch: an "auto" or f32 policy always gets the new head and f32 operands, and the f16 operands when every folded
 * weight fits (their content is unspecified otherwise); a policy pinned to f16x3 whose new weights do not fit is left
 * untouched - image and flat copy - and a status word on the device says "refused".
 * mse_policy_sync: one small blocking read of that status word (behind the repack on its stream; nothing is read when
 * no device repack is outstanding).  It brings the host's view up to date, so an "auto" policy changes form exactly as
 * after mse_policy_set_weights, and returns MSE_ERR_UNSUPPORTED_CONFIG for a refused pinned policy.  UNTIL IT IS CALLED,
 * launches use the form last known: call it before the next launch whenever the new weights may cross f16's range.
 * mse_policy_pack_host / mse_policy_image_floats: the host twin, which needs no device: image_out
 * f32[mse_policy_image_floats()], *f16_ok_out = every folded weight is below 65 504 (the image's f16 section is specified
 * only then).  Dimensions outside 1..32: MSE_ERR_UNSUPPORTED_CONFIG.
 * mse_policy_read_image: a blocking copy of the device image into image_out_host (same size), for tests and debugging.
 * mse_policy_get_weights: a blocking copy of the handle's flat weights into out_host f32[W]. */
int mse_policy_set_weights_device(mse_policy *policy, const float *weights_dev, void *stream);
int mse_policy_sync(mse_policy *policy);
int64_t mse_policy_image_floats(void);
int mse_policy_pack_host(int obs_dim, int n_actions, const float *weights_host, float *image_out, int32_t *f16_ok_out);
int mse_policy_read_image(mse_policy *policy, float *image_out_host);
int mse_policy_get_weights(mse_policy *policy, float *out_host);

/* ---- The learner's half of PPO (SB3's model.learn -> MaskablePPO.train, src/training.py:191) ---------------------------
 * All buffers are caller-owned device memory, all work goes to `stream`, nothing allocates or synchronises, and the
 * arguments are checked before any device call.
 *
 * RolloutBuffer.compute_returns_and_advantage over step-major [K, N] arrays (the reference never truncates an episode,
 * so there is no terminal-value bootstrap):  backwards over k,  nnt = 1 - episode_starts[k + 1]  (1 - last_dones at
 * k = K - 1),  delta = r + gamma * next_v * nnt - v,  gae = delta + gamma * lambda * nnt * gae,  returns = advantages +
 * values.  float32 with every operation rounded separately in exactly that order (gamma and gamma * lambda rounded to
 * f32 once): bit-identical to numpy's evaluation of SB3's loop. */
int mse_gae(int32_t k_steps, int64_t n, const float *rewards, const float *values, const uint8_t *episode_starts,
            const float *last_values, const uint8_t *last_dones, double gamma, double gae_lambda, float *advantages_out,
            float *returns_out, void *stream);

/* What MaskablePPO.train computes for one minibatch (`rollout_data`), and the gradient of its loss.
 *   weights_dev  f32[W], W = mse_policy_num_weights(D, A), in the FLAT order documented above (not the packed image)
 *   rows_dev     i64[batch] or NULL: the minibatch's rows out of the n_rows = K * N flattened rollout rows
 *                (NULL = rows 0 .. batch - 1; an index outside [0, n_rows) is clamped)
 *   obs f32[n_rows, D], mask u8[n_rows, A] or NULL, actions i32[n_rows], old_logp / advantages / returns f32[n_rows]
 * Per minibatch: advantages normalised as (a - mean) / (std + 1e-8) with the unbiased std (normalize_advantage != 0 and
 * batch > 1); both 2 x 32 tanh MLPs forward, illegal actions at logit -1e8; ratio = exp(logp - old_logp);
 * policy_loss = -mean(min(adv ratio, adv clamp(ratio, 1 - clip, 1 + clip))); value_loss = mean((returns - value)^2);
 * entropy_loss = -mean(entropy over the legal actions); loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss.
 *   grad_out     f32[W]: d loss / d weights, flat order
 *   stats_out    f32[8]: loss, policy_loss, value_loss, entropy_loss, approx_kl = mean((ratio - 1) - log ratio),
 *                clip_fraction, and the advantage mean and std that were used (0 and 1 when not normalised)
 *   workspace    mse_ppo_workspace_bytes(D, A) bytes, 16-byte aligned; contents need not survive between calls
 * Three launches; sums are formed in a fixed order without atomics, so equal inputs give bit-equal outputs.
 * Grid rule of the gradient launch: a workgroup takes 128 minibatch rows per pass (two tiles of 64) and writes one slab;
 * there are min(ceil(batch / 128), 2 * CUs, 512) workgroups, so past 128 * min(2 * CUs, 512) rows a workgroup makes a
 * second pass. */
typedef struct mse_ppo_params {
    uint32_t struct_size; /* = sizeof(mse_ppo_params) */
    float    clip_range;
    float    ent_coef;
    float    vf_coef;
    int32_t  normalize_advantage;
} mse_ppo_params;
int64_t mse_ppo_workspace_bytes(int obs_dim, int n_actions); /* 0 for dimensions outside 1..32; needs no device */
int mse_ppo_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev, int64_t batch,
                      const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                      const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                      float *stats_out, void *workspace, void *stream);

/* torch.nn.utils.clip_grad_norm_ (coef = min(1, max_grad_norm / (norm + 1e-6)); max_grad_norm <= 0: no clipping) followed
 * by torch.optim.Adam without weight decay or amsgrad, in place on weights / m / v (f32[n_weights], zero m and v before
 * the first step); `step` counts from 1.  grad is not modified.  grad_norm_out f32[1] or NULL: the norm before clipping.
 * One workgroup (a policy has at most 4 791 weights). */
int mse_ppo_adam_step(int64_t n_weights, float *weights, const float *grad, float *m, float *v, int64_t step, double lr,
                      double beta1, double beta2, double eps, double max_grad_norm, float *grad_norm_out, void *stream);

/* SB3's target_kl (PPO.train: after a minibatch's loss, `if approx_kl_div > 1.5 * target_kl` the minibatch takes no
 * optimiser step and no further minibatch of any epoch runs; its statistics are still logged) with the decision on the
 * device, so the host enqueues every minibatch of an update and never reads a value in between.
 *   control_dev  i32[2] = {stopped, minibatches_run}, caller-owned device memory, zeroed by the caller before an update
 * mse_ppo_loss_grad_gated: with stopped != 0 on entry all three launches exit at once: grad_out and stats_out are not
 * written (the workspace, whose contents never survive a call, gets one marker cell).  Otherwise it is
 * mse_ppo_loss_grad, same bits; the lane that writes stats_out then increments minibatches_run and sets stopped = 1 when
 * (double)stats_out[4] > 1.5 * target_kl - the comparison SB3 makes between a float32 mean and a Python float.
 * target_kl <= 0: the flag is honoured and the count kept, but never set.
 * mse_ppo_adam_step_gated: does nothing when stopped != 0, else mse_ppo_adam_step.  `step` is the caller's count as if
 * every step were taken: no step follows a skipped one, so the steps that run have the right number.
 * The flag is only ever written by that one lane and read at the entry of LATER launches of the same stream, so every
 * wave of a launch sees the same value.  The ungated entry points are these with no control block. */
int mse_ppo_loss_grad_gated(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                            int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                            const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                            float *stats_out, void *workspace, void *stream, double target_kl, int32_t *control_dev);
int mse_ppo_adam_step_gated(int64_t n_weights, float *weights, const float *grad, float *m, float *v, int64_t step, double lr,
                            double beta1, double beta2, double eps, double max_grad_norm, float *grad_norm_out, void *stream,
                            const int32_t *control_dev);

/* mse_ppo_loss_grad / mse_ppo_loss_grad_gated with the gradient launch on the f32 matrix cores (k_ppo_grad_matrix:
 * v_mfma_f32_32x32x2_f32, f32 operands and f32 accumulation).  Same arguments, same checks in the same order before any
 * device call, same status codes, same workspace, same meaning of every output; control_dev may be NULL: no gate, and
 * target_kl is not read.  With a control block it behaves as mse_ppo_loss_grad_gated does (a closed gate writes neither
 * grad_out nor stats_out; the lane that writes stats_out counts the minibatch and sets stopped on
 * (double)stats_out[4] > 1.5 * target_kl).
 * What differs from mse_ppo_loss_grad is the ORDER in which the sums of products are formed, nothing else: the forward
 * layers, the back-propagations and the weight gradients run as matrix products (a weight's input index, or the tile's
 * rows, in the k order of the instruction), the per-row arithmetic (tanh, the masked softmax and its terms, the value
 * error, the advantage normalisation, the clamping of rows and actions) is the same code.  The results therefore agree
 * with mse_ppo_loss_grad within rounding, not bit for bit; stats_out[6..7] (from the launches around the gradient, which
 * are the same) are bit-equal.  Equal inputs still give bit-equal outputs: no atomics, fixed orders.  The grid rule is
 * mse_ppo_loss_grad's. */
int mse_ppo_loss_grad_matrix(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                             int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions,
                             const float *old_logp, const float *advantages, const float *returns,
                             const mse_ppo_params *params, float *grad_out, float *stats_out, void *workspace,
                             void *stream, double target_kl, int32_t *control_dev /* NULL: no gate, target_kl unread */);

/* SB3's clip_range_vf, and the one entry point that covers every form above: either arithmetic, gated or not, with or
 * without value clipping.  The first 17 arguments are mse_ppo_loss_grad's; target_kl and control_dev are
 * mse_ppo_loss_grad_matrix's (NULL: no gate, target_kl unread).
 *   arithmetic     0: fmaf chains (k_ppo_grad), 1: matrix cores (k_ppo_grad_matrix)
 *   old_values     f32[n_rows] or NULL: the value predictions the rollout was collected with, read at the rows `returns`
 *                  is read at
 *   clip_range_vf  read only with old_values; then it must be finite and > 0, also once rounded to float32
 * old_values == NULL: no value clipping; the call is mse_ppo_loss_grad (arithmetic 0, no control block),
 * mse_ppo_loss_grad_gated (0, control block) or mse_ppo_loss_grad_matrix (1): the same launches, the same bits.
 * old_values != NULL: the critic's loss is that of the clipped prediction (PPO.train), float32, every operation rounded
 * separately, c = (float)clip_range_vf:
 *   d = value - old_value;  dc = min(max(d, -c), c);  vp = old_value + dc;  e = vp - returns
 *   value_loss = mean(e^2) (stats_out[2], and the value term of stats_out[0]: of the clipped prediction, as SB3 logs them)
 *   d loss / d value = vf_coef * 2 * e / batch where d == dc (torch.clamp passes the gradient on its closed range), else 0
 * Nothing else differs: the policy network's gradient and stats_out[1], [3] .. [7] are bit-equal with and without
 * old_values.  The gradient launch is a separate instantiation of the same kernel, so the unclipped launch is unchanged.
 * Checks, all before any device call, in this order: a NaN target_kl beside a control block; then mse_ppo_loss_grad's
 * (null arguments, dimensions, struct_size, batch, coefficients, workspace alignment); then arithmetic outside {0, 1};
 * then, with old_values, a clip_range_vf that is not finite and > 0.  Each is MSE_ERR_INVALID_ARGUMENT
 * (MSE_ERR_ALIGNMENT for the workspace).  Same workspace, same grid rule, equal inputs give bit-equal outputs. */
int mse_ppo_loss_grad_vclip(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                            int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                            const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                            float *stats_out, void *workspace, void *stream, double target_kl,
                            int32_t *control_dev /* NULL: no gate */, int arithmetic /* 0 fma, 1 matrix */,
                            const float *old_values /* f32[n_rows] or NULL */, double clip_range_vf);

/* mse_ppo_loss_grad_vclip for ONE minibatch whose rows live in several places ("shards": the ranks of a data-parallel
 * learner, each with the rollout rows it collected).  The call is cut at the two points where the other shards' numbers
 * enter, and what crosses is small: four doubles, then mse_ppo_shard_partial_len(D, A) doubles.  Per minibatch every shard runs
 *   1. mse_ppo_shard_moments      -> moments_out; the caller SUMS the shards' moments element-wise (an all-reduce)
 *   2. mse_ppo_shard_loss_grad    on the summed moments -> partial_out; the caller SUMS the shards' partials element-wise
 *   3. mse_ppo_shard_finish       on the summed partial and the summed moments -> grad_out, stats_out, the target_kl gate
 * then mse_ppo_adam_step[_gated], unchanged.  Every shard that is given the same sums computes the same bits in step 3 and so
 * takes the same decision.  The PPO head only (either arithmetic, with or without old_values); the behaviour-cloning and
 * imitation-term losses have no sharded form.  As everywhere here: caller-owned device memory, all work on `stream`, nothing
 * allocates or synchronises, every argument is checked before any device call, no atomics and fixed orders, so equal inputs give
 * bit-equal outputs.  The result is NOT independent of how the rows are cut into shards: the sums are formed in another
 * order, so two splits of the same rows agree within rounding, as the two arithmetics do.
 *
 * mse_ppo_shard_moments: n_rows, rows_dev, advantages are mse_ppo_loss_grad's, with its clamping of row indices (row_at).
 *   batch_local  >= 0 rows of this shard in the minibatch; 0 is legal: zeros are written and no row is read (rows_dev, which
 *                is otherwise i64[batch_local] or NULL for rows 0 .. batch_local - 1, may then be NULL)
 *   moments_out  f64[4], 8-byte aligned: {batch_local, sum a, sum a^2, 0} over this shard's rows a = advantages[row], in
 *                double: lanes add their rows in order, a fixed tree inside a group of 256 lanes, the min(256, ceil(batch_local
 *                / 1024)) groups' pairs (in the workspace) added in index order by one lane
 *   workspace    mse_ppo_workspace_bytes(D, A) bytes of any D, A (4 KiB are used), 16-byte aligned
 *   control_dev  i32[2] or NULL, mse_ppo_loss_grad_gated's block: with stopped != 0 on entry nothing is written
 * The rule the sums serve, B being the global row count: mean = sum a / B; unbiased variance = (sum a^2 - (sum a)^2 / B) /
 * (B - 1), in double, clamped at 0; std = sqrt(variance); mean and std rounded to float32 once; a row's advantage becomes
 * (a - mean) / (std + 1e-8) in float32, as in mse_ppo_loss_grad.
 * Checks, in this order: null advantages, moments_out or workspace; n_rows < 1, batch_local < 0 or batch_local > n_rows
 * without rows_dev; workspace not 16-byte aligned, then moments_out not 8-byte aligned (MSE_ERR_ALIGNMENT); no device
 * (MSE_ERR_NO_DEVICE).  The others are MSE_ERR_INVALID_ARGUMENT.
 *
 * mse_ppo_shard_loss_grad: the first 13 arguments are mse_ppo_loss_grad's, `batch` being batch_local >= 0.
 *   global_batch B >= max(1, batch_local): the rows of the minibatch over all shards.  Every per-row term is scaled by 1 / B
 *                where mse_ppo_loss_grad scales by 1 / batch
 *   moments_dev  f64[4], device memory, 8-byte aligned: the SUM of all shards' moments_out.  Advantages are normalised by the
 *                rule above when normalize_advantage != 0 and B >= 2 (mse_ppo_loss_grad's rule on the global count)
 *   partial_out  f64[mse_ppo_shard_partial_len(D, A)], 8-byte aligned, in DOUBLE: the W gradient sums in the flat order,
 *                then the five statistic sums of the gradient kernels' slabs, not divided (surrogate, squared value error,
 *                entropy, kl, clipped), then zeros up to a multiple of 4.  Each is the sum of the shard's slabs in slab order
 *   workspace    mse_ppo_workspace_bytes(D, A) bytes, 16-byte aligned
 *   control_dev  i32[2] or NULL: with stopped != 0 on entry partial_out is not written (the workspace gets one marker cell)
 *   arithmetic, old_values, clip_range_vf   mse_ppo_loss_grad_vclip's
 * Two launches: the SHARD instantiation of the gradient kernel of either arithmetic (the grid rule is mse_ppo_loss_grad's on
 * batch_local), then the slab sums.  batch_local = 0 launches no gradient kernel and writes zeros.
 * Checks, in this order: null arguments (rows_dev, mask, control_dev and old_values may be NULL); dimensions outside 1..32;
 * struct_size; n_rows < 1, batch_local < 0 or batch_local > n_rows without rows_dev; global_batch < max(1, batch_local);
 * clip_range / ent_coef / vf_coef; workspace not 16-byte aligned, then moments_dev or partial_out not 8-byte aligned
 * (MSE_ERR_ALIGNMENT); arithmetic outside {0, 1}; with old_values, a clip_range_vf that is not finite and > 0; no device
 * (MSE_ERR_NO_DEVICE).  The others are MSE_ERR_INVALID_ARGUMENT.
 *
 * mse_ppo_shard_finish: one launch of one workgroup.
 *   reduced_dev  f64[mse_ppo_shard_partial_len(D, A)]: the SUM of all shards' partial_out;  moments_dev as above
 *   grad_out     f32[W]: grad_out[i] = (float)reduced[i]
 *   stats_out    f32[8]: exactly mse_ppo_loss_grad's eight, from the statistic sums divided by global_batch in double; [6], [7]
 *                are the mean and std that were used, 0 and 1 when not normalised
 *   target_kl, control_dev   mse_ppo_loss_grad_matrix's (NULL: no gate, target_kl unread): a gate that was closed on entry
 *                writes nothing; otherwise one lane counts the minibatch and sets stopped on
 *                (double)stats_out[4] > 1.5 * target_kl.  Every lane reads the gate before that lane writes it.
 * Checks, in this order: a NaN target_kl beside a control block; null reduced_dev, moments_dev, params, grad_out or
 * stats_out; dimensions; struct_size; global_batch < 1; ent_coef or vf_coef not finite; reduced_dev or moments_dev not 8-byte
 * aligned (MSE_ERR_ALIGNMENT); no device (MSE_ERR_NO_DEVICE).  The others are MSE_ERR_INVALID_ARGUMENT. */
int64_t mse_ppo_shard_partial_len(int obs_dim, int n_actions); /* in doubles; 0 for dimensions outside 1..32; needs no device */
int mse_ppo_shard_moments(int64_t n_rows, const int64_t *rows_dev, int64_t batch_local, const float *advantages,
                          double *moments_out /* f64[4] */, void *workspace, void *stream,
                          const int32_t *control_dev /* NULL: no gate */);
int mse_ppo_shard_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                            int64_t batch_local, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                            const float *advantages, const float *returns, const mse_ppo_params *params, int64_t global_batch,
                            const double *moments_dev /* f64[4], summed */, double *partial_out, void *workspace, void *stream,
                            const int32_t *control_dev /* NULL: no gate */, int arithmetic /* 0 fma, 1 matrix */,
                            const float *old_values /* f32[n_rows] or NULL */, double clip_range_vf);
int mse_ppo_shard_finish(int obs_dim, int n_actions, int64_t global_batch, const double *reduced_dev /* summed */,
                         const double *moments_dev /* f64[4], summed */, const mse_ppo_params *params, float *grad_out,
                         float *stats_out /* f32[8] */, void *stream, double target_kl, int32_t *control_dev /* NULL: no gate */);

/* Behaviour cloning: the cross-entropy of DEMONSTRATED actions (the rule-based controller's, mse_rule_actions) under the
 * policy's masked softmax, its statistics and the gradient of its loss, for one minibatch.  weights_dev, n_rows, rows_dev,
 * batch, obs, mask, grad_out, workspace and stream are mse_ppo_loss_grad's, with its clamping of row indices.
 *   actions      i32[n_rows]: the demonstrated action of every row, clamped into [0, A)
 *   returns      f32[n_rows] or NULL.  NULL: actor only - the critic contributes nothing, value_loss is 0 and the
 *                gradient of every critic weight is exactly 0
 *   params       ent_coef and vf_coef are read; clip_range and normalize_advantage are ignored
 *   arithmetic   0: fmaf chains (k_ppo_grad), 1: matrix cores (k_ppo_grad_matrix); each its behaviour-cloning instantiation
 * Per row, float32 with every operation rounded separately (csrc/mse_ppo_math.h, bc_head_terms): the actor's 2 x 32 tanh
 * MLP forward; illegal actions at logit -1e8; m = max logit, lse = m + log(sum exp(logit - m)); lp[a] = logit[a] - lse and
 * p[a] = exp(lp[a]) for legal a, p[a] = 0 otherwise; entropy = -sum p[a] lp[a]; mass = sum p[a]; rest = mass - entropy.
 * usable = the demonstrated action is legal under the mask:
 *   ce = usable ? -lp[action] : 0;      g = usable ? -1 / batch : 0
 *   d loss / d logit[a] = g (onehot(a == action) - p[a]) + ent_coef / batch (p[a] (lp[a] + 1) - p[a] rest)   for legal a, else 0
 *   hit = usable and argmax of the masked logits == action (ties to the lowest index: the policy head's deterministic rule)
 * so a row whose demonstrated action the mask forbids adds 0 to the cross-entropy and its gradient and 1 to `unusable`,
 * and keeps its entropy term.  With returns the critic is mse_ppo_loss_grad's: e = value - returns, value_loss = mean(e^2),
 * d loss / d value = vf_coef * 2 * e / batch.
 *   bc_loss = mean(ce) over the batch (unusable rows counting 0);  entropy_loss = -mean(entropy)
 *   loss = bc_loss + ent_coef entropy_loss + vf_coef value_loss
 *   stats_out    f32[8]: loss, bc_loss, value_loss, entropy_loss, accuracy = hits / batch, unusable rows / batch, 0, 1
 * Two launches (the gradient kernel, then mse_ppo_loss_grad's reduction; there is no advantage pass), the grid rule, the
 * slab sums in a fixed order without atomics: equal inputs give bit-equal outputs.  The two arithmetics agree within
 * rounding; accuracy and unusable are counts and agree exactly wherever the argmax is not a float32 near-tie.
 * Checks, all before any device call, in this order: null arguments (weights_dev, obs, actions, params, grad_out,
 * stats_out, workspace); dimensions outside 1..32; struct_size; n_rows < 1, batch < 1 or batch > n_rows without rows_dev;
 * ent_coef or vf_coef not finite; workspace not 16-byte aligned (MSE_ERR_ALIGNMENT); arithmetic outside {0, 1}; no device
 * (MSE_ERR_NO_DEVICE).  The others are MSE_ERR_INVALID_ARGUMENT. */
int mse_bc_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev, int64_t batch,
                     const float *obs, const uint8_t *mask /* or NULL */, const int32_t *actions,
                     const float *returns /* or NULL: actor only */, const mse_ppo_params *params, float *grad_out,
                     float *stats_out, void *workspace, void *stream, int arithmetic /* 0 fma, 1 matrix */);

/* PPO with an auxiliary imitation term (DAPG / kickstarting): mse_ppo_loss_grad_vclip's loss plus bc_coef times the
 * cross-entropy of the rule-based controller's action at every row, from ONE forward pass, in one gradient launch:
 *   loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss + bc_coef bc_loss
 * The first 22 arguments are mse_ppo_loss_grad_vclip's with the same meaning (either arithmetic, gated or not, with or
 * without old_values), except:
 *   stats_out      f32[12]: [0] the loss above, [1..7] as mse_ppo_loss_grad, [8] bc_loss = mean(ce), [9] accuracy = hits /
 *                  batch, [10] unusable rows / batch, [11] 0.  The gate reads [4] as before.
 *   workspace      mse_ppo_bc_workspace_bytes(D, A) bytes (a few KiB more than mse_ppo_workspace_bytes: wider slabs)
 *   expert_actions i32[n_rows]: the label of every row (mse_rule_actions of the state the row shows:
 *                  mse_rollout_policy_labelled's expert_actions_out), clamped into [0, A)
 *   bc_coef        >= 0, used as a float32; 0 is allowed
 * Per row (csrc/mse_ppo_math.h, policy_bc_head_terms): the masked softmax and every PPO term are policy_head_terms'; with
 * usable = the label is legal under the mask,  ce = usable ? -lp[expert] : 0,  g_bc = usable ? -(bc_coef / batch) : 0,
 *   d loss / d logit[a] = g_logp (onehot(a == action) - p[a]) + g_bc (onehot(a == expert) - p[a])
 *                         + ent_coef / batch (p[a] (lp[a] + 1) - p[a] rest)        for legal a, else 0,  added left to right
 *   hit = usable and argmax of the masked logits == expert (ties to the lowest index)
 * A row whose label the mask forbids adds 0 to ce and its gradient and 1 to `unusable`, and keeps its PPO and entropy terms.
 * With bc_coef = 0 grad_out and stats_out[0..7] equal mse_ppo_loss_grad_vclip's on the same inputs bit for bit, up to the
 * sign of a zero.  Three launches as before (the advantage pass, the KICK entry of the gradient kernel, the reduction's
 * twelve-column form), the same grid rule, fixed-order sums without atomics: equal inputs give bit-equal outputs.
 * Checks, all before any device call, in this order: mse_ppo_loss_grad_vclip's; expert_actions == NULL; bc_coef not finite,
 * negative, or not finite as a float32.  Each of the new ones is MSE_ERR_INVALID_ARGUMENT. */
int64_t mse_ppo_bc_workspace_bytes(int obs_dim, int n_actions); /* 0 for dimensions outside 1..32; needs no device */
int mse_ppo_bc_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                         int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                         const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                         float *stats_out /* f32[12] */, void *workspace, void *stream, double target_kl,
                         int32_t *control_dev /* NULL: no gate */, int arithmetic /* 0 fma, 1 matrix */,
                         const float *old_values /* f32[n_rows] or NULL */, double clip_range_vf,
                         const int32_t *expert_actions /* i32[n_rows] */, double bc_coef);

/* SB3's train/explained_variance: 1 - var(returns - values) / var(returns) over n rows (all K * N of a rollout), population
 * variances, NaN when var(returns) is 0 (n = 1, constant returns).  csrc/mse_ppo_math.h specifies the arithmetic
 * completely; in short: the differences returns - values are formed in double from the f32 inputs; sums and sums of
 * squares are taken in double about a pivot (element 0) by min(256, ceil(n / 1024)) groups of 256 lanes, a fixed tree
 * inside a group, the groups' partials added in index order; variances and their ratio in double; ONE rounding to f32 at
 * the store.  No atomics: equal inputs give equal bits, and the host twin adds the same numbers in the same order, so
 * device and host agree bit for bit.  values == returns gives exactly 1.
 *   out_dev      f32[1], the only thing written beside the workspace
 *   workspace    mse_explained_variance_workspace_bytes() bytes (8 KiB), 8-byte aligned, contents need not survive; a
 *                workspace of mse_ppo_workspace_bytes is large enough and may be passed between two gradient calls
 * Two small launches on `stream` (the partials, then one lane that adds them); nothing allocates or synchronises; the
 * arguments (non-null, n >= 1, alignment) are checked before any device call.  The host form needs no device. */
int64_t mse_explained_variance_workspace_bytes(void);
int mse_explained_variance(int64_t n, const float *values, const float *returns, float *out_dev /* f32[1] */, void *workspace,
                           void *stream);
int mse_explained_variance_host(int64_t n, const float *values, const float *returns, float *out);

/* The learner's minibatch shuffle: rows_out[j] = perm(seed, epoch, total, first + j) for j < count, where perm(seed, epoch,
 * total, .) is a bijection of [0, total) computed per element from its arguments alone (a keyed Feistel network with
 * cycle walking, 32-bit integer arithmetic; csrc/mse_ppo_math.h specifies it completely).  No generator and no state:
 * any window (first, count) of any epoch can be produced anywhere, and the host twin returns the very same integers,
 * so an update is replayed without the device.  The learner passes its seed and a counter of the epochs it has run.
 *   total        1 .. 2^31 rows; first >= 0, count >= 0, first + count <= total, else MSE_ERR_INVALID_ARGUMENT
 *   rows_out     i64[count], 8-byte aligned; may be NULL only when count == 0 (which succeeds and does nothing)
 * The device form is one launch on `stream` (16-byte stores where the address allows), the host form needs no device. */
int mse_ppo_shuffle(int64_t total, uint64_t seed, uint64_t epoch, int64_t first, int64_t count, int64_t *rows_out_dev,
                    void *stream);
int mse_ppo_shuffle_host(int64_t total, uint64_t seed, uint64_t epoch, int64_t first, int64_t count, int64_t *rows_out);

/* ---- Episode accounting: cumulative reward per episode, the unit the reference measures a policy in ---------------------
 * (SB3's Monitor: rollout/ep_rew_mean, ep_len_mean; evaluate_policy(model, env, n_eval_episodes) and EvalCallback,
 * src/training.py:69,149-157,196-209; np.mean / np.std of cumulative rewards, utils/benchmark_models.py:39;
 * cumulative_reward, src/testing.py:54.)  All buffers are caller-owned device memory (host memory for the *_host forms),
 * all work goes to `stream`, nothing allocates or synchronises, and the arguments are checked before any device call.
 * csrc/mse_episode_math.h specifies the arithmetic completely; the kernels and the host forms run that one header.
 *
 * mse_episode_scan walks step-major rollout buffers, one env per lane, steps k = 0 .. K - 1 in order:
 *   rewards        f32[K,N]
 *   the end of an episode, given in exactly ONE of the project's two forms (else MSE_ERR_INVALID_ARGUMENT):
 *     dones          u8[K,N]   done_out of mse_rollout / mse_rollout_model: step k ended an episode iff dones[k] != 0
 *     episode_starts u8[K,N] + last_dones u8[N]   the buffers of mse_rollout_policy: step k ended an episode iff
 *                    episode_starts[k + 1] != 0, last_dones at k = K - 1; episode_starts[0] is not read
 *   run_return f64[N], run_length i32[N]   the carry, read and written: zero it once, then a return spans any number of calls
 *   ep_count   i32[N]   read and written: the episodes of env i counted so far
 *   targets    i32[N] or NULL: an ended episode is counted iff targets == NULL or ep_count[i] < targets[i] - the per-env
 *              rule of evaluate_policy, whose targets are (n_eval_episodes + i) / N rounded down
 *   slots, ledger_return f64[slots,N], ledger_length i32[slots,N], or 0 / NULL / NULL: a counted episode is stored at slot
 *              ep_count[i] while that is < slots (slot-major, so the stores coalesce); cells of episodes that did not
 *              happen are not written
 *   totals     f64[5] or NULL: counted episodes, sum of returns, sum of lengths, min return, max return.  ADDED TO what
 *              is passed in (min / max combined; those of a totals[] whose count is 0 are ignored), so a window over
 *              several rollouts is one zero-fill and then calls
 *   workspace  mse_episode_workspace_bytes() bytes, 8-byte aligned, needed with totals; contents need not survive
 * Per step: run_return += (double)reward, run_length += 1; at an episode's end it is counted (ledger, totals,
 * ep_count += 1) or not, and the carry is cleared either way.  A return is thus the float64 sum, in step order, of the
 * FLOAT32 rewards the buffer holds; Monitor sums the env's float64 rewards and rounds to 6 digits, so the two differ by
 * at most  episode length x 2^-24 x max |reward|  (plus Monitor's own rounding).  Per-env outputs do not depend on the
 * launch shape.  The totals are reduced per wave, then over the workgroup's waves in LDS, one slab per workgroup goes to
 * the workspace and a one-workgroup launch folds the slabs in a fixed order: no atomics, equal inputs give bit-equal
 * outputs.  The lane -> env mapping and the grid cap are fixed functions of N and the device.  Two launches (one
 * without totals).
 *
 * mse_episode_summary: np.mean / np.std (ddof 0) over the ledger entries of the counted episodes, two passes with the
 * rounded mean subtracted in the second, in a fixed order.  summary f64[6]: episodes, mean return, std return, mean
 * length, min return, max return (NaN beside a count of 0).  It covers what the ledger holds: slots 0 ..
 * min(ep_count[i], slots) - 1 of env i.  Without a ledger it refuses (MSE_ERR_INVALID_ARGUMENT, nothing launched).
 * One launch of one workgroup.
 *
 * The *_host forms run the same walk and the same formulas on host arrays (envs in ascending order) and need no
 * device: per-env outputs, counts, lengths, min and max equal the device's bit for bit, the sums to rounding. */
int64_t mse_episode_workspace_bytes(void);
int mse_episode_scan(int32_t k_steps, int64_t n, const float *rewards, const uint8_t *dones, const uint8_t *episode_starts,
                     const uint8_t *last_dones, double *run_return, int32_t *run_length, int32_t *ep_count, const int32_t *targets,
                     int32_t slots, double *ledger_return, int32_t *ledger_length, double *totals, void *workspace, void *stream);
int mse_episode_scan_host(int32_t k_steps, int64_t n, const float *rewards, const uint8_t *dones, const uint8_t *episode_starts,
                          const uint8_t *last_dones, double *run_return, int32_t *run_length, int32_t *ep_count,
                          const int32_t *targets, int32_t slots, double *ledger_return, int32_t *ledger_length, double *totals);
int mse_episode_summary(int64_t n, int32_t slots, const int32_t *ep_count, const double *ledger_return, const int32_t *ledger_length,
                        double *summary, void *stream);
int mse_episode_summary_host(int64_t n, int32_t slots, const int32_t *ep_count, const double *ledger_return,
                             const int32_t *ledger_length, double *summary);

/* ---- Plant ledger: per-episode plant quantities of every env, out of the all-env trace ------------------------------------
 * What the reference's dashboard reads off ONE env - reward_data's (r_sort, r_press) pairs, press_actions_per_timestep,
 * the bale_count lists and _calculate_avg_bale_deviation (env_super.py:235-241, 661-687, 928-946; utils/plotting.py:32-48)
 * - as one row of MSE_PLANT_COLS doubles per episode, for all N envs.  csrc/mse_plant_math.h specifies the arithmetic
 * completely; the kernel and the host form run that one header.
 *
 * mse_plant_scan walks records f64[K, MSE_TRACE_COLS, N] (mse_trace_begin_all), one env per lane, steps k = 0 .. K - 1 in
 * order.  Per step: first the N_BALE press_bale calls in order (n / S full bales; a remainder > remainder_units opens a
 * bale; else it merges into the last bale of that material if the episode has one; else it opens one), then the N_LOG
 * press-log codes, then the reward parts.  An episode closes at DONE != 0; its row is
 *    0        length
 *    1 2 3    sum REWARD, sum R_SORT, sum R_PRESS (float64 sums in step order)
 *    4 5      presses started on press 1 / press 2 (codes 1, 2)
 *    6        busy or invalid attempts (codes 111, 222)        7   no-ops (code 0)
 *    8        OVERFLOW of the closing step                     9   material left in the containers at the closing step
 *    10-14    bales of A..E after the merge rule               15-19  their mass
 *    20-24    sum over bales of the stored quality in hundredths (a merge keeps the last bale's quality)
 *    25-29    sum over bales of |size - S|, an integer (a merge replaces the last bale's term)
 *    30 31    zero
 * The reference's average bale deviation is (sum of 25-29) / (S x sum of 10-14), formed once outside the sums.
 *   bale_standard_size S, remainder_units = floor(S x bale_remainder_threshold): mse_plant_params gives both
 *   run        f64[MSE_PLANT_RUN_COLS, N]  the carry, read and written: rows 0-29 are the open episode's columns (8 and 9
 *              stay 0), rows 30-34 the size of the last bale of A..E, row 35 is not touched.  Zero it once.
 *   ep_count, targets, slots   as in mse_episode_scan; ledger f64[slots, MSE_PLANT_COLS, N] or NULL with slots 0: a counted
 *              episode is stored at slot ep_count[i] while that is < slots; the carry is cleared at every episode end
 *   totals     f64[1 + MSE_PLANT_COLS] or NULL, ADDED TO: [0] counted episodes, [1 + c] the sum of column c (column 8 as
 *              overflow != 0).  Every column but 1-3 is integer-valued, so exact in any order.
 *   workspace  mse_plant_workspace_bytes() bytes, 8-byte aligned, needed with totals
 * Totals are reduced per wave, then over the workgroup's waves in LDS, one slab per workgroup goes to the workspace, a
 * one-workgroup launch folds the slabs in index order: no atomics, equal inputs give bit-equal outputs.
 * Refusals, all before any device call, in this order: k_steps < 1 or n < 1; records, run or ep_count NULL; slots < 0,
 * or a ledger without slots, or slots without a ledger; bale_standard_size < 1 or remainder_units outside
 * [0, bale_standard_size) (all MSE_ERR_INVALID_ARGUMENT); device form only: totals without a workspace
 * (MSE_ERR_INVALID_ARGUMENT); records, run, ledger, totals or workspace not 8-byte aligned (MSE_ERR_ALIGNMENT); device
 * form only: no HIP device (MSE_ERR_NO_DEVICE).  Nothing is written on a refusal.
 * mse_plant_scan_host is the same on host arrays, envs in ascending order; it and mse_plant_params need no device.
 * Per-env outputs (carry, ledger, ep_count) and the integer totals equal the device's bit for bit, totals 1-3 to rounding. */
#define MSE_PLANT_COLS 32
#define MSE_PLANT_RUN_COLS 36
int64_t mse_plant_workspace_bytes(void);
int mse_plant_scan(int32_t k_steps, int64_t n, const double *records, int32_t bale_standard_size, int32_t remainder_units,
                   double *run, int32_t *ep_count, const int32_t *targets, int32_t slots, double *ledger, double *totals,
                   void *workspace, void *stream);
int mse_plant_scan_host(int32_t k_steps, int64_t n, const double *records, int32_t bale_standard_size, int32_t remainder_units,
                        double *run, int32_t *ep_count, const int32_t *targets, int32_t slots, double *ledger, double *totals);
/* out = {bale_standard_size, floor(bale_standard_size x bale_remainder_threshold)} as the handle's compiled config holds them */
int mse_plant_params(const mse_env *env, int32_t out[2]);

/* ---- Lookahead: fork every env and score each candidate action in ONE launch (the rollout algorithm's inner loop) ----------
 * Per env i, candidate action a < A (A = mse_num_actions) and sample m < n_samples, the fork is a copy of env i's current
 * state held in registers, stepped with masking on (use_action_masking=True; MSE_STEP_CHECK_OVERFLOW honoured):
 *   - a candidate that the current action_masks() forbids runs no step and gets q = -inf;
 *   - step 0 is mse_step's transition under action a; steps s = 1 .. horizon - 1 take the base policy's action for the
 *     fork's state: base_policy = 1 what mse_rule_actions returns for it, base_policy = 0 the masked-uniform action
 *     mse_sample_actions draws with the policy stream's word of (base_seed, index_offset + i, s) (csrc/mse_policy_stream.h:
 *     the word at s under the key of base_seed and the index) - it depends on neither a nor m: common random numbers; Env_2's sorting decision
 *     is sort_mode_dev[i] at every step of the fork (NULL: sorting_rules());
 *   - the fork ends with its episode (max_steps, or an overflow under MSE_STEP_CHECK_OVERFLOW): there is no auto-reset
 *     inside a fork, and steps after `done` add nothing;
 *   - ret = sum over the steps taken of disc_s * reward64_s in double, formed in step order as acc += disc * r;
 *     disc *= gamma, every operation rounded on its own (no fused multiply-add), acc = 0 and disc = 1 at the start;
 *   - q_out[a][i] = (ret_0 + ... + ret_{M-1}) / M, added in sample order, in double (every fork writes its return to the
 *     workspace, f64[M][A][N]; a second small kernel forms the mean and the argmax);
 *   - action_out[i] = the legal candidate of largest q, ties to the lowest index; value_out[i] = that q;
 *   - streams = 0 ("own"): every PCG64 stream of the fork continues the env's own: the fork sees the draws the env itself
 *     is going to see (clairvoyant: an upper bound, and the form that can be held against real stepping);
 *   - streams = 1 ("fresh"): every stream column of the fork's state record (the rng block of mse_get_state) is the one
 *     mse_reset gives an env seeded with mse_lookahead_stream_seed(lookahead_seed, index_offset + i, m); everything else,
 *     the seasonal generator's position included, stays the env's.  The candidate is not part of the key: the candidates of
 *     one env and sample share their draws.  With streams = 0 the samples are copies of one another;
 *   - nothing of the handle is written: state planes, policy step counter, bale ledger, trace and error count stay; a
 *     fork's press_bale bookings go to a ledger that discards them (nothing a step computes reads the ledger).
 * mse_lookahead_stream_seed (host, pure; csrc/mse_lookahead_seed.h is the one definition, for host and device): with
 * mix(z) { z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31); }
 * and arithmetic modulo 2^64:  a = mix(lookahead_seed + 0x9E3779B97F4A7C15);  b = mix(a ^ global_env_index);
 * c = mix(b + (sample + 1) * 0x9E3779B97F4A7C15);  the seed is c >> 1 (below 2^63).
 * Shape: one lane per (env, candidate, sample), grid (ceil(N / 256), A, M) x 256 threads, the lookup tables in LDS; one
 * launch of it and one of the reduction, both on `stream`; no allocation, no synchronisation.  Works on a handle with or
 * without auto_reset, with or without an attached trace, and with literal_choice.
 *   q_out f64[A][N]; action_out i32[N] or NULL; value_out f64[N] or NULL; workspace: mse_lookahead_workspace_bytes(env,
 *   n_samples) bytes of device memory (8 N A M; a negative mse_status for a NULL env or n_samples out of range).
 * Refusals, all before any device call, in this order: MSE_ERR_INVALID_ARGUMENT - a NULL env, q_out or workspace;
 * horizon < 1 or > MSE_LOOKAHEAD_MAX_HORIZON; n_samples < 1 or > MSE_LOOKAHEAD_MAX_SAMPLES; gamma not a number in [0, 1];
 * base_policy or streams outside {0, 1}; a flag other than MSE_STEP_CHECK_OVERFLOW; sort_mode_dev on a kind other than
 * Env_2.  MSE_ERR_UNSUPPORTED_CONFIG - general generator mode (the fork does not carry the input generator's private
 * stream).  MSE_ERR_NOT_RESET - a handle not yet reset.  MSE_ERR_ALIGNMENT - q_out, value_out or workspace not 8-byte
 * aligned.  A handle exists only on a device (mse_create's MSE_ERR_NO_DEVICE), so there is no such refusal here.  A refused
 * call writes nothing. */
#define MSE_LOOKAHEAD_MAX_HORIZON 65535 /* = the largest max_steps: no fork runs longer */
#define MSE_LOOKAHEAD_MAX_SAMPLES 256
int64_t  mse_lookahead_workspace_bytes(const mse_env *env, int32_t n_samples);
uint64_t mse_lookahead_stream_seed(uint64_t lookahead_seed, uint64_t global_env_index, uint32_t sample);
int mse_lookahead(mse_env *env, int32_t horizon, double gamma, int32_t base_policy /* 0 random, 1 rule_based */,
                  uint64_t base_seed, int32_t streams /* 0 own, 1 fresh */, uint64_t lookahead_seed, int32_t n_samples,
                  const int32_t *sort_mode_dev /* Env_2, or NULL */, uint32_t flags /* MSE_STEP_CHECK_OVERFLOW or 0 */,
                  double *q_out /* f64[A][N] */, int32_t *action_out /* i32[N] or NULL */, double *value_out /* f64[N] or NULL */,
                  void *workspace, void *stream);

/* ---- Lookahead with a learned network inside the fork: the policy as base, the critic as leaf value -------
 * mse_lookahead's sentence - forks, candidates, samples, step 0, the end of a fork with its episode, ret, q_out, action_out,
 * value_out, both stream modes, sort_mode_dev, MSE_STEP_CHECK_OVERFLOW, the workspace (mse_lookahead_workspace_bytes), the
 * reduction, "nothing of the handle is written" and the fork's discarded bale ledger - with two changes:
 *   - the base policy: base_policy = 0 and 1 are mse_lookahead's (base_deterministic is ignored for them); with base_policy = 2
 *     steps s = 1 .. horizon - 1 take the action mse_policy_forward(policy, ...) returns for the fork's current state: its
 *     arguments are the fork's observation and action_masks() (masking always on), seed = base_seed, t = s, index_offset + i
 *     as the global env index and deterministic = base_deterministic.  base_deterministic != 0: the argmax of the masked
 *     logits, ties to the lowest index.  base_deterministic == 0: inverse-cdf sampling with the policy stream's word of
 *     (base_seed, index_offset + i, s) - the same word for every candidate and sample of an env (common random numbers),
 *     the rule base_policy = 0 follows;
 *   - the leaf value: with leaf_value = 1 a fork that has taken `horizon` steps and whose last step did not end its episode
 *     adds the critic's value of the state it stands in: ret = ret + disc * (double)v, the product and the sum rounded on
 *     their own, disc as the step loop left it (gamma multiplied in `horizon` times), v the f32 `value` mse_policy_forward
 *     returns for that state's observation.  A fork that ended with its episode adds nothing.  horizon = 1 with the leaf
 *     is the TD-greedy policy of the critic.
 * The policy's precision form (f32 or f16x3) is the handle's current one, as in mse_rollout_policy; its weights are read
 * when the launch runs (a learner that updates the handle in place is seen by the next call).  Neither handle is written.
 * Shape: mse_lookahead's grid, (ceil(N / 256), A, M) x 256 threads; a wave is 64 neighbouring envs under one candidate and
 * sample and runs the network on the matrix cores for its own 64 forks (two 32-env tiles), observations from registers;
 * LDS holds one policy weight image and the lookup tables.  The matrix work is done for whole waves, whatever share of
 * their lanes are legal forks.  One launch of it and one of the reduction, both on `stream`; no allocation, no
 * synchronisation.  Works with or without auto_reset and with or without an attached trace.
 * Refusals, all before any device call, in this order: mse_lookahead's MSE_ERR_INVALID_ARGUMENT refusals in its order - a NULL
 * env, q_out or workspace; horizon < 1 or > MSE_LOOKAHEAD_MAX_HORIZON; n_samples < 1 or > MSE_LOOKAHEAD_MAX_SAMPLES; gamma
 * not a number in [0, 1]; base_policy outside {0, 1, 2} or streams outside {0, 1}; a flag other than
 * MSE_STEP_CHECK_OVERFLOW; sort_mode_dev on a kind other than Env_2 -; then MSE_ERR_INVALID_ARGUMENT - a NULL policy; a policy
 * whose dimensions are not the env's obs_dim -> num_actions, or that lives on another device; leaf_value outside {0, 1};
 * base_policy != 2 with leaf_value == 0 (the network has nothing to do: mse_lookahead is the call).
 * MSE_ERR_UNSUPPORTED_CONFIG - general generator mode; a literal_choice handle; a config whose tables do not fit the LDS
 * beside the weight image.  MSE_ERR_NOT_RESET - a handle not yet reset.  MSE_ERR_ALIGNMENT - q_out, value_out or workspace not
 * 8-byte aligned.  A refused call writes nothing. */
int mse_lookahead_net(mse_env *env, mse_policy *policy, int32_t horizon, double gamma,
                      int32_t base_policy /* 0 random, 1 rule_based, 2 network */, int32_t base_deterministic,
                      uint64_t base_seed, int32_t leaf_value /* 0 or 1 */, int32_t streams /* 0 own, 1 fresh */,
                      uint64_t lookahead_seed, int32_t n_samples, const int32_t *sort_mode_dev /* Env_2, or NULL */,
                      uint32_t flags /* MSE_STEP_CHECK_OVERFLOW or 0 */, double *q_out /* f64[A][N] */,
                      int32_t *action_out /* i32[N] or NULL */, double *value_out /* f64[N] or NULL */, void *workspace,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MSE_H */
