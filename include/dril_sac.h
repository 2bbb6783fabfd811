/*
 * dril_sac.h — C ABI of the off-policy (SAC) path of libdril_hip.so (BASELINE.json configs[4]:
 * "SAC on Pendulum-v1, n_envs=4096, device ReplayBuffer + twin-Q/actor HIP kernels").
 *
 * Stands in for, in the reference checkout (KristianHolme/DRiL.jl):
 *   src/algorithms/sac.jl                       SAC, SACLayer, losses, update!, train!
 *   src/buffers/replay_buffer.jl                ReplayBuffer, get_data_loader
 *   src/buffers/off_policy_collection.jl        collect_trajectories / collect_rollout! (off-policy)
 *   src/DRiLDistributions/squashedDiagGaussian.jl
 *   src/layers/layer_forward.jl:15-28,75-87,118-125   ContinuousActorCriticLayer{QCritic}
 *   src/utils/optimization_utils.jl:3-58        polyak_update!, merge_params
 *
 * Conventions are those of dril_hip.h: int32 status (enum dril_status), the library owns device memory and the
 * handle, the caller owns host pointers for the duration of the call, calls are synchronous at return, arrays are
 * (features x batch) column-major, weights (out x in) column-major as Lux.Dense stores them.
 *
 * The SAC handle is its own object (the on-policy handle of dril_hip.h holds a RolloutBuffer and PPO state that
 * SAC has no use for); both live in the same shared library and share the device env kernels.
 */
#ifndef DRIL_SAC_H
#define DRIL_SAC_H

#include "dril_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRIL_SAC_ABI_VERSION 1u

typedef struct dril_sac_handle dril_sac_handle;

/* fields of ReplayBuffer (src/buffers/buffer_types.jl:28-41) for dril_sac_replay_copy_out; logical index 0 = oldest
 * element; within one collect call the device order is time-major (step, env) where the reference pushes whole
 * trajectories in completion order (replay_buffer.jl:98-114) — irrelevant to uniform sampling, documented for
 * anyone comparing flat arrays */
enum dril_replay_id {
    DRIL_RB_OBSERVATIONS = 0,      /* f32 (D, n)                                                          */
    DRIL_RB_ACTIONS = 1,           /* f32 (A, n): the UNPROCESSED policy action (off_policy_collection.jl:72) */
    DRIL_RB_REWARDS = 2,           /* f32 (n)                                                             */
    DRIL_RB_TERMINATED = 3,        /* u8  (n)                                                             */
    DRIL_RB_TRUNCATED = 4,         /* u8  (n): trajectory cut here by the env's time limit                */
    DRIL_RB_NEXT_OBSERVATIONS = 5  /* f32 (D, n): what get_data_loader resolves per sample, replay_buffer.jl:127-146
                                      (next step's observation | truncated_observation); rows of TERMINATED steps hold the
                                      terminal observation where the reference substitutes NaN — the loss never reads them */
};

/* Plain-C mirror of `SAC` (src/algorithms/sac.jl:25-36), the SACLayer kwargs (:72-85), the entropy-coefficient
 * types (src/interfaces/entropy.jl) and the env ctor kwargs */
typedef struct dril_sac_config {
    uint32_t abi_version;       /* DRIL_SAC_ABI_VERSION */
    int32_t env_kind;           /* Box action space required (sac.jl:74): DRIL_ENV_PENDULUM[_SCALED], DRIL_ENV_MOUNTAINCAR_CONTINUOUS, DRIL_ENV_EXTERNAL (host envs: ext_* below), or DRIL_ENV_MODULE (a device env plug-in: dril_sac_create_with_env_module) */
    int32_t n_envs;
    int32_t episode_len;        /* max_steps kwarg: 200 Pendulum-v1; DRIL_ENV_MODULE: 0 = the plug-in's own time limit */
    int32_t hidden1, hidden2;   /* SACLayer hidden_dims, default [512, 512] (sac.jl:76); multiples of 32 */
    int32_t activation;         /* 0 tanh, 1 relu (SACLayer default, sac.jl:77) */
    int64_t buffer_capacity;    /* :27 */
    int32_t start_steps;        /* :28 */
    int32_t batch_size;         /* :29 */
    float tau, gamma;           /* :30-31 */
    int32_t train_freq;         /* :32 */
    int32_t gradient_steps;     /* :33, -1 = train_freq * n_envs (get_gradient_steps :59-65) */
    int32_t target_update_interval; /* :35 */
    int32_t auto_ent_coef;      /* 1 AutoEntropyCoefficient, 0 FixedEntropyCoefficient (entropy.jl:17-24) */
    float ent_coef_init;        /* initial_value (1.0) | coef */
    int32_t auto_target_entropy;/* 1: -prod(size(action_space)) (sac.jl:47-57) */
    float target_entropy;       /* FixedEntropyTarget value */
    float learning_rate;        /* :26; the optimiser is Optimisers.Adam(lr) with library defaults (agent_methods.jl:116-118) */
    float adam_beta1, adam_beta2, adam_eps;   /* 0.9, 0.999, 1e-8 */
    uint64_t seed;              /* env i is seeded seed + i (wrapper_utils.jl:39-44) */
    int32_t device;
    int32_t profile_events;
    /* DRIL_ENV_EXTERNAL only: observation_space = Box of ext_obs_dim floats (<= 1024), action_space = Box(ext_action_low, ext_action_high) of
     * ext_action_dim floats (<= 16; the bounds feed TanhScaleAdapter, default_adapters.jl:13-21, and rand(action_space) of the start phase) */
    int32_t ext_obs_dim, ext_action_dim;
    float ext_action_low, ext_action_high;
    int32_t reserved[4];
} dril_sac_config;

/* NamedTuple returned by update!(agent, alg::SAC, batch), sac.jl:395-403; one per gradient step */
typedef struct dril_sac_stats {
    float actor_loss, critic_loss, entropy_loss, mean_q_values, entropy_coefficient, grad_norm;
    int32_t has_entropy_loss;   /* entropy_loss === nothing for FixedEntropyCoefficient */
    int32_t reserved;
} dril_sac_stats;

/* SAC() sac.jl:25-36, SACLayer kwargs :72-85, AutoEntropyCoefficient() entropy.jl:21-24 */
int32_t dril_sac_config_default(dril_sac_config* cfg, int32_t env_kind);

/* ---- lifetime: ReplayBuffer(obs_space, act_space, capacity) sac.jl:411 + Agent(layer, alg::SAC) sac.jl:160-188 */
int32_t dril_sac_create(const dril_sac_config* cfg, dril_sac_handle** out);
/* the same for cfg->env_kind == DRIL_ENV_MODULE: SAC on a device env plug-in (include/device/dril_env_plugin.h), the twin of dril_create_with_env_module with the same
 * load-time order and statuses (null / unreadable / non-code-object path: DRIL_ERR_INVALID_ARG before any HIP call; plug-in ABI number, argument-block size, S / D / A /
 * time limit: DRIL_ERR_UNSUPPORTED with a message before anything of the module is launched).  Refused in addition, each with a message: a Discrete plug-in (SAC needs
 * a Box, sac.jl:74), more than 16 action dims (the ext_action_dim limit), a dimension with action_low >= action_high (TanhScaleAdapter scales into a finite Box).
 * cfg->episode_len == 0 takes the descriptor's time limit; observation / action dims and the Box bounds PER DIMENSION come from the descriptor, the ext_* fields are
 * ignored.  Every verb below that works on a built-in device env works on such a handle; dril_sac_ext_push stays refused (the env is not on the host).  The module
 * is unloaded by dril_sac_destroy and on every failing path of this call.  dril_sac_create itself refuses DRIL_ENV_MODULE: it has no code object to load.
 * dril_env_module_describe (dril_hip.h) describes a path before a handle exists. */
int32_t dril_sac_create_with_env_module(const dril_sac_config* cfg, const char* code_object_path, dril_sac_handle** out);
/* spaces and bounds of the plug-in behind a live handle (DRIL_ERR_UNSUPPORTED for a handle of dril_sac_create) */
int32_t dril_sac_env_module_info_of(const dril_sac_handle* h, dril_env_module_info* out);
/* the declared observation space of the plug-in behind a live handle: dril_env_module_obs_space_of (dril_hip.h) for a SAC handle */
int32_t dril_sac_env_module_obs_space_of(const dril_sac_handle* h, float* low, float* high, int32_t* declared);
/* ScalingWrapperEnv around every env of a plug-in handle: dril_scaling_enable (dril_hip.h) for a SAC handle — the same env side, the same rule (between create and
 * the first dril_sac_env_reset, DRIL_ERR_INVALID_ARG afterwards), the same refusals.  While it is on the adapters see the WRAPPER's action space: the
 * per-dimension TanhScaleAdapter table is [-1, 1] in every dimension, rand(action_space) of the start phase draws in [-1, 1], and the replay ring holds scaled
 * observations.  Collection (dril_sac_collect_rollout / _continue), dril_sac_train, dril_sac_iterate, dril_sac_evaluate_agent, the monitor (raw rewards) and
 * dril_sac_normalize_* (outside the wrapper: statistics of scaled observations) honour it with no code of their own. */
int32_t dril_sac_scaling_enable(dril_sac_handle* h, int32_t on);
/* dril_agent_spaces (dril_hip.h) for a SAC handle */
int32_t dril_sac_agent_spaces(const dril_sac_handle* h, float* obs_low, float* obs_high, float* action_low, float* action_high, int32_t* scaling);
int32_t dril_sac_destroy(dril_sac_handle* h);
const char* dril_sac_last_error(const dril_sac_handle* h);

int32_t dril_sac_obs_dim(const dril_sac_handle* h);
int32_t dril_sac_action_dim(const dril_sac_handle* h);
/* Lux.parameterlength of ContinuousActorCriticLayer{QCritic}: actor + n_critics(2) Q nets + log_std */
int64_t dril_sac_param_count(const dril_sac_handle* h);
/* parameters of ONE Q network: (D+A)*H1+H1 + H1*H2+H2 + H2+1 */
int64_t dril_sac_q_param_count(const dril_sac_handle* h);

/* ---- parameters -----------------------------------------------------------------------------------------------
 * flat layout: actor_head {W1(H1xD) b1 W2(H2xH1) b2 W3(AxH2) b3}, critic_head.layer_1 {W1(H1x(D+A)) b1 W2 b2 W3(1xH2) b3},
 * critic_head.layer_2 {...} (Lux.Parallel(vcat, mlp, mlp), layer_helpers.jl:100-112), log_std(A).
 * dril_sac_set_params also re-initialises the target networks from the critics, as Agent(layer, alg::SAC) does
 * (copy_critic_parameters, sac.jl:172,191-197) */
int32_t dril_sac_set_params(dril_sac_handle* h, const float* flat, size_t n);
int32_t dril_sac_get_params(dril_sac_handle* h, float* flat, size_t n);
/* agent.aux.Q_target_parameters: {layer_1, layer_2}, 2 * q_param_count floats */
int32_t dril_sac_get_target_params(dril_sac_handle* h, float* flat, size_t n);
int32_t dril_sac_set_target_params(dril_sac_handle* h, const float* flat, size_t n);
/* agent.aux.ent_train_state.parameters.log_ent_coef[1] (init_entropy_coefficient, sac.jl:207-213) */
int32_t dril_sac_get_log_ent_coef(dril_sac_handle* h, float* value);
int32_t dril_sac_set_log_ent_coef(dril_sac_handle* h, float value);
/* fresh Adam state for the layer and for the entropy coefficient; gradient-update counter back to 0 */
int32_t dril_sac_reset_optimizer(dril_sac_handle* h);

/* ---- env ---------------------------------------------------------------------------------------------------- */
int32_t dril_sac_env_reset(dril_sac_handle* h, uint64_t seed);
int32_t dril_sac_env_observe(dril_sac_handle* h, float* host_obs /* D x E */);

/* ---- layer calls on host batches ------------------------------------------------------------------------------ */
/* action_log_prob(layer, obs, ps, st; rng): layer_methods.jl:66-76 with SquashedDiagGaussian (squashedDiagGaussian.jl:24-46).
 * noise f32 (A x B) standard normals, NULL = draw from the handle's Philox stream; actions are the squashed samples
 * tanh(mean + exp(log_std) * noise) */
int32_t dril_sac_action_log_prob(dril_sac_handle* h, const float* obs, int64_t batch, const float* noise,
                                 float* actions, float* logprobs);
/* predict_actions(agent, obs; deterministic, raw): sac.jl:215-240.  raw actions = rand / mode of the squashed
 * distribution; env actions = to_env(TanhScaleAdapter(), raw, space) = scale_to_space(tanh.(raw), space)
 * (default_adapters.jl:13-21 — the adapter applies tanh again; kept as the reference has it).  Either out pointer may be NULL */
int32_t dril_sac_predict_actions(dril_sac_handle* h, const float* obs, int64_t batch, int32_t deterministic,
                                 const float* noise, float* raw_actions, float* env_actions);
/* predict_values(layer, obs, actions, ps, st): layer_methods.jl:63-67 — q is (2 x B) column-major (vcat of the critics);
 * use_target != 0 evaluates the target networks (merge_params(ps, target_ps), sac.jl:124-127) */
int32_t dril_sac_predict_q(dril_sac_handle* h, const float* obs, const float* actions, int64_t batch,
                           int32_t use_target, float* q);

/* ---- collection: collect_rollout!(buffer, agent, alg, env, n_steps; use_random_actions) off_policy_collection.jl:117-136
 * = collect_trajectories :28-96 + push!(buffer, traj) replay_buffer.jl:98-114.  fps = steps / wall time (:126-128) */
int32_t dril_sac_collect_rollout(dril_sac_handle* h, int32_t n_steps, int32_t use_random_actions, double* fps);
/* further steps of the collection the previous dril_sac_collect_rollout / dril_sac_collect_continue call left off: for step-granular drivers that run host code
 * (callbacks' on_step, off_policy_collection.jl:43-49) between the env steps of ONE collect_trajectories.  Without NormalizeWrapperEnv the same as
 * dril_sac_collect_rollout.  Under it there is no opening observe(env): collect_rollout(1) followed by n - 1 x collect_continue(1) updates the statistics
 * n_envs * (n + 1) times and writes the bits of collect_rollout(n).  DRIL_ERR_NOT_INITIALISED when the wrapper is on and no collection is in progress (the env
 * was reset, the statistics were set or the wrapper was switched since the last collected step). */
int32_t dril_sac_collect_continue(dril_sac_handle* h, int32_t n_steps, int32_t use_random_actions, double* fps);
/* injected noise for the NEXT collect call only, f32 [step][env][A]: standard normals for policy actions, uniforms in
 * [0,1) for random actions (rand(rng, act_space) = low + u * (high - low)); NULL clears */
int32_t dril_sac_debug_set_collect_noise(dril_sac_handle* h, const float* noise, size_t count);

/* ---- collection over HOST envs (DRIL_ENV_EXTERNAL): one env step of collect_trajectories (off_policy_collection.jl:28-96) + push! (replay_buffer.jl:98-114)
 *   obs = observe(env);  dril_sac_predict_actions(h, obs, E, 0, noise, raw, env_actions)   (or rand(action_space) during the start phase, :50-53)
 *   rewards, terminateds, truncateds, infos = act!(env, env_actions);  next_obs = observe(env)
 *   dril_sac_ext_push(h, obs, stored_actions, rewards, terminateds, truncateds, next_obs, terminal_obs)
 * stored_actions (A x E) are what the reference stores: the raw squashed policy action, or the env-space random action (:72); the next observation of a
 * truncated env is its terminal_obs column (infos[i]["terminal_observation"], :75-79; may be NULL when no env was truncated).  n_envs transitions per call. */
int32_t dril_sac_ext_push(dril_sac_handle* h, const float* obs, const float* stored_actions, const float* rewards, const uint8_t* terminated,
                          const uint8_t* truncated, const float* next_obs, const float* terminal_obs);

/* ---- the same loop on DEVICE arrays (DRIL_ENV_EXTERNAL): envs whose batched arrays already live on the GPU (a simulator in torch-ROCm or CuPy, another HIP
 * library of the process).  One env step is
 *   dril_sac_ext_act_device(h, d_obs, use_random, d_noise, d_stored, d_env_actions, stream)       first half of collect_trajectories' step, :51-61
 *   ... the caller's simulator steps on `stream` ...
 *   dril_sac_ext_push_device(h, d_rewards, d_terminated, d_truncated, d_next_obs, d_terminal_obs, stream)   push! of the pending step, replay_buffer.jl:98-114
 *   dril_sac_update_enqueue(h, gradient_steps)
 * and NONE of the three waits on the host, copies across PCIe or calls a stream / event / device synchronisation; dril_sac_flush is the one drain.
 * caller_stream (a hipStream_t; NULL = the null stream) follows the contract of dril_ext_act_device (dril_hip.h): on entry the handle's stream waits for an event
 * recorded on caller_stream, before return caller_stream waits for an event recorded on the handle's stream.  Every device pointer must be memory the handle's
 * device can address, in an allocation long enough for the array, else DRIL_ERR_INVALID_ARG before anything is enqueued.  Every verb of this block returns
 * DRIL_ERR_UNSUPPORTED on a handle that was not created with DRIL_ENV_EXTERNAL.  A loop may mix these verbs with dril_sac_ext_push step by step: one ring, one set
 * of counters.
 *
 * dril_sac_ext_act_device: d_obs f32 (D x E) is kept by the handle as the pending step's observation.  use_random_actions == 0: stored / env actions are exactly
 * what dril_sac_predict_actions(h, obs, E, 0, noise, raw, env) returns for the same observations, parameters and noise; d_noise f32 (A x E) standard normals, or
 * NULL = the handle's stream (the words dril_sac_predict_actions draws with noise == NULL at the same position of the stream).  use_random_actions != 0:
 * stored = env = rand(action_space), per element low[a] + u * (high[a] - low[a]) with each operation rounded to float32 on its own; u from d_noise (uniforms in
 * [0, 1)) or the handle's stream.  Either output pointer may be NULL; the stored action is kept by the handle in both cases.  DRIL_ERR_INVALID_ARG for null obs
 * and for a second act before the push of the first. */
int32_t dril_sac_ext_act_device(dril_sac_handle* h, const float* d_obs, int32_t use_random_actions, const float* d_noise, float* d_stored_actions,
                                float* d_env_actions, void* caller_stream);
/* the pending step into the ring, with the slots and rows of dril_sac_ext_push: a truncated env stores its d_terminal_obs column as next observation (columns of
 * other envs may hold anything, NaN included, but must be readable).  d_terminal_obs == NULL states that no env was truncated in this step; a truncated flag set all
 * the same raises a sticky error word on the device which dril_sac_flush returns as DRIL_ERR_INVALID_ARG — the rows of that push STAY in the ring and hold next_obs
 * in place of the terminal observation (a ring cannot be rolled back), and the handle stays usable.  DRIL_ERR_INVALID_ARG for a push without a pending act and for
 * null rewards / flags / next_obs. */
int32_t dril_sac_ext_push_device(dril_sac_handle* h, const float* d_rewards, const uint8_t* d_terminated, const uint8_t* d_truncated, const float* d_next_obs,
                                 const float* d_terminal_obs, void* caller_stream);
/* dril_sac_predict_actions on device arrays, any batch >= 1 (chunked like the host verb); d_noise as above for deterministic == 0.  The two output pointers must
 * not both be NULL.  Does not touch the pending step: the verb of evaluation. */
int32_t dril_sac_predict_actions_device(dril_sac_handle* h, const float* d_obs, int64_t batch, int32_t deterministic, const float* d_noise, float* d_raw_actions,
                                        float* d_env_actions, void* caller_stream);
/* the launches of dril_sac_update(h, n_updates, ...) enqueued, no wait (legal on an external handle only).  Honours dril_sac_debug_set_batches like dril_sac_update.
 * The statistics rows go to a pending table on the device of DRIL_SAC_PENDING_CAPACITY rows; a call that would overflow it returns DRIL_ERR_INVALID_ARG ("flush
 * first") and enqueues nothing.  DRIL_ERR_NOT_INITIALISED on an empty ring.  k x update_enqueue(n) + flush leaves parameters, targets, optimiser state, entropy
 * coefficient, update counters and statistics bit-identical to k x dril_sac_update(n). */
#define DRIL_SAC_PENDING_CAPACITY 4096
int32_t dril_sac_update_enqueue(dril_sac_handle* h, int32_t n_updates);
/* the one drain: waits for the handle's stream, copies out the pending statistics rows in order (up to stats_capacity of them; *n_stats = rows pending; both may
 * be NULL / 0), empties the table, and returns and clears the sticky error of dril_sac_ext_push_device (DRIL_ERR_INVALID_ARG, the message names terminal_obs).
 * Legal with nothing pending. */
int32_t dril_sac_flush(dril_sac_handle* h, dril_sac_stats* stats, int64_t stats_capacity, int64_t* n_stats);
/* the Box per dimension for TanhScaleAdapter and rand(action_space) on an external handle: low / high are HOST arrays of action_dim floats.  Rewrites the table the
 * sampling kernels read, so dril_sac_predict_actions and dril_policy_from_sac_handle honour it from then on.  DRIL_ERR_INVALID_ARG for a null pointer, a non-finite
 * bound or low >= high in a dimension (the first such dimension is named). */
int32_t dril_sac_ext_set_action_bounds(dril_sac_handle* h, const float* low, const float* high);
/* counters of an external handle since create.  A struct tag only: the verb below has the same name */
struct dril_sac_ext_device_info {
    int64_t steps_device;      /* env steps pushed through dril_sac_ext_push_device */
    int64_t steps_host;        /* env steps pushed through dril_sac_ext_push */
    int64_t host_syncs;        /* host waits made INSIDE act_device / push_device / predict_actions_device / update_enqueue calls: stays 0 */
    int64_t flushes;           /* dril_sac_flush calls */
    int64_t launches;          /* kernels and device-to-device copies enqueued by act_device / push_device / predict_actions_device calls */
    int32_t pending_updates;   /* statistics rows waiting for dril_sac_flush */
    int32_t pending_capacity;  /* DRIL_SAC_PENDING_CAPACITY */
    int32_t per_dim_bounds;    /* 1 after dril_sac_ext_set_action_bounds */
    int32_t reserved[5];
};
int32_t dril_sac_ext_device_info(const dril_sac_handle* h, struct dril_sac_ext_device_info* out);

/* ---- replay buffer ---------------------------------------------------------------------------------------------- */
int64_t dril_sac_replay_size(const dril_sac_handle* h);       /* length(buffer) */
int64_t dril_sac_replay_capacity(const dril_sac_handle* h);
int32_t dril_sac_replay_copy_out(dril_sac_handle* h, int32_t which, void* host, size_t bytes);
/* empty!(buffer) followed by `count` pushes of caller transitions (tests) */
int32_t dril_sac_replay_fill(dril_sac_handle* h, int64_t count, const float* obs, const float* actions,
                             const float* rewards, const uint8_t* terminated, const uint8_t* truncated,
                             const float* next_obs);

/* ---- gradient steps ------------------------------------------------------------------------------------------------
 * n_updates x update!(agent, alg, batch) sac.jl:299-404 over batches drawn like get_data_loader (replay_buffer.jl:116-157:
 * batch_size * n_updates indices uniform with replacement).  Per step, in the reference's order: entropy-coefficient
 * step (:313-343), critic step (:345-363), actor step with zero_critic_grads! (:365-383), polyak target update
 * (:385-389).  out has n_updates entries (may be NULL) */
int32_t dril_sac_update(dril_sac_handle* h, int32_t n_updates, dril_sac_stats* out);
/* injected batches for the NEXT dril_sac_update call only: idx i64 [n_updates][B] 0-based logical replay indices;
 * noise_ent / noise_next / noise_pi f32 [n_updates][B][A] standard normals for the three action_log_prob draws of one
 * update! (entropy constant :318-325, next actions in the critic target :120, actor loss :104).  Any pointer may be NULL
 * (= device Philox stream for that input) */
int32_t dril_sac_debug_set_batches(dril_sac_handle* h, int32_t n_updates, const int64_t* idx, const float* noise_ent,
                                   const float* noise_next, const float* noise_pi);
/* gradients of the LAST gradient step in the parameter layout (n = param_count): critic_grad = d critic_loss (non-zero
 * only in the two Q nets), actor_grad = d actor_loss after zero_critic_grads! (non-zero in actor_head and log_std) */
int32_t dril_sac_get_last_grads(dril_sac_handle* h, float* critic_grad, float* actor_grad, size_t n);
/* the launches the LAST gradient step enqueued, as text: "gather=l1|plain head=fused,pre|fused,nopre|unfused dw1=fused|launch
 * l1pre=<0|1> hb=<head blocks> adam_blocks=<n> end_blocks=<n> fl_blocks=<first-layer blocks among them>" ("none" before the first
 * step).  Host state only: no launch, no device read.  The pointer stays valid until the next call on this handle */
const char* dril_sac_update_info(const dril_sac_handle* h);

/* ---- train!(agent, env, alg::SAC, max_steps) sac.jl:406-549 ----------------------------------------------------------
 * first collection of max(1, start_steps / E) steps with random actions (:438-440,485-489), then `iterations` rounds of
 * {collect train_freq steps, get_gradient_steps updates}.  stats: up to stats_capacity entries, one per gradient step;
 * fps: up to fps_capacity entries, one per iteration.  Any out pointer may be NULL */
int32_t dril_sac_train(dril_sac_handle* h, int64_t max_steps, dril_sac_stats* stats, int64_t stats_capacity,
                       int64_t* n_updates_done, double* fps, int64_t fps_capacity, int32_t* iterations_done,
                       int64_t* total_steps);

/* the loop body of train! (sac.jl:464-535) for `iterations` iterations on a handle whose env has been reset: {collect train_freq env steps with the policy,
 * get_gradient_steps updates} enqueued back to back, the stream drained once per 64 iterations (dril_sac_train runs its iterations after the first through the same
 * loop).  Bit-identical to calling dril_sac_collect_rollout(train_freq, 0) + dril_sac_update(n) per iteration.  stats: one entry per gradient step; fps: one entry per
 * iteration = env steps / HIP-event time of its collection */
int32_t dril_sac_iterate(dril_sac_handle* h, int32_t iterations, dril_sac_stats* stats, int64_t stats_capacity, double* fps,
                         int64_t fps_capacity);

/* ---- MonitorWrapperEnv(env, stats_window) around the handle's device envs (src/environment_wrappers/monitorWrapperEnv.jl) -------------------------------
 * window >= 1 switches it on (the reference's default is 100): a fresh wrapper with zero running sums and an empty window; the window the handle already has is a
 * no-op; 0 switches it off and forgets the window.  Running return / length per env are those of the RAW env rewards and accumulate over every collected step
 * (start phase and policy steps alike: dril_sac_collect_rollout, dril_sac_train, dril_sac_iterate); the finished episodes of a collection enter the window in
 * (step, env) order by one launch at the collection's end, the ring is written exactly as without the monitor.  dril_sac_env_reset zeroes the running sums and keeps
 * the window (:36-42).  DRIL_ERR_UNSUPPORTED on a DRIL_ENV_EXTERNAL handle (host envs are wrapped on the host), DRIL_ERR_INVALID_ARG for window < 0. */
int32_t dril_sac_monitor_enable(dril_sac_handle* h, int32_t window);
/* log_stats (:64-70): mean return / length over the last min(n, window) finished episodes and their number; n_episodes == 0 leaves the two means untouched.
 * DRIL_ERR_NOT_INITIALISED while the monitor is off. */
int32_t dril_sac_monitor_get_stats(dril_sac_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes);

/* ---- NormalizeWrapperEnv(env; training, norm_obs, norm_reward, clip_obs, clip_reward, gamma, epsilon) around the handle's device envs
 * (src/environment_wrappers/normalizeWrapperEnv.jl), for every observation width the handle accepts (1 .. 1024): built-in Box envs and device env plug-ins alike.
 * Statistics, `returns`, normalisation and the ring push stay on the device.  While the wrapper is on, every collection (dril_sac_collect_rollout, every iteration of
 * dril_sac_train / dril_sac_iterate) begins with observe(env) (off_policy_collection.jl:42): one update of the observation statistics over the current raw
 * observations, which are re-normalised, then per collected step act! (:139-165: returns = returns * gamma + reward, update of the return statistics, reward /
 * sqrt(ret_var + epsilon) clipped, returns of finished envs to zero, the terminal observation of a truncated env normalised with the observation statistics as they
 * are before the following observe) and observe (:123-137: batch mean / uncorrected batch variance over all envs merged by update_from_moments! :28-50 in float32,
 * (obs - mean) / sqrt(var + epsilon) clipped): obs_count grows by n_envs * (n_steps + 1) per collection, ret_count by n_envs * n_steps.  The ring holds what the
 * reference's ReplayBuffer would: normalised observation, unprocessed action, normalised reward, flags, normalised next | terminal observation; rows already in the
 * ring are never re-normalised.  training == 0 freezes both statistics and `returns`; norm_obs / norm_reward switch the two halves independently.  MonitorWrapperEnv
 * sits inside: its sums are those of raw rewards.  dril_sac_env_reset zeroes `returns`, caches the raw observation and keeps the statistics (reset! :110-121).
 * dril_sac_env_observe returns the observation the actor will see under the statistics in force and updates nothing (docs/deviations.md).
 * dril_sac_evaluate_agent runs with the statistics in force, frozen (set_training(eval_env, false) after sync_normalization_stats!, :299-309), reports raw episode
 * returns and leaves statistics, returns, the cached originals and the current observation as they were.  With the wrapper off a handle enqueues exactly the launches
 * it did before this verb existed.  The PPO handle wraps a device env plug-in through the twin family dril_normalize_* (dril_hip.h). */
typedef struct dril_sac_normalize_config {
    int32_t training, norm_obs, norm_reward;   /* 1, 1, 1 */
    float clip_obs, clip_reward;               /* 10, 10 */
    float gamma, epsilon;                      /* 0.99, 1e-8 */
    int32_t reserved;
} dril_sac_normalize_config;
/* the keyword defaults of normalizeWrapperEnv.jl:71-80 */
int32_t dril_sac_normalize_config_default(dril_sac_normalize_config* cfg);
/* a fresh wrapper (mean 0, var 1, count 0, returns 0), after which the handle's current observation is invalid so that the next collection observes through it.  A
 * configuration that differs from the handle's in `training` at most keeps the wrapper as it is — statistics, returns, current observation — and sets `training`
 * as dril_sac_normalize_set_training would (a second sac_train_ on a handle that evaluated with training off continues with its statistics).  cfg == NULL switches
 * the wrapper off (nothing to do when it is off); the next collection then observes the env itself.  DRIL_ERR_UNSUPPORTED on a DRIL_ENV_EXTERNAL handle (host envs
 * are wrapped on the host), DRIL_ERR_INVALID_ARG for a negative clip or epsilon. */
int32_t dril_sac_normalize_enable(dril_sac_handle* h, const dril_sac_normalize_config* cfg);
/* the configuration in force (`training` as dril_sac_normalize_set_training left it) */
int32_t dril_sac_normalize_get_config(dril_sac_handle* h, dril_sac_normalize_config* cfg);
/* set_training (:245-249).  This and the verbs below: DRIL_ERR_NOT_INITIALISED while the wrapper is off */
int32_t dril_sac_normalize_set_training(dril_sac_handle* h, int32_t training);
/* obs_rms / ret_rms: obs_mean, obs_var hold obs_dim floats */
int32_t dril_sac_normalize_get_stats(dril_sac_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count);
/* load_normalization_stats! / sync_normalization_stats! (:280-309): DRIL_ERR_INVALID_ARG for null pointers or negative counts */
int32_t dril_sac_normalize_set_stats(dril_sac_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count);
/* get_original_obs / get_original_rewards (:225-226): the raw observation of the latest observe (D x E) and the raw rewards of the latest act! (E); either may be NULL */
int32_t dril_sac_normalize_get_original(dril_sac_handle* h, float* obs, float* rewards);
/* env.returns (E): the discounted running return per env behind ret_rms */
int32_t dril_sac_normalize_get_returns(dril_sac_handle* h, float* returns);

/* ---- NormalizeWrapperEnv / MonitorWrapperEnv around the envs of a DRIL_ENV_EXTERNAL handle whose arrays live on the device: honoured by dril_sac_ext_act_device,
 * dril_sac_ext_push_device and dril_sac_predict_actions_device, which stay free of host waits, copies across PCIe, allocations and memsets (docs/sac.md last section).
 * The dril_sac_normalize_* / dril_sac_monitor_* verbs above keep returning DRIL_ERR_UNSUPPORTED on such a handle; every verb of this block returns
 * DRIL_ERR_UNSUPPORTED on a handle that was NOT created with DRIL_ENV_EXTERNAL (use dril_sac_normalize_enable / dril_sac_monitor_enable there).
 *
 * The caller drives collect_trajectories (off_policy_collection.jl:28-96) step by step, so it also says where one begins: dril_sac_ext_collection_begin marks the next
 * dril_sac_ext_act_device as the opening observe(env) (:43).  With the normaliser on
 *   first act after collection_begin   observe (normalizeWrapperEnv.jl:123-137): old_obs <- d_obs; with training && norm_obs the observation statistics are updated from
 *                                      the batch over the n_envs envs; the actor reads d_obs normalised with the NEW statistics and clipped (norm_obs == 0: the raw
 *                                      bits).  d_obs itself is never written
 *   any later act of the collection    no update: d_obs normalised with the statistics in force — for the same raw array what the preceding push stored as next observation
 *   an act with no collection begun since enable / set_stats / normalize_reset      DRIL_ERR_NOT_INITIALISED, the message names dril_sac_ext_collection_begin
 *   push                               act! (:139-165) then observe: old_rewards <- d_rewards; returns = returns * gamma + r, the return statistics updated, r /
 *                                      sqrt(ret_var + epsilon) clipped; returns of finished envs to 0; the terminal observation of a truncated env normalised with the
 *                                      observation statistics in force BEFORE this push's observe; d_next_obs updates the observation statistics and is normalised
 *                                      with the NEW ones; old_obs <- d_next_obs.  Ring row: normalised pending observation, stored action as kept, normalised reward,
 *                                      flags, normalised terminal | next observation.  Rows of d_terminal_obs of envs that were not truncated are never read into the
 *                                      ring or a sum.  d_terminal_obs == NULL with a truncated flag: the sticky error of dril_sac_flush as without the wrapper, the
 *                                      row holds the normalised d_next_obs, the statistics updates are kept
 *   dril_sac_predict_actions_device    normalises with the statistics in force and never updates them, whatever `training` says; touches nothing else of the wrapper
 * obs_count grows by n_envs per opening act and per push, ret_count by n_envs per push: n_envs * (n + 1) and n_envs * n per collection of n steps.  training == 0
 * freezes both statistics; `returns` then changes only by the reset of finished envs.  MonitorWrapperEnv sits inside the normaliser: running return (float32, step
 * order) and length of RAW rewards per env; finished episodes enter the window in (step, env) order — the window is brought up to date by dril_sac_flush and
 * dril_sac_ext_monitor_get_stats before they drain (and, inside a push, once per block of buffered steps).  With both wrappers off the handle enqueues exactly what
 * it did before these verbs existed.  While a wrapper is on the host verb dril_sac_ext_push returns DRIL_ERR_UNSUPPORTED. */
/* a fresh wrapper (mean 0, var 1, counts 0, returns 0); the same configuration up to `training` keeps statistics and returns and sets `training`; NULL switches the
 * wrapper off.  Every array of the wrapper is allocated here.  DRIL_ERR_INVALID_ARG for a negative or NaN clip / epsilon and while an act is pending */
int32_t dril_sac_ext_normalize_enable(dril_sac_handle* h, const dril_sac_normalize_config* cfg);
/* the contracts of the dril_sac_normalize_* verbs of the same names; DRIL_ERR_NOT_INITIALISED while the wrapper is off; the getters drain the handle's stream */
int32_t dril_sac_ext_normalize_get_config(dril_sac_handle* h, dril_sac_normalize_config* cfg);
int32_t dril_sac_ext_normalize_set_training(dril_sac_handle* h, int32_t training);
int32_t dril_sac_ext_normalize_get_stats(dril_sac_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count);
int32_t dril_sac_ext_normalize_set_stats(dril_sac_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count);
int32_t dril_sac_ext_normalize_get_original(dril_sac_handle* h, float* obs, float* rewards);
int32_t dril_sac_ext_normalize_get_returns(dril_sac_handle* h, float* returns);
/* the wrapper's half of reset! (:110-121): returns <- 0, statistics kept; enqueued behind caller_stream (as in the device verbs), no host wait */
int32_t dril_sac_ext_normalize_reset(dril_sac_handle* h, void* caller_stream);
/* the next dril_sac_ext_act_device opens a collect_trajectories call.  A host flag: launches nothing; a no-op while the normaliser is off */
int32_t dril_sac_ext_collection_begin(dril_sac_handle* h);
/* MonitorWrapperEnv(env, window): the window in force again is a no-op, 0 switches it off; DRIL_ERR_INVALID_ARG for window < 0 and while an act is pending */
int32_t dril_sac_ext_monitor_enable(dril_sac_handle* h, int32_t window);
/* dril_sac_monitor_get_stats for such a handle: collects what is outstanding, then drains; DRIL_ERR_NOT_INITIALISED while the monitor is off */
int32_t dril_sac_ext_monitor_get_stats(dril_sac_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes);
/* A struct tag only: the verb below has the same name */
struct dril_sac_ext_wrap_info {
    int32_t normalize_on, monitor_on, monitor_window, reserved0;
    int64_t launches_act;      /* launches the wrappers ADDED to dril_sac_ext_act_device calls since create, against the same calls with the wrappers off */
    int64_t launches_push;     /* ... to dril_sac_ext_push_device calls */
    int64_t allocations;       /* always 0, by construction: no path of act / push / predict allocates (every array of a wrapper is made by its enable verb), so
                                  nothing counts here; the field keeps the struct the shape of dril_ext_wrap_info, whose handle has a path that grows a scratch array */
    int64_t reserved[3];
};
int32_t dril_sac_ext_wrap_info(const dril_sac_handle* h, struct dril_sac_ext_wrap_info* out);

/* ---- evaluate_agent(agent, env; n_eval_episodes, deterministic) (src/evaluation.jl:54-143) with the handle's actor on the handle's envs --------------------
 * reset (env e seeded seed + e), then predict_actions(; deterministic) -> act! -> observe until the first n_eval_episodes episodes have finished, taken in
 * (step, env) order.  deterministic: mode(d) = tanh(mean) (squashedDiagGaussian.jl:48-50) through TanhScaleAdapter; otherwise a sample, its noise from env e's
 * collection stream under `seed`.  dril_eval_stats as in dril_hip.h (Julia mean / corrected std, NaN std for one episode; n_steps = the 1-based env step at which
 * the last counted episode finished).  episode_rewards / episode_lengths (n_eval_episodes entries each) may be NULL.
 * The episode accounting lives on the device (running sums per env, finished episodes appended to an event list); the host looks at the list's counter once every
 * K enqueued env steps (K = min(episode_len, 32); DRIL_SAC_EVAL_POLL=<k> read at create overrides; 1 = step by step).  The result is the same for every K.
 * Evaluation has no side effect on training: it never writes the replay ring, parameters, targets, optimiser state, update counters or the monitor's window, and the
 * env side of the handle (state, step / episode counters, the noise stream's position, the current observation, the monitor's running sums) is set aside before and
 * put back after, on error paths too — the reference evaluates on a separate env object; one handle is agent and envs together.
 * DRIL_ERR_UNSUPPORTED on a DRIL_ENV_EXTERNAL handle (evaluate host envs on the host with dril_sac_predict_actions) and when no episode finishes within the time
 * limits n_eval_episodes can take; DRIL_ERR_INVALID_ARG for n_eval_episodes < 1 or out == NULL. */
int32_t dril_sac_evaluate_agent(dril_sac_handle* h, int32_t n_eval_episodes, int32_t deterministic, uint64_t seed,
                                dril_eval_stats* out, float* episode_rewards, int32_t* episode_lengths);

/* ---- collect_trajectory(agent, env; max_steps, deterministic) (src/utils/trajectory_utils.jl:3-49) with the handle's actor on the handle's envs ----------------
 * The SAC form of dril_collect_trajectory_device (dril_hip.h; docs/sac.md "Trajectories"): dril_traj_options, dril_traj_info, dril_traj_options_default, the layouts
 * of the five output arrays and the end-flag bits are those of that verb.  Envs 0..M-1 record their FIRST episode after the call's own reset (has_seed ? seed : the
 * seed in force; env e gets seed + e).  Row t < L is the ORIGINAL observation before step t + 1: never normalised, and under ScalingWrapperEnv (the scaled kinds,
 * or dril_sac_scaling_enable on a plug-in) mapped back with unscale_from_unit.  The agent sees the wrapper's observation: scaled, and normalised with the statistics
 * of dril_sac_normalize_enable FROZEN for the call whatever its training flag.  Action row t is mode(d) = tanh(mean) (deterministic) or a sample, through
 * to_env(TanhScaleAdapter), then unscale! under ScalingWrapperEnv: the value the env's physics receives.  Reward row t is the env's raw reward.  The episode ends at
 * its first terminated || truncated or after max_steps steps, the episode's end taking precedence; row L is observe(env) of the env that did not auto-reset, in the
 * wrapper's scale unless final_original.  With deterministic = 0 the draws are those of dril_sac_evaluate_agent on the same seed, which are those of a collection
 * after dril_sac_env_reset(seed).  The trajectory of env m does not depend on M, on poll_steps or on the other envs.
 * The call leaves nothing behind: it never writes the replay ring, parameters, targets, optimiser state, update counters, the monitor's window or the normaliser's
 * statistics / returns / old_obs, and it sets aside and puts back what dril_sac_evaluate_agent sets aside and puts back, on error paths too.
 * poll_steps = 0: K of dril_sac_evaluate_agent (DRIL_SAC_EVAL_POLL honoured).  reserved[DRIL_TRAJ_OPT_PERSISTENT] is accepted and ignored (there is one form);
 * info.reserved[DRIL_TRAJ_INFO_PATH] is 0.
 * DRIL_ERR_NOT_INITIALISED: null handle.  DRIL_ERR_INVALID_ARG: null options or output array, n_trajectories outside 1..n_envs, negative max_steps or poll_steps, a
 * recording whose device arrays exceed 1 GiB.  DRIL_ERR_UNSUPPORTED: DRIL_ENV_EXTERNAL (the envs live with the caller: loop there over dril_sac_predict_actions).
 * All of them are decided before anything is enqueued. */
int32_t dril_sac_trajectory_capacity(const dril_sac_handle* h, const dril_traj_options* o, int32_t* capacity);
int32_t dril_sac_collect_trajectory(dril_sac_handle* h, const dril_traj_options* o,
                                    float* observations,  /* (D, Tcap+1, M) column-major, as dril_collect_trajectory_device */
                                    float* actions,       /* f32 (A, Tcap, M); rows >= lengths[m] are 0 */
                                    float* rewards,       /* (Tcap, M) */
                                    int32_t* lengths,     /* (M): steps taken */
                                    uint8_t* end_flags,   /* (M): bit0 terminated, bit1 truncated, bit2 stopped by max_steps */
                                    dril_traj_info* info  /* may be NULL; the five arrays may not */);

/* ---- measurement: accumulated HIP-event milliseconds since the last reset --------------------------------------------- */
int32_t dril_sac_profile_get(dril_sac_handle* h, double* collect_ms, int64_t* collect_steps, double* update_ms,
                             int64_t* updates);
int32_t dril_sac_profile_reset(dril_sac_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* DRIL_SAC_H */
