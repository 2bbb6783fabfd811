/*
 * dril_hip.h — C ABI of libdril_hip.so: the MI355X (gfx950) implementation of
 * DRiL.jl's vectorised rollout-collection + PPO-update hot path.
 *
 * The reference (KristianHolme/DRiL.jl) is pure Julia and has no FFI; the seam
 * this library plugs into is Julia dispatch.  Every entry point
 * below names the reference function it stands in for (paths relative to the
 * reference checkout).  A Julia `ccall` shim (dril.jl_amd/julia/DRiLHIP.jl) and
 * a Python ctypes mirror (dril.jl_amd/host.py) both bind exactly these symbols.
 *
 * Conventions
 *   - every function returns int32_t status, 0 == DRIL_OK; no C++ exception
 *     crosses the ABI; dril_last_error() returns the message of the last failure
 *   - the library owns all device memory and the handle; the CALLER owns every
 *     host pointer and must keep it alive for the duration of the call only
 *   - a handle is not thread-safe; different handles may be used concurrently
 *   - all calls are synchronous at return (the handle's HIP stream is drained)
 *     unless documented otherwise
 *   - arrays use the reference's memory layout: observations (D x n) column-major
 *     (each observation's D floats contiguous, src/spaces.jl:259), weights
 *     (out x in) column-major exactly as Lux.Dense stores them
 *   - the device rollout buffer is TIME-MAJOR: flat index n = t * n_envs + env
 *     (the reference buffer is trajectory-major in completion order,
 *     src/buffers/rollout_buffer.jl:70-80; DESIGN.md §3 gives the index map)
 */
#ifndef DRIL_HIP_H
#define DRIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRIL_ABI_VERSION 2u   /* 2: n_hidden / hidden[] / activation (any-depth MLPs, relu) */

typedef struct dril_handle dril_handle;

enum dril_status {
    DRIL_OK = 0,
    DRIL_ERR_INVALID_ARG = 1,
    DRIL_ERR_HIP = 2,
    DRIL_ERR_RCCL = 3,
    DRIL_ERR_NAN_IN_GRADS = 4, /* mirrors `@assert !nested_has_nan(grads)` src/algorithms/ppo.jl:213-214 */
    DRIL_ERR_NOT_INITIALISED = 5,
    DRIL_ERR_UNSUPPORTED = 6
};

enum dril_env_kind {
    DRIL_ENV_CARTPOLE = 0, /* CartPole-v1: D=4, Discrete(2)            */
    DRIL_ENV_PENDULUM = 1, /* Pendulum-v1: D=3, Box(-2,2) 1-dim action */
    /* ScalingWrapperEnv(PendulumEnv()) (src/environment_wrappers/scalingWrapperEnv.jl:15-49): every sub-env is wrapped, so the agent sees
     * observation_space = action_space = Box(-1, 1): observe returns (obs - low) * 2/(high - low) - 1 (:71-74,93-98) and act! maps the
     * action back with (a + 1) / (2/(high - low)) + low (:76-79,110-113) before the physics; the affine maps are fused into the env kernels */
    DRIL_ENV_PENDULUM_SCALED = 2,
    DRIL_ENV_MOUNTAINCAR = 3,            /* MountainCar-v0: D=2 (position, velocity), Discrete(3), reward -1/step, goal at 0.5, limit 200 */
    DRIL_ENV_MOUNTAINCAR_CONTINUOUS = 4, /* MountainCarContinuous-v0: D=2, Box(-1,1), reward 100 at the goal (0.45) - 0.1 a^2, limit 999 */
    /* any AbstractParallelEnv that lives on the HOST (the caller's own Julia envs, interfaces/environments.jl:21-39): observations come in and
     * actions go out once per env step (dril_ext_act / dril_ext_record / dril_ext_finish below), everything else of the path — policy forward,
     * sampling, rollout buffer, bootstrap values, GAE, the PPO update — runs on the device.  Spaces are given by ext_obs_dim / ext_action_dim /
     * ext_discrete; any hidden_dims = [h1, h2] up to 1024.  The env verbs (dril_env_*), dril_collect_rollout, dril_train, dril_evaluate_agent
     * and the wrappers fused into the env kernels (norm_*, monitor_window) belong to the device envs and return DRIL_ERR_UNSUPPORTED here */
    DRIL_ENV_EXTERNAL = 5,
    /* Acrobot-v1 (Gymnasium "book" dynamics, one RK4 step of 0.2 s per env step): D=6 (cos t1, sin t1, cos t2, sin t2, w1, w2), Discrete(3) torques
     * -1/0/+1, reward -1 per step (0 on reaching the height), limit 500.  A device env like the others; hidden_dims [64,64] run the fused kernels (four
     * first-layer k-steps for its six observation dims; the update on the pair / persistent f16-piece kernels like the other envs, dW1 through a third piece image),
     * hidden 128 / 256 the wide fused kernels, any other hidden_dims the generic kernels */
    DRIL_ENV_ACROBOT = 6,
    /* ScalingWrapperEnv(MountainCarContinuousEnv()): observations Box((-1.2, -0.07), (0.6, 0.07)) scaled to Box(-1, 1), actions Box(-1, 1) mapped back by the same
     * affine formulas (scalingWrapperEnv.jl:71-79); every kernel that does not touch the simulator is shared with DRIL_ENV_MOUNTAINCAR_CONTINUOUS */
    DRIL_ENV_MOUNTAINCAR_CONTINUOUS_SCALED = 7,
    /* a DEVICE ENV PLUG-IN: the caller's own env, written against include/device/dril_env_plugin.h (reset / observe / step of one env as device functions), compiled on
     * its own into a gfx950 code object (hipcc --genco) and loaded with the HIP module API by dril_create_with_env_module below.  Spaces, bounds and the default
     * time limit come from the code object's descriptor; its three kernels stand where env_reset_kernel / env_observe_kernel / env_step_kernel stand for a built-in
     * kind, so every device-env verb works: dril_env_*, dril_collect_rollout (step-granular: policy launches + ONE env launch per step), dril_train,
     * dril_evaluate_agent, monitor_window.  Always on the generic kernels (any hidden_dims).  NormalizeWrapperEnv arrives as a verb on the created handle,
     * dril_normalize_enable below, for any observation width; cfg.norm_obs / cfg.norm_reward at create stay refused (they size the built-in envs' 8-dim tables), and
     * so do the dril_ext_* verbs.  SAC on a Box plug-in is available through dril_sac_create_with_env_module (dril_sac.h).  dril_create and
     * dril_sac_create themselves refuse this kind: they have no code object to load.  docs/external_envs.md */
    DRIL_ENV_MODULE = 8
};

/* ids for dril_buffer_copy_out / dril_buffer_copy_in (fields of RolloutBuffer,
 * src/buffers/buffer_types.jl:3-15, plus the per-step flags the reference keeps
 * in Trajectory, buffer_types.jl:17-26) */
enum dril_buffer_id {
    DRIL_BUF_OBSERVATIONS = 0, /* f32  (D, N)                                  */
    DRIL_BUF_ACTIONS = 1,      /* i32 (1, N) discrete | f32 (A, N) continuous   */
    DRIL_BUF_REWARDS = 2,      /* f32 (N)                                       */
    DRIL_BUF_ADVANTAGES = 3,   /* f32 (N)                                       */
    DRIL_BUF_RETURNS = 4,      /* f32 (N)                                       */
    DRIL_BUF_LOGPROBS = 5,     /* f32 (N)                                       */
    DRIL_BUF_VALUES = 6,       /* f32 (N)                                       */
    DRIL_BUF_FLAGS = 7,        /* u8 (N): bit0 terminated, bit1 truncated       */
    DRIL_BUF_BOOTSTRAP = 8,    /* f32 (N): V(terminal_observation), valid where truncated */
    DRIL_BUF_LAST_VALUES = 9   /* f32 (n_envs): V(obs after the last step)      */
};

/* kernels whose HIP-event timings dril_profile_get reports */
enum dril_kernel_id {
    DRIL_K_ROLLOUT = 0,
    DRIL_K_GAE = 1,
    DRIL_K_ADV_MOMENTS = 2,
    DRIL_K_PPO_GRAD = 3,
    DRIL_K_GRAD_REDUCE = 4,
    DRIL_K_ADAM = 5,
    DRIL_K_ALLREDUCE = 6,
    DRIL_K_PACK_RECORDS = 7,   /* pack_records_kernel: the rollout buffer's SoA fields -> one 32-byte record per sample and net, once per update */
    DRIL_K_EXPLAINED_VAR = 8,  /* explained_var_kernel: the four sums of ppo.jl:256 over the whole buffer */
    DRIL_K_COUNT = 9           /* grows with the library: loop to dril_kernel_count() */
};

/* Plain-C mirror of `PPO` (src/algorithms/ppo.jl:25-40), the layer kwargs
 * (src/layers/layer_constructors.jl:3-11,55-56), `NormalizeWrapperEnv` kwargs
 * (src/environment_wrappers/normalizeWrapperEnv.jl:71-80) and the env ctor
 * kwargs used by the reference's benchmarks (benchmark/bench_utils.jl:14,20). */
typedef struct dril_config {
    uint32_t abi_version;      /* must be DRIL_ABI_VERSION */
    int32_t env_kind;          /* enum dril_env_kind */
    int32_t n_envs;            /* E on THIS rank */
    int32_t n_steps;           /* T (PPO.n_steps) */
    int32_t hidden1, hidden2;  /* hidden_dims = [hidden1, hidden2], 1..1024 each, when n_hidden == 0 (below): [64,64], [128,128], [256,256] with tanh run the
                                * fused kernels, every other shape (and DRIL_ENV_EXTERNAL) the generic layer-by-layer kernels */
    int32_t episode_len;       /* max_steps kwarg: 500 CartPole-v1, 200 Pendulum-v1 */
    int32_t fixed_length_episodes; /* 1: termination disabled (synthetic bench episodes) */
    int32_t action_start;      /* Discrete(n, start): src/spaces.jl:157-164 */

    float gamma, gae_lambda, clip_range;
    float clip_range_vf;  int32_t has_clip_range_vf;   /* Union{T,Nothing} */
    float ent_coef, vf_coef;
    float max_grad_norm;  int32_t has_max_grad_norm;
    float target_kl;      int32_t has_target_kl;
    int32_t normalize_advantage;
    int64_t batch_size;        /* GLOBAL minibatch size B (over all ranks) */
    int32_t epochs;
    float learning_rate;
    float adam_beta1, adam_beta2, adam_eps; /* Optimisers.Adam defaults + eps=1e-5, ppo.jl:64-66 */
    float log_std_init;

    int32_t norm_obs, norm_reward, norm_training; /* NormalizeWrapperEnv; all 0 = no wrapper */
    float clip_obs, clip_reward, norm_gamma, norm_epsilon;

    uint64_t seed;             /* env i (0-based, global index) is seeded seed + i, wrapper_utils.jl:39-44 */
    int32_t device;            /* HIP device ordinal */
    int32_t rank, world_size;  /* data-parallel position; global env index = rank*n_envs + local */
    int32_t profile_events;    /* k >= 1: bracket hot kernels with HIP events (dril_profile_get); the per-optimiser-step kernels at every k-th launch */
    int32_t monitor_window;    /* MonitorWrapperEnv(env, stats_window): > 0 tracks episode returns/lengths (monitorWrapperEnv.jl:15-24); 0 = no wrapper */
    /* DRIL_ENV_EXTERNAL only (ignored otherwise): observation_space = Box of ext_obs_dim floats (<= 1024); action_space =
     * Discrete(ext_action_dim, action_start) when ext_discrete, else Box(ext_action_low, ext_action_high) of ext_action_dim floats (<= 64);
     * the bounds feed ClampAdapter (default_adapters.jl:4-11); low >= high = no clamp */
    int32_t ext_obs_dim, ext_action_dim, ext_discrete;
    float ext_action_low, ext_action_high;
    /* ActorCriticLayer(...; hidden_dims, activation) in full (src/layers/layer_constructors.jl:6-10,55-56; get_mlp layer_helpers.jl:27-57 builds
     * Dense(in => h_1, act), ..., Dense(h_{n-1} => h_n, act), Dense(h_n => out)): n_hidden = length(hidden_dims) in 1..4 with hidden[0..n_hidden-1]
     * (1..1024 each), or 0 = the two-layer form hidden1 / hidden2 above.  activation: 0 tanh (the reference's default), 1 relu, 2 sigmoid, 3 elu (alpha 1), 4 leakyrelu (0.01), 5 softplus, 6 gelu (the tanh form), 7 swish (NNlib's definitions; the generic kernels).  Every shape other
     * than two equal tanh layers of 64 / 128 / 256 runs the generic kernels.  Parameter layout per net: {W_1 b_1 ... W_{n+1} b_{n+1}} */
    int32_t n_hidden, hidden[4], activation;
    int32_t reserved[1];
} dril_config;

/* per-iteration means returned by dril_ppo_update; field names follow the
 * `learn_stats` NamedTuple, src/algorithms/ppo.jl:301-312 */
typedef struct dril_ppo_stats {
    float entropy_loss, policy_loss, value_loss, approx_kl_div, clip_fraction;
    float loss, grad_norm, explained_variance, entropy, ratio_first; /* ratio of epoch1/batch1, ppo.jl:209-212 */
    int32_t n_updates;         /* optimiser steps actually applied */
    int32_t early_stopped;     /* 1 if target_kl stopped the loops, ppo.jl:235-238 */
    int32_t nan_or_inf;        /* 1 if a gradient contained NaN/Inf (status is DRIL_ERR_NAN_IN_GRADS too) */
    int32_t f32_path;          /* which kernels produced THIS update (was `reserved`): 0 the default ones; 1 redone on the exact-f32 kernels after an f16-piece kernel
                                * left f16's range; 2 run directly on the exact-f32 kernels (latched after repeated redos, or a W2 entry out of range) */
} dril_ppo_stats;

/* The fused kernels' default arithmetic (fp32-equivalent products from two f16 pieces per operand) holds fp32's PRECISION but f16's RANGE.  The reference asks no range of
 * its user (ppo.jl:213-214 only asserts finiteness), so leaving it is handled inside the library and merely COUNTED here:
 *   retries              updates taken back and redone on the exact-f32 kernels because an f16-piece step met a non-finite gradient (2x the update's time, each)
 *   direct_updates       updates run on the exact-f32 kernels at once: after 2 consecutive retries the next 16 updates (then one update probes f16 again), or max|W2| >= 350
 *   persistent_fallbacks updates of the two-workgroup persistent kernel (batch_size <= 64) redone on the per-step kernels because its workgroups were not co-resident
 *   latch_updates_left   updates the latch still covers; forward_exact_f32: 1 while rollout / policy forwards run the f32-MFMA kernels (max_abs_w2 >= 350 or DRIL_GRAD_VARIANT=0) */
typedef struct dril_f32_fallback {
    int64_t retries, direct_updates, persistent_fallbacks;
    int32_t latch_updates_left, forward_exact_f32;
    float max_abs_w2; int32_t reserved;
} dril_f32_fallback;

/* fill cfg with the reference defaults: PPO() ppo.jl:26-39, hidden_dims [64,64]
 * layer_constructors.jl:55, NormalizeWrapperEnv kwargs normalizeWrapperEnv.jl:71-80 (disabled) */
int32_t dril_config_default(dril_config* cfg, int32_t env_kind);

/* ---- lifetime ------------------------------------------------------------ */
/* RolloutBuffer(...) ppo.jl:112-115 + Agent(layer, alg) ppo.jl:42-62 (device state only) */
int32_t dril_create(const dril_config* cfg, dril_handle** out);
/* the same for cfg->env_kind == DRIL_ENV_MODULE: code_object_path names a gfx950 code object built from include/device/dril_env_plugin.h (a plain ELF or a
 * clang-offload-bundle).  A null path, an unreadable file and a file that is neither are DRIL_ERR_INVALID_ARG before any HIP call; then the module is loaded, its
 * descriptor copied out and checked (plug-in ABI number, size of the kernel argument block, S 1..64 (a world: agents 2..16, S 1..256), D 1..1024, A 1..64, time limit) and its three kernels looked
 * up: a mismatch is DRIL_ERR_UNSUPPORTED with a message, before anything of the module is launched.  cfg->episode_len == 0 takes the descriptor's time limit;
 * Box bounds per dimension come from the descriptor (ClampAdapter).  The module is unloaded by dril_destroy and on every failing path of this call. */
int32_t dril_create_with_env_module(const dril_config* cfg, const char* code_object_path, dril_handle** out);
/* what a code object says about itself — the host needs the spaces to build the ActorCriticLayer before a handle exists */
typedef struct dril_env_module_info {
    uint32_t plugin_abi;                                   /* DRIL_ENV_PLUGIN_ABI the code object was compiled against */
    int32_t state_dim, obs_dim, action_dim, discrete;      /* S, D, A (Discrete: number of actions), 1 = Discrete(A, action_start) / 0 = Box */
    int32_t episode_len;                                   /* default time limit */
    float action_low[64], action_high[64];                 /* Box bounds, entries 0 .. action_dim-1 (continuous) */
    char name[64];
} dril_env_module_info;
/* loads the code object on `device`, reads and checks its descriptor, unloads it again; same checks and statuses as dril_create_with_env_module */
int32_t dril_env_module_describe(const char* code_object_path, int32_t device, dril_env_module_info* out);
/* the same record of a live handle (DRIL_ERR_UNSUPPORTED for a handle of another env kind) */
int32_t dril_env_module_info_of(const dril_handle* h, dril_env_module_info* out);
/* The OBSERVATION SPACE a plug-in declares (static constexpr float obs_low[D], obs_high[D] in the env; observation_space of interfaces/environments.jl): low / high
 * take obs_dim floats each (either may be NULL), *declared = 1.  A code object that declares none (or was built before the space existed) gives *declared = 0 and
 * -inf / +inf in every dimension.  The struct above is unchanged by this; the checks and statuses are those of dril_env_module_describe.  The _of form reports the
 * env's own space of a live handle, whether ScalingWrapperEnv is on or not (DRIL_ERR_UNSUPPORTED for a handle of another env kind). */
int32_t dril_env_module_obs_space(const char* code_object_path, int32_t device, float* low, float* high, int32_t* declared);
int32_t dril_env_module_obs_space_of(const dril_handle* h, float* low, float* high, int32_t* declared);
/* WORLDS (include/device/dril_env_world.h, DRIL_ENV_PLUGIN_WORLD): a code object whose descriptor says agents = N in 2..16 holds a multi-agent world — N agents, one
 * shared state of state_dim floats (up to 256) and one joint step; the device form of MultiAgentParallelEnv (multiAgentParallelEnv.jl).  The library sees agent i of
 * world w as ROW w N + i, and every verb works per row as for a classic plug-in: n_envs counts rows and must be a multiple of N (per rank), else
 * dril_create_with_env_module returns DRIL_ERR_INVALID_ARG.  World w is seeded seed0 + w N (the global row index of its agent 0); action noise stays keyed by row.
 * *agents is N for a world and 1 for a classic plug-in; dril_env_module_info keeps its layout (state_dim is the world's, obs_dim / action_dim are per agent).
 * On a world handle: the env state array stays n_envs x state_dim floats on the device (N times what the worlds need), world w at float offset w state_dim;
 * dril_env_get_state / dril_env_set_state move the W = n_envs / N world states (W x state_dim floats) and the per-row step counts, and dril_env_set_state refuses
 * step counts that differ between the rows of one world (DRIL_ERR_INVALID_ARG).  dril_collect_trajectory_device records whole worlds: n_trajectories must be a multiple
 * of N.  DRIL_ERR_UNSUPPORTED with a message, before anything is launched: dril_scaling_enable, dril_rollout_fused_enable, dril_sac_create_with_env_module;
 * dril_evaluate_fused_info answers available = 0 (evaluation and trajectories run on path 0).  The checks and statuses of the path form are those of
 * dril_env_module_describe; the _of form is DRIL_ERR_UNSUPPORTED for a handle of another env kind. */
int32_t dril_env_module_agents(const char* code_object_path, int32_t device, int32_t* agents);
int32_t dril_env_module_agents_of(const dril_handle* h, int32_t* agents);
/* ScalingWrapperEnv(env) (scalingWrapperEnv.jl) around every env of a device env plug-in handle: on != 0 makes the env side launch the plug-in's
 * dril_env_plugin_observe_scaled / dril_env_plugin_step_scaled kernels where it launched observe / step — no launch is added per env step.  The agent-facing
 * spaces become Box(-1, 1): raw actions are clamped to [-1, 1] and unscaled into the env's own bounds, every observation the env side hands out (observe, the next
 * observation, the terminal observation of a truncated env) is scaled from the declared space; rewards, flags, counters and the monitor's sums are the env's own.
 * Every device-env verb honours it (dril_env_reset / _observe / _step, dril_collect_rollout, dril_train, dril_evaluate_agent); NormalizeWrapperEnv
 * (dril_normalize_enable) sits OUTSIDE it, so its statistics are those of scaled observations.
 * LEGAL between create and the first dril_env_reset of the handle only: afterwards it is DRIL_ERR_INVALID_ARG and nothing changes (observations already handed
 * out would change their meaning).  DRIL_ERR_UNSUPPORTED, with a message that says what to do, for: a handle that is not a plug-in handle (the built-in scaled
 * kinds stay the way to scale a built-in env; a host env is wrapped on the host), a Discrete plug-in, a plug-in that declares no observation space, an
 * observation or action dimension whose bounds are not finite with low < high (the first such dimension is named), a code object without the two kernels,
 * a world.
 * dril_env_module_info_of keeps reporting the env's own action bounds; dril_agent_spaces reports what the agent sees. */
int32_t dril_scaling_enable(dril_handle* h, int32_t on);
/* the spaces the agent of a plug-in handle sees: obs_low / obs_high (obs_dim floats) and action_low / action_high (action_dim floats; untouched for a Discrete
 * plug-in), any of them NULL; *scaling = 1 and Box(-1, 1) throughout under ScalingWrapperEnv, else the declared observation space and the env's own action bounds */
int32_t dril_agent_spaces(const dril_handle* h, float* obs_low, float* obs_high, float* action_low, float* action_high, int32_t* scaling);
/* The FUSED ROLLOUT of a device env plug-in (include/device/dril_env_rollout.h): a code object built with DRIL_ENV_PLUGIN_ROLLOUT(Env) holds a collection kernel
 * with the env inlined — observe, critic and actor forward, the draw, the transition and the buffer rows of all n_steps steps in ONE launch, a workgroup per tile
 * of envs, no grid barrier.  on != 0: from now on dril_collect_rollout and dril_train launch it (dril_env_plugin_rollout_scaled while dril_scaling_enable is on)
 * where they issued the policy launches and the plug-in's step kernel per env step; GAE, the update, the env verbs and dril_evaluate_agent are unchanged and a
 * collection of either kind may follow the other.  Legal at any time between collections; off is the default.
 * Numerics: the fused forward is plain f32 FMA with k ascending, the step-granular one the bf16 x 3-piece MFMA contractions — two f32-equivalent arithmetics, so
 * values, log-probabilities and Gaussian actions of the two paths agree like device and oracle do, not to the bit; noise words, flags for equal states, counters,
 * monitor bookkeeping and the buffer layout are identical.  An env's rows do not depend on n_envs or on the env's position (batch invariance).
 * Speed: the fused path removes the per-step launches; whether it also wins at very large n_envs is a measurement (docs/external_envs.md section 11).
 * DRIL_ERR_UNSUPPORTED, each with a message that says what to do and the handle left as it was, for: a handle that is not a plug-in handle; a code object without
 * the kernel; a rollout descriptor of another ABI number or argument-block size; a hidden layer or observation wider than the plug-in's compiled
 * DRIL_ENV_ROLLOUT_MAX_WIDTH; a handle on which dril_normalize_enable is on (running statistics couple all envs at every step).  dril_normalize_enable on a
 * handle whose fused path is on is refused likewise. */
typedef struct dril_fused_rollout_info {
    int32_t available;                 /* the code object has a usable rollout kernel for this handle's net */
    int32_t enabled;
    int32_t tile, threads, max_width;  /* of the plug-in's compile; 0 without a rollout descriptor */
    int32_t reserved;
    int64_t last_collection_launches;  /* launch calls the last dril_collect_rollout enqueued for collect_trajectories on this plug-in handle (either path; 0 before) */
    char reason[256];                  /* why it is not available ("" when it is) */
} dril_fused_rollout_info;
int32_t dril_rollout_fused_enable(dril_handle* h, int32_t on);
int32_t dril_rollout_fused_info(const dril_handle* h, dril_fused_rollout_info* out);
/* The ONE-LAUNCH COLLECTION of a normalising built-in handle (cfg.norm_obs / cfg.norm_reward on a built-in env kind, docs/normalized_rollout.md).  By default such a
 * handle collects step-granular: three launches per env step, because NormalizeWrapperEnv's running statistics couple all envs at every step.  Up to max_envs = 128
 * envs fit in one workgroup, which couples them through LDS: on != 0 makes dril_collect_rollout and dril_train run collect_trajectories as the opening observe and
 * ONE launch of rollout_norm_kernel, whatever n_steps is.  Opt-in, off by default, legal at any time between collections; the step verbs, the dril_norm_* verbs, the
 * evaluation and trajectory verbs are untouched and may run between two such collections, and a collection of either kind may follow the other.
 * Equality: observations, actions, rewards, log-probabilities, flags, the running statistics and their counts, env state and the monitor's figures are bit-equal to
 * the step-granular collection of the same handle (the batch moments are summed by the same tree); values, last values and bootstrap values agree to 1e-6 (the
 * critic's two forward forms, as between the step-granular launches and rollout_duo_kernel).
 * A collection while the forward is the exact-f32 one (max |W2| >= 350, dril_f32_fallback_info) runs step-granular for that call and is counted.
 * DRIL_ERR_UNSUPPORTED, each with a message that says what to do and the handle left as it was, for: a handle that is not a normalising built-in handle (plug-ins have
 * dril_normalize_enable, external handles dril_ext_normalize_enable); a generic or wide net, hidden 32; n_envs > max_envs; world_size > 1 or a ready communicator
 * (the batch moments are an all-reduce per env step); DRIL_FORCE_STEPWISE / DRIL_FORCE_GENERIC. */
typedef struct dril_norm_rollout_report {
    int32_t available;                 /* dril_norm_rollout_enable(h, 1) would be accepted */
    int32_t enabled;
    int32_t max_envs;                  /* the envs one workgroup couples: 128 */
    int32_t last_collection_path;      /* of the last collection of a normalising built-in handle: 1 = rollout_norm_kernel, 0 = step-granular */
    int64_t last_collection_launches;  /* launch calls that collection enqueued for collect_trajectories (the opening observe and the monitor's window included, GAE not) */
    int64_t total_stepwise_fallbacks;  /* collections of an enabled handle that ran step-granular because the forward was the exact-f32 one */
    char reason[256];                  /* why it is not available ("" when it is) */
} dril_norm_rollout_report;
int32_t dril_norm_rollout_enable(dril_handle* h, int32_t on);
int32_t dril_norm_rollout_info(const dril_handle* h, dril_norm_rollout_report* out);
/* The ONE-LAUNCH UPDATE of a generic handle (docs/generic_update.md).  A handle on the layer-by-layer kernels — a device env plug-in, DRIL_ENV_EXTERNAL, a built-in env
 * with hidden_dims / an activation the fused kernels are not built for, DRIL_FORCE_GENERIC — runs every optimiser step of dril_ppo_update as a chain of 3 nh + 6
 * dependent launches (nh hidden layers).  on != 0 makes dril_ppo_update and dril_train run the whole
 * epoch x minibatch loop inside ppo_update_generic_small_kernel, one workgroup, steps_per_launch optimiser steps per launch.  Opt-in, off by default, legal at any time
 * between updates; enable(h, 0) returns to the per-step route exactly, and an update of either route may follow the other.
 * Measured (docs/generic_update.md): 1.26 - 1.51 x the per-step route's speed at batch_size <= 32, 0.75 - 0.92 x (slower) at 64, where a minibatch is two sample
 * tiles; the report says so in faster_up_to_batch.
 * Arithmetic: f32 throughout, every sum in an order fixed by the launch shape — two runs give the same bits, however the steps are cut into launches.  The route
 * agrees with the per-step route like the device agrees with the oracle (f32 rounding in another order), not to the bit.
 * DRIL_ERR_UNSUPPORTED, each with a message that says what to do and the handle left as it was, for: a fused-shape handle (its update already is one launch);
 * world_size > 1, a ready communicator or DRIL_FORCE_ALLREDUCE; batch_size outside min_batch .. max_batch; DRIL_NO_PERSISTENT_UPDATE or DRIL_GRAD_VARIANT set; a net
 * beyond the caps below (the kernel keeps parameters, gradients and a sample tile's activations in one CU's LDS). */
typedef struct dril_update_fused_report {
    int32_t available;                 /* dril_update_fused_enable(h, 1) would be accepted */
    int32_t enabled;
    int32_t max_width, max_obs_dim, max_action_dim, max_params, max_hidden_layers;   /* the kernel's caps: 64, 16, 8, 11 264, 4 */
    int32_t min_batch, max_batch;      /* 2, 64: what the kernel holds and the verb accepts */
    int32_t faster_up_to_batch;        /* 32: the largest batch_size at which the route measured faster than the per-step route on every admitted shape
                                          (docs/generic_update.md, "Measured"); from 33 to max_batch it is accepted and measured SLOWER */
    int32_t reserved;
    int32_t last_update_path;          /* of the last dril_ppo_update: 1 = ppo_update_generic_small_kernel, 0 = per step */
    int64_t last_update_launches;      /* launches of the update kernel in that update (path 1), else 0 */
    int64_t steps_per_launch;          /* optimiser steps one launch runs at most */
    char reason[256];                  /* why it is not available ("" when it is) */
} dril_update_fused_report;
int32_t dril_update_fused_enable(dril_handle* h, int32_t on);
int32_t dril_update_fused_info(const dril_handle* h, dril_update_fused_report* out);
/* The FUSED EVALUATION of a device env plug-in (include/device/dril_env_evaluate.h): a code object built with DRIL_ENV_PLUGIN_EVALUATE(Env) holds a second, optional
 * kernel with the env inlined — K env steps of observe, (frozen) normalisation, actor forward, mode or draw and the transition in ONE launch, a workgroup per tile
 * of envs, no grid barrier — with a descriptor and an ABI number of its own (the rollout's are untouched).  It is path 2 of dril_evaluate_agent_device and
 * dril_collect_trajectory_device, taken where the options ask for the persistent form (reserved[DRIL_EVAL_OPT_PERSISTENT] / reserved[DRIL_TRAJ_OPT_PERSISTENT] = 1);
 * nothing switches a handle to it.  This verb says whether such a request would be served on this handle, and why not: a handle that is not a plug-in handle; a code
 * object without the kernel; an evaluation descriptor of another ABI number or argument-block size; a hidden layer or observation wider than the plug-in's compiled
 * DRIL_ENV_ROLLOUT_MAX_WIDTH; dril_scaling_enable on without the _scaled kernel.  A request on a handle where it is not available runs path 0, never an error. */
typedef struct dril_fused_evaluate_info {
    int32_t available;                 /* the code object has a usable evaluation kernel for this handle's net */
    int32_t tile, threads, max_width;  /* of the plug-in's compile; 0 without an evaluation descriptor */
    char reason[256];                  /* why it is not available ("" when it is) */
} dril_fused_evaluate_info;
int32_t dril_evaluate_fused_info(const dril_handle* h, dril_fused_evaluate_info* out);
int32_t dril_destroy(dril_handle* h);
/* message of the last failing call on h (or of the last failing create when h == NULL) */
const char* dril_last_error(const dril_handle* h);
/* drains the handle's stream */
int32_t dril_synchronize(dril_handle* h);

/* ---- shapes ---------------------------------------------------------------*/
int32_t dril_obs_dim(const dril_handle* h);     /* D  */
int32_t dril_action_dim(const dril_handle* h);  /* A: n for Discrete, dims for Box */
int32_t dril_is_discrete(const dril_handle* h);
int64_t dril_param_count(const dril_handle* h); /* Lux.parameterlength, layer_lux.jl */

/* ---- parameters: agent.train_state.parameters <-> flat f32 -----------------
 * layout: actor_head {W1(H1xD) b1 W2(H2xH1) b2 W3(AoutxH2) b3}, critic_head {W1 b1 W2 b2 W3(1xH2) b3},
 * then log_std(A) for Box actions (layer_lux.jl:4-39); every W column-major (out x in).  With n_hidden layers: {W_1 b_1 ... W_{n+1} b_{n+1}} per head */
int32_t dril_set_params(dril_handle* h, const float* flat, size_t n);
int32_t dril_get_params(dril_handle* h, float* flat, size_t n);
/* fresh optimiser state (load_policy_params_and_state! rebuilds Adam, ppo.jl:77-94) */
int32_t dril_reset_optimizer(dril_handle* h);
/* the optimiser state itself — what Lux.Training.TrainState carries as optimizer_state between train! calls (ppo.jl:52-53,239; Optimisers.Adam leaf state
 * (mt, vt, betat)): first and second moments in the parameter layout of dril_get_params, the running products (beta1^t, beta2^t) and the number of applied
 * steps.  The handle keeps this state between dril_train / dril_ppo_update calls; get / set move it with a TrainState from one handle to another (another
 * env, a re-created handle).  n = dril_param_count; beta_powers = 2 floats. */
int32_t dril_get_optimizer_state(dril_handle* h, float* m, float* v, size_t n, float* beta_powers, int64_t* steps);
int32_t dril_set_optimizer_state(dril_handle* h, const float* m, const float* v, size_t n, const float* beta_powers, int64_t steps);
/* Optimisers.adjust!(train_state, lr) ppo.jl:155-156 */
int32_t dril_set_learning_rate(dril_handle* h, float lr);

/* ---- env verbs (MultiThreadedParallelEnv, src/environment_wrappers/multithreadedParallelEnv.jl) */
/* Random.seed!(env, seed) wrapper_utils.jl:39-44 followed by reset!(env) :12-17 */
int32_t dril_env_reset(dril_handle* h, uint64_t seed);
/* observe(env) :19-25 (NormalizeWrapperEnv.observe normalizeWrapperEnv.jl:123-137 when enabled:
 * updates obs statistics when update_stats != 0); host_obs is (D x E) column-major */
int32_t dril_env_observe(dril_handle* h, float* host_obs, int32_t update_stats);
/* act!(env, actions) :47-74 with auto-reset; actions i32(E) | f32(A x E) are ENV-space
 * (already passed through to_env, src/adapters/default_adapters.jl:4-11,34-38);
 * terminal_obs (D x E) is written only for truncated envs; any out pointer may be NULL */
int32_t dril_env_step(dril_handle* h, const void* host_actions, float* rewards, uint8_t* terminated,
                      uint8_t* truncated, float* terminal_obs);
/* raw simulator state: CartPole (x, x_dot, theta, theta_dot), Pendulum (theta, theta_dot), + step counter */
int32_t dril_env_get_state(dril_handle* h, float* state /* S x E; a world handle: S x W, W = E / agents */, int32_t* step_count /* E */);
int32_t dril_env_set_state(dril_handle* h, const float* state, const int32_t* step_count);
/* RunningMeanStd fields, normalizeWrapperEnv.jl:8-19 (save/load :261-297) */
int32_t dril_norm_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count,
                            float* ret_mean, float* ret_var, int64_t* ret_count);
int32_t dril_norm_set_stats(dril_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count,
                            float ret_mean, float ret_var, int64_t ret_count);
/* get_original_obs(env) / get_original_rewards(env) (normalizeWrapperEnv.jl:220-222): the un-normalised observations (D x E) of the last
 * observe and the un-normalised rewards (E) of the last act! through the step-granular verbs; either pointer may be NULL */
int32_t dril_norm_get_original(dril_handle* h, float* obs, float* rewards);
/* The three verbs above on a DRIL_ENV_MODULE handle: DRIL_ERR_UNSUPPORTED while its wrapper is off (as before dril_normalize_enable existed); with the wrapper on
 * they forward to dril_normalize_get_stats / _set_stats / _get_original below, so host code written for the built-in envs reads a wrapped plug-in unchanged. */

/* ---- NormalizeWrapperEnv(env; training, norm_obs, norm_reward, clip_obs, clip_reward, gamma, epsilon) around a DEVICE ENV PLUG-IN (DRIL_ENV_MODULE), for every
 * observation width a plug-in may have (1 .. 1024).  The verb family reads like dril_sac_normalize_* (dril_sac.h).  Built-in envs are wrapped at create
 * (cfg.norm_*) and are not touched by it.  With the wrapper on, every device-env verb honours it with the reference's semantics:
 *   dril_collect_rollout / dril_train   the opening observe updates the observation statistics over the current raw observations (trajectory.jl:32); then per step
 *       act! (normalizeWrapperEnv.jl:139-165: returns = returns * gamma + reward, update of the return statistics, reward / sqrt(ret_var + epsilon) clipped, the
 *       terminal observation of a truncated env normalised with the observation statistics as they are before the following observe, returns of finished envs to
 *       zero) and observe (:123-137: batch mean / uncorrected batch variance over all envs merged by update_from_moments! :28-50 in float32, (obs - mean) /
 *       sqrt(var + epsilon) clipped).  Row t of the rollout buffer holds the normalised observation and reward, DRIL_BUF_BOOTSTRAP of a truncated step is
 *       V(normalised terminal observation), DRIL_BUF_LAST_VALUES is V of the normalised last observation.  obs_count grows by n_envs * (n_steps + 1) per rollout
 *       and ret_count by n_envs * n_steps.  Two launches more per env step than the unwrapped plug-in path; nothing leaves the device.
 *   dril_env_observe(update_stats) / dril_env_step   observe / act! of the wrapper; dril_env_reset zeroes `returns`, caches the raw observation and keeps the
 *       statistics (reset! :110-121).
 *   MonitorWrapperEnv (monitor_window) sits inside: its sums are those of raw rewards.
 *   dril_evaluate_agent   runs with the statistics in force, frozen, reports RAW episode returns and leaves statistics, `returns` and the cached originals as they
 *       were (the envs themselves are reset, as by every dril_evaluate_agent).
 *   world_size > 1   the batch moments cover every env of the job: one all-reduce of 2 obs_dim + 2 doubles per statistics update, the identical merge with
 *       n = world_size * n_envs on every rank (the counts grow by that n), statistics bit-identical across ranks.
 * training == 0 freezes both statistics and `returns`; norm_obs / norm_reward switch the two halves independently.  With the wrapper off a handle enqueues exactly
 * the launches it did before this family existed. */
typedef struct dril_normalize_config {
    int32_t training, norm_obs, norm_reward;   /* 1, 1, 1 */
    float clip_obs, clip_reward;               /* 10, 10 */
    float gamma, epsilon;                      /* 0.99, 1e-8 */
    int32_t reserved;
} dril_normalize_config;
/* the keyword defaults of normalizeWrapperEnv.jl:71-80 */
int32_t dril_normalize_config_default(dril_normalize_config* cfg);
/* a fresh wrapper: mean 0, var 1, counts 0, returns 0.  A configuration that differs from the handle's in `training` at most keeps the wrapper as it is —
 * statistics and returns — and sets `training`.  cfg == NULL switches the wrapper off (nothing to do when it is off).  DRIL_ERR_INVALID_ARG for a negative clip or
 * epsilon; DRIL_ERR_UNSUPPORTED on a handle that is not DRIL_ENV_MODULE: a built-in env is wrapped with cfg.norm_obs / cfg.norm_reward at create, the envs of
 * DRIL_ENV_EXTERNAL are wrapped on the host. */
int32_t dril_normalize_enable(dril_handle* h, const dril_normalize_config* cfg);
/* the configuration in force (`training` as dril_normalize_set_training left it).  This and the verbs below: DRIL_ERR_NOT_INITIALISED while the wrapper is off on a
 * plug-in handle, DRIL_ERR_UNSUPPORTED on any other handle */
int32_t dril_normalize_get_config(dril_handle* h, dril_normalize_config* cfg);
/* set_training (:245-249) */
int32_t dril_normalize_set_training(dril_handle* h, int32_t training);
/* obs_rms / ret_rms: obs_mean, obs_var hold obs_dim floats; any out pointer may be NULL */
int32_t dril_normalize_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count);
/* load_normalization_stats! (:280-297): DRIL_ERR_INVALID_ARG for null pointers or negative counts */
int32_t dril_normalize_set_stats(dril_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count);
/* get_original_obs / get_original_rewards (:220-222): the raw observation of the latest observe (D x E) and the raw rewards of the latest act! (E); either may be NULL */
int32_t dril_normalize_get_original(dril_handle* h, float* obs, float* rewards);
/* env.returns (E): the discounted running return per env behind ret_rms */
int32_t dril_normalize_get_returns(dril_handle* h, float* returns);

/* MonitorWrapperEnv: mean return / length over the last `monitor_window` finished episodes (log_stats, monitorWrapperEnv.jl:64-70)
 * and the number of episodes currently in the window; rewards are the RAW env rewards (the monitor sits inside the normaliser) */
int32_t dril_monitor_get_stats(dril_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes);

/* ---- policy (src/layers/layer_forward.jl, layer_methods.jl) on host batches -- */
/* layer(obs, ps, st) -> (actions, values, logprobs): layer_forward.jl:3-13 / :30-39.
 * noise: f64(B) uniforms for Categorical.rand (categorical.jl:47-52) or f32(A x B) normals for
 * DiagGaussian.rand (diagGaussian.jl:13-17); NULL = draw from the handle's Philox stream.
 * actions are the RAW policy actions (pre-adapter, trajectory.jl:48) */
int32_t dril_policy_forward(dril_handle* h, const float* obs, int64_t batch, const void* noise,
                            void* actions, float* values, float* logprobs);
/* evaluate_actions(layer, obs, actions, ps, st): layer_methods.jl:28-55 */
int32_t dril_evaluate_actions(dril_handle* h, const float* obs, const void* actions, int64_t batch,
                              float* values, float* logprobs, float* entropy);
/* predict_actions(layer, obs, ps, st; deterministic, rng): layer_methods.jl:3-26 — mode(d) when deterministic (argmax of the Categorical,
 * categorical.jl:42-44; the mean of the DiagGaussian, diagGaussian.jl:45-47), else rand(d) with `noise` as in dril_policy_forward.
 * actions are RAW policy actions (evaluate_agent passes them through to_env, evaluation.jl:92-93) */
int32_t dril_predict_actions(dril_handle* h, const float* obs, int64_t batch, int32_t deterministic, const void* noise, void* actions);
/* predict_values(layer, obs, ps, st): layer_methods.jl:57-61 */
int32_t dril_predict_values(dril_handle* h, const float* obs, int64_t batch, float* values);

/* ---- rollout over HOST envs (DRIL_ENV_EXTERNAL): collect_trajectories, trajectory.jl:22-78, one call pair per env step ------------
 * for step in 1:n_steps
 *     obs = observe(env)                                   # caller
 *     dril_ext_act(h, obs, raw, env_actions)               # get_action_and_values :41 + to_env :42; obs/actions/values/logprobs -> buffer :46-51
 *     rewards, terminateds, truncateds, infos = act!(env, env_actions)     # caller
 *     dril_ext_record(h, rewards, terminateds, truncateds, terminal_obs)   # rewards/flags -> buffer; V(terminal_observation) for truncated envs :57-61
 * end
 * dril_ext_finish(h, observe(env))                         # V(new_obs) for unfinished trajectories :65-70, compute_advantages!, returns
 * obs / terminal_obs / last_obs are (D x E) column-major host arrays; raw_actions (stored, pre-adapter) and env_actions (ClampAdapter /
 * DiscreteAdapter applied) are i32(E) | f32(A x E), either may be NULL; terminal_obs may be NULL when no env was truncated; only the
 * columns of truncated envs are read.  dril_debug_set_noise injects the sampling noise of the next n_steps dril_ext_act calls. */
int32_t dril_ext_act(dril_handle* h, const float* obs, void* raw_actions, void* env_actions);
int32_t dril_ext_record(dril_handle* h, const float* rewards, const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs);
int32_t dril_ext_finish(dril_handle* h, const float* last_obs);
/* env steps recorded since the last dril_ext_finish (0 .. n_steps) */
int32_t dril_ext_steps(const dril_handle* h);

/* ---- the same rollout over envs whose arrays already live on the DEVICE (a batched simulator in PyTorch-ROCm / CuPy, another HIP library of the process) ----
 * The *_device verbs take DEVICE memory of the handle's device in the layouts of the host verbs: obs / terminal_obs / last_obs f32 (D x E) column-major,
 * actions i32 (E) | f32 (A x E), rewards f32 (E), flags u8 (E).  They share the host verbs' state machine (a rollout may mix both, step by step) and fill the
 * same buffer: observations, raw actions, values and log-probabilities of a step are the host verb's bits.
 * caller_stream: the hipStream_t on which the caller produced the inputs and will consume the outputs (NULL = the null stream).  On entry the library records an
 * event on it and makes the handle's stream wait; before returning it records an event on its own stream and makes caller_stream wait for that: the caller may
 * enqueue its env step on the actions at once.  dril_ext_act_device and dril_ext_record_device never wait on the host — no stream, event or device
 * synchronisation and no blocking copy, truncation steps included; dril_ext_finish_device enqueues V(last_obs) and GAE and drains ONCE: the one
 * synchronisation of a rollout, and where deferred errors surface.
 *   act:    d_raw_actions (pre-adapter, as stored) and d_env_actions (ClampAdapter applied on the device: per dimension after dril_ext_set_action_bounds, else
 *           the scalar ext_action_low / ext_action_high; low >= high = not clamped; Discrete: equal to the raw actions); either may be NULL.
 *   record: d_terminal_obs != NULL: V of ALL E columns is computed (one critic forward) and kept where the env was truncated; the other columns may hold
 *           anything, finite or not, but must be readable memory of E x D floats.  d_terminal_obs == NULL states that no env was truncated in this step and
 *           skips that forward; a truncated flag set all the same raises a sticky error on the device, which dril_ext_finish_device returns as
 *           DRIL_ERR_INVALID_ARG after its drain — the rollout then counts as not collected (dril_ext_steps == 0).
 * Statuses: those of the host verbs for null pointers and call order; DRIL_ERR_INVALID_ARG, before anything is enqueued, for a pointer that
 * hipPointerGetAttributes does not report as accessible from the handle's device (or whose allocation is shorter than the array); DRIL_ERR_UNSUPPORTED on a
 * handle that is not DRIL_ENV_EXTERNAL. */
int32_t dril_ext_act_device(dril_handle* h, const float* d_obs, void* d_raw_actions, void* d_env_actions, void* caller_stream);
int32_t dril_ext_record_device(dril_handle* h, const float* d_rewards, const uint8_t* d_terminated, const uint8_t* d_truncated, const float* d_terminal_obs, void* caller_stream);
int32_t dril_ext_finish_device(dril_handle* h, const float* d_last_obs, void* caller_stream);
/* dril_predict_actions on device arrays with the adapter applied (evaluate_agent over such an env): d_obs f32 (D x batch); noise from the handle's stream, as
 * dril_predict_actions with noise == NULL; d_raw_actions / d_env_actions as in dril_ext_act_device (not both NULL).  Ordered on caller_stream like the verbs above;
 * no host wait except when a larger batch than any before makes the library grow its scratch arrays. */
int32_t dril_predict_actions_device(dril_handle* h, const float* d_obs, int64_t batch, int32_t deterministic, void* d_raw_actions, void* d_env_actions, void* caller_stream);
/* the ClampAdapter's Box per dimension: low / high are HOST arrays of action_dim floats (both NULL: back to the scalar pair of the config).  Honoured by
 * dril_ext_act as well from then on.  DRIL_ERR_INVALID_ARG for a Discrete action space or one NULL pointer, DRIL_ERR_UNSUPPORTED on a handle that is not external */
int32_t dril_ext_set_action_bounds(dril_handle* h, const float* low, const float* high);
/* what the current (or, between rollouts, the last) rollout of an external handle did.  A struct tag only: the verb below has the same name */
struct dril_ext_device_info {
    int32_t steps_device;      /* env steps recorded through dril_ext_record_device */
    int32_t steps_host;        /* env steps recorded through dril_ext_record */
    int32_t host_syncs;        /* host-side waits the library made inside act / record calls: 0 for the device verbs */
    int32_t per_dim_bounds;    /* 1 after dril_ext_set_action_bounds */
    int64_t launches;          /* kernel launches enqueued by act / record / finish calls */
    int32_t reserved[4];
};
int32_t dril_ext_device_info(const dril_handle* h, struct dril_ext_device_info* out);

/* ---- NormalizeWrapperEnv / MonitorWrapperEnv around the envs of a DRIL_ENV_EXTERNAL handle, honoured by the DEVICE-ARRAY verbs (docs/external_envs.md section 10, "Wrappers on device-resident arrays").
 * The env arrays stay the caller's; the wrappers are the library's and sit between them and the rollout buffer, so nothing leaves the device:
 *   dril_ext_act_device(d_obs)      observe (normalizeWrapperEnv.jl:123-137): old_obs <- the raw observation; with training && norm_obs the observation statistics
 *       are updated from the batch over the E envs; row t of DRIL_BUF_OBSERVATIONS holds the observation normalised with the NEW statistics and clipped (the raw bits
 *       with norm_obs == 0), and the forward reads that row.
 *   dril_ext_record_device(...)     act! (:139-165): old_rewards <- the raw rewards; with training && norm_reward returns = returns * gamma + reward and the return
 *       statistics are updated; row t of DRIL_BUF_REWARDS holds reward / sqrt(ret_var + epsilon) clipped; `returns` of finished envs go to 0; the terminal
 *       observation of a truncated env is normalised with the observation statistics in force (before the following observe) into an array of the handle's own —
 *       d_terminal_obs is not written — and DRIL_BUF_BOOTSTRAP is V of that; rows of envs that were not truncated are never selected.
 *   dril_ext_finish_device(d_last_obs)   one more observe; DRIL_BUF_LAST_VALUES = V(normalised last observation).  obs_count grows by n_envs * (n_steps + 1) per
 *       rollout and ret_count by n_envs * n_steps.  A rollout that finish reports as discarded (the sticky terminal_obs error) keeps its statistics updates: they
 *       were enqueued.
 *   dril_predict_actions_device     evaluation: normalises with the statistics in force and never updates them, whatever `training` says; nothing else of the
 *       wrapper is touched.
 *   MonitorWrapperEnv sits inside the normaliser: per-env running return (float32, step order) and length of RAW rewards; an episode enters the window where
 *       terminated | truncated, in (step, env) order, when dril_ext_finish_device collects the rollout's rows.
 * With a wrapper on, act / record still make no host wait, no allocation and no memset (dril_ext_device_info.host_syncs stays 0): per verb at most two launches more
 * than without (batch moments, then one apply kernel that also replaces the unwrapped verb's device-to-device copy of the observation); the monitor's window costs
 * finish the two launches of its collector.  With both wrappers off a handle enqueues exactly what it did before these verbs existed.
 * training == 0: statistics are frozen and `returns` changes only by the reset of finished envs.
 * Refusals (the handle is left as it was): DRIL_ERR_UNSUPPORTED on a handle that is not DRIL_ENV_EXTERNAL (built-in envs: cfg.norm_* / cfg.monitor_window; plug-ins:
 * dril_normalize_enable) and with world_size > 1 (single rank only); DRIL_ERR_INVALID_ARG for a negative or NaN clip / epsilon, and for an enable inside a rollout
 * (dril_ext_steps != 0 or an act without its record).  While either wrapper is on, the HOST verbs dril_ext_act / dril_ext_record / dril_ext_finish return
 * DRIL_ERR_UNSUPPORTED: a wrapped rollout is device verbs only.  dril_normalize_* and cfg.norm_* / cfg.monitor_window stay refused on an external handle. */
/* a fresh wrapper (mean 0, var 1, counts 0, returns 0); the same configuration up to `training` keeps statistics and returns and sets `training`; NULL: off.
 * Every array of the wrapper is allocated here */
int32_t dril_ext_normalize_enable(dril_handle* h, const dril_normalize_config* cfg);
/* as the dril_normalize_* verbs of the same names; DRIL_ERR_NOT_INITIALISED while the wrapper is off.  The getters drain the handle's stream */
int32_t dril_ext_normalize_get_config(dril_handle* h, dril_normalize_config* cfg);
int32_t dril_ext_normalize_set_training(dril_handle* h, int32_t training);
int32_t dril_ext_normalize_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count);
int32_t dril_ext_normalize_set_stats(dril_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count);
int32_t dril_ext_normalize_get_original(dril_handle* h, float* obs, float* rewards);
int32_t dril_ext_normalize_get_returns(dril_handle* h, float* returns);
/* the wrapper's half of reset! (:111-121): returns <- 0, statistics kept.  Enqueued on the handle's stream behind everything it has enqueued; no host wait.
 * caller_stream: as in the device verbs (the handle's stream waits for it first) */
int32_t dril_ext_normalize_reset(dril_handle* h, void* caller_stream);
/* MonitorWrapperEnv(env, stats_window): 0 switches it off; the window in force again keeps it.  Between rollouts only */
int32_t dril_ext_monitor_enable(dril_handle* h, int32_t stats_window);
/* what dril_monitor_get_stats reports for a device env; DRIL_ERR_NOT_INITIALISED while the monitor is off */
int32_t dril_ext_monitor_get_stats(dril_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes);
/* A struct tag only: the verb below has the same name */
struct dril_ext_wrap_info {
    int32_t normalize_on;      /* 1 while dril_ext_normalize_enable is in force */
    int32_t monitor_on;        /* 1 while dril_ext_monitor_enable is in force */
    int32_t monitor_window;
    int32_t reserved0;
    int64_t launches_act;      /* launches the wrappers ADDED to the act calls of the current (or last) rollout, against the same calls with the wrappers off */
    int64_t launches_record;   /* ... to its record calls */
    int64_t launches_finish;   /* ... to its finish call */
    int64_t allocations;       /* device allocations a wrapper made inside act / record / finish / predict since the last enable: stays 0 over rollouts (a
                                  dril_predict_actions_device batch larger than n_envs grows a scratch array once and is counted) */
    int64_t reserved[2];
};
int32_t dril_ext_wrap_info(const dril_handle* h, struct dril_ext_wrap_info* out);

/* ---- rollout --------------------------------------------------------------- */
/* collect_rollout!(buffer, agent, alg, env): rollout_buffer.jl:46-90 =
 * collect_trajectories trajectory.jl:22-78 + compute_advantages! :80-102 + returns :87.
 * fps = steps / wall time of the collection part, rollout_buffer.jl:60-64 */
int32_t dril_collect_rollout(dril_handle* h, double* fps);
/* injected sampling noise for the NEXT dril_collect_rollout call only: f64 (E x T) uniforms
 * [t*E+e] (discrete) or f32 (A x E x T) normals; NULL clears */
int32_t dril_debug_set_noise(dril_handle* h, const void* noise, size_t count);
int32_t dril_buffer_copy_out(dril_handle* h, int32_t which, void* host, size_t bytes);
int32_t dril_buffer_copy_in(dril_handle* h, int32_t which, const void* host, size_t bytes);
/* compute_advantages! over the device buffer as it stands (rewards/values/flags/bootstrap/last_values) */
int32_t dril_compute_gae(dril_handle* h);
/* stand-alone GAE on caller arrays, time-major [t*E+e]; no handle state is used or changed */
int32_t dril_gae(int32_t n_envs, int32_t n_steps, float gamma, float gae_lambda, const float* rewards,
                 const float* values, const uint8_t* flags, const float* bootstrap, const float* last_values,
                 float* advantages, float* returns);

/* ---- PPO update -------------------------------------------------------------- */
/* the epoch x minibatch loop of train!, ppo.jl:188-264 (DataLoader shuffle, loss :365-407 + gradient,
 * NaN asserts :213-214, nested_norm/nested_scale! :216-232, target_kl :235-238, Adam :239,
 * explained_variance :256, per-iteration means :257-264) */
int32_t dril_ppo_update(dril_handle* h, dril_ppo_stats* out);
/* see dril_f32_fallback above; dril_f32_retries = its `retries` alone (-1 for a null handle).  A healthy run on normalised data shows 0 / 0 */
int64_t dril_f32_retries(const dril_handle* h);
int32_t dril_f32_fallback_info(const dril_handle* h, dril_f32_fallback* out);
/* injected DataLoader order: perm[e*N + p] = 0-based buffer index at position p of epoch e
 * (ppo.jl:188-195); NULL = device-generated pseudo-random bijection per epoch */
int32_t dril_debug_set_permutation(dril_handle* h, const int64_t* perm, size_t count);
/* DEBUG / TEST: the per-optimiser-step rows of the last dril_ppo_update, as the device wrote them: rows x 16 floats, row s = {policy loss, value loss, entropy loss,
 * clip fraction, approx KL, entropy, mean ratio, loss, gradient norm, applied, non-finite, KL stop, 4 unused}; rows must not exceed that update's epochs x minibatches. */
int32_t dril_debug_get_step_stats(dril_handle* h, float* out, size_t rows);
/* (alg::PPO)(layer, ps, st, batch) ppo.jl:365-407 and its gradient (Lux.Training.compute_gradients,
 * ppo.jl:207) on a caller minibatch; stats7 = policy_loss, value_loss, entropy_loss, clip_fraction,
 * approx_kl_div, entropy, ratio; grads has dril_param_count entries, same layout as the params.
 * normalises advantages per ppo.jl:350-363 when cfg.normalize_advantage */
int32_t dril_ppo_loss_grad(dril_handle* h, const float* obs, const void* actions, const float* advantages,
                           const float* returns, const float* old_logprobs, const float* old_values,
                           int64_t batch, float* loss, float* stats7, float* grads);
/* one optimiser step from caller gradients: nested_norm, nested_scale!, Adam (ppo.jl:216-239);
 * returns the pre-clip norm */
int32_t dril_apply_gradients(dril_handle* h, const float* grads, size_t n, float* grad_norm);

/* ---- evaluate_agent (src/evaluation.jl:54-143) --------------------------------------------- */
typedef struct dril_eval_stats {
    double mean_reward, std_reward, mean_length, std_length;   /* Julia mean / std (corrected) over the collected episodes */
    int32_t n_episodes, n_steps;                               /* episodes collected, env steps taken */
} dril_eval_stats;
/* reset!(env); then predict_actions(agent, obs; deterministic) -> act! -> observe until the first n_eval_episodes episodes have
 * finished, taken in (step, env) order (evaluation.jl:90-124).  deterministic: mode(d) — argmax for Categorical (categorical.jl:42-44),
 * the mean for DiagGaussian (diagGaussian.jl:45-47).  With MonitorWrapperEnv on (cfg.monitor_window > 0) episode returns use the RAW
 * rewards, like infos[i]["episode"]["r"]; otherwise the rewards as the wrappers deliver them.  episode_rewards / episode_lengths
 * (n_eval_episodes entries each) may be NULL. */
int32_t dril_evaluate_agent(dril_handle* h, int32_t n_eval_episodes, int32_t deterministic, dril_eval_stats* out,
                            float* episode_rewards, int32_t* episode_lengths);

/* The same evaluation ON THE DEVICE, and leaving nothing behind (docs/evaluation.md).  The episode accounting runs on the device: every env's thread adds its
 * reward in float32 and in step order and appends {step, env, return, length} to one list where its episode ends; the host looks at the list's 4-byte counter
 * once per K env steps, sorts the copied slots by (step, env) and takes n_eval_episodes — the numbers dril_evaluate_agent returns, whatever K is and whichever
 * path ran.  Two paths: a persistent evaluate kernel (a wave keeps 32 envs in registers for K steps, the actor's weights in LDS) for the built-in kinds on the
 * fused shapes without a normaliser, and step-granular launches with a small accounting launch for every other device-env handle (generic shapes, cfg.norm_*,
 * plug-ins with or without dril_scaling_enable / dril_normalize_enable / the fused rollout).  On request (reserved[DRIL_EVAL_OPT_PERSISTENT] = 1) a cfg.norm_*
 * handle on a fused shape takes the persistent kernel too: it reads the frozen statistics as an argument and returns the same numbers.  On the same request a
 * plug-in handle whose code object carries a usable evaluation kernel (dril_evaluate_fused_info) takes PATH 2: that kernel, K env steps per launch, and one
 * accounting launch of the library over the K rows of raw rewards and flag bytes it leaves — 2 launches per K env steps, with dril_scaling_enable, with
 * dril_normalize_enable (frozen statistics read as an argument; raw returns, the rule for plug-ins) and with the monitor on.  Its forward is the fused rollout's plain
 * f32 FMA chain, path 0's the bf16 x 3-piece contractions: two f32-equivalent arithmetics, so paths 0 and 2 agree like device and oracle do, not to the bit.
 * A normaliser is FROZEN for the call whatever its training flag (set_training(env, false), evaluation of a training env; docs/deviations.md).
 * The call brings its own reset and puts back what it writes, on error paths too: env state, step counts, episode and noise-stream counters, the seed in force,
 * `returns`, the E-sized per-step arrays, the statistics' buffers and parities, and whether the envs count as reset.  The monitor's sums / window / meta are not
 * written at all (its launches are not made during the call), nor are the call counter of the policy noise, the rollout buffer, parameters, optimiser state, update
 * and profile counters; no all-reduce is enqueued (every rank of a data-parallel job evaluates its own envs).
 * DRIL_ERR_NOT_INITIALISED: null handle.  DRIL_ERR_INVALID_ARG: n_eval_episodes < 1, null o / out, poll_steps < 0.  DRIL_ERR_UNSUPPORTED: DRIL_ENV_EXTERNAL; no
 * episode finishes within ceil(n / n_envs) + 1 time limits and one poll interval. */
typedef struct dril_eval_options {
    int32_t n_eval_episodes, deterministic;
    uint64_t seed; int32_t has_seed;     /* 0: the handle's current env seed; env e is reset with seed + global env index */
    int32_t poll_steps;                  /* 0: the library's default K; >= 1: look at the counter every poll_steps env steps */
    int32_t force_step_granular;         /* 1: never take the persistent kernel (tests, A/B); wins over the request below, as DRIL_FORCE_STEPWISE=1 at create does */
    int32_t reserved[3];                 /* reserved[DRIL_EVAL_OPT_PERSISTENT]: the opt-in request for the persistent kernel.  0 (default): today's rule — the kernel
                                          * where no normaliser is on.  1: the kernel wherever it can run, cfg.norm_obs / cfg.norm_reward handles included: the FROZEN
                                          * statistics in force are passed to it as an argument and only read.  Same numbers on either path.  A plug-in handle with a
                                          * usable evaluation kernel (dril_evaluate_fused_info) takes path 2.  Generic shapes, other plug-ins and DRIL_ENV_EXTERNAL keep
                                          * their answers (path 0, or the refusal), never an error because of the request.  The other words: 0 */
} dril_eval_options;
#define DRIL_EVAL_OPT_PERSISTENT 0       /* index into dril_eval_options.reserved */
typedef struct dril_eval_info {
    int32_t path;                        /* what ran: 0 step-granular launches + device accounting, 1 persistent evaluate kernel, 2 a plug-in's fused evaluation kernel */
    int32_t launches, steps_enqueued, events, reserved[4];   /* launch calls of the loop, env steps enqueued, events the device counted */
} dril_eval_info;
int32_t dril_eval_options_default(dril_eval_options* o);   /* 10 episodes, deterministic, evaluation.jl:57-58 */
int32_t dril_evaluate_agent_device(dril_handle* h, const dril_eval_options* o, dril_eval_stats* out,
                                   float* episode_rewards, int32_t* episode_lengths, dril_eval_info* info /* may be NULL */);

/* ---- collect_trajectory on the device (src/utils/trajectory_utils.jl:3-49; docs/evaluation.md, "Trajectories") ---- */
/* The reference loop, once per recorded env and independently of the others: envs 0..M-1 of this handle record their FIRST episode after the call's own reset.
 * Row t < L of a trajectory is the ORIGINAL observation before step t + 1 (never normalised; mapped back with unscale_from_unit under ScalingWrapperEnv), action row t
 * what predict_actions returns after to_env (and after unscale! under ScalingWrapperEnv: the value the env's physics receives), reward row t the env's own raw reward.
 * The agent sees the wrapper's observation: scaled, and normalised with the statistics in force, FROZEN for the call (every normaliser of the handle, as in
 * dril_evaluate_agent_device).  Row L is observe(env) of the env that did not auto-reset — the terminal state, in the wrapper's scale unless final_original.
 * The episode ends at its first terminated || truncated, or after max_steps steps; the episode's end takes precedence when both coincide.  With deterministic = 0 the
 * draws are those of dril_evaluate_agent_device on the same seed.  The trajectory of env m does not depend on M, on poll_steps or on the other envs.
 * The call leaves nothing behind: everything dril_evaluate_agent_device sets aside and puts back is set aside and put back here, on error paths too; the monitor's
 * launches are not made and no all-reduce is enqueued (each rank of a data-parallel job records its own envs).
 * Two forms, the same recording bit for bit: step-granular launches with shadow envs (default), and on request (reserved[DRIL_TRAJ_OPT_PERSISTENT] = 1) the
 * recording inside the persistent evaluate kernel, one launch per K env steps, for the built-in kinds on the fused shapes of width 64 / 128 / 256.  A third form
 * (path 2) serves the same request on a plug-in handle whose code object carries a usable evaluation kernel (dril_evaluate_fused_info): the kernel's recording mode —
 * the lane of a recorded env takes each step a second time on a shadow env that never resets — and one launch of the library's per-trajectory rule over the K rows:
 * 2 launches per K env steps, no step past Tcap enqueued.  Against path 0 it agrees as two f32-equivalent arithmetics do (see dril_evaluate_agent_device).
 * DRIL_ERR_NOT_INITIALISED: null handle.  DRIL_ERR_INVALID_ARG: null options or output array, n_trajectories outside 1..n_envs, negative max_steps or poll_steps, a
 * recording whose device arrays exceed 1 GiB.  DRIL_ERR_UNSUPPORTED: DRIL_ENV_EXTERNAL (the envs live with the caller). */
typedef struct dril_traj_options {
    int32_t n_trajectories;              /* M: envs 0..M-1 record; 1 <= M <= n_envs */
    int32_t max_steps;                   /* trajectory_utils.jl:6,38-41; 0 = nothing (the env's time limit ends every episode) */
    int32_t deterministic;               /* :8, default 1 */
    int32_t has_seed; uint64_t seed;     /* as dril_eval_options: 0 = the env seed in force; else env e resets with seed + global env index */
    int32_t poll_steps;                  /* env steps between two looks at the finished-counter; 0 = the library's default */
    int32_t final_original;              /* 0 (reference): the last observation as ScalingWrapperEnv delivers it (:44); 1: unscaled like rows 0..L-1 */
    int32_t reserved[5];                 /* reserved[DRIL_TRAJ_OPT_PERSISTENT]: the opt-in request for the one-launch form.  0 (default): the step-granular launches with
                                          * shadow envs.  1: where the persistent evaluate kernel can run (built-in kinds on the fused shapes of width 64 / 128 / 256, with
                                          * or without cfg.norm_*), envs 0..M-1 are recorded inside it, K env steps per launch, no shadow envs — the same recording, bit
                                          * for bit.  A plug-in handle with a usable evaluation kernel records through it (path 2).  Elsewhere (generic shapes, other
                                          * plug-ins, DRIL_FORCE_STEPWISE) the request falls back silently.  The other words: 0 */
} dril_traj_options;
#define DRIL_TRAJ_OPT_PERSISTENT 0       /* index into dril_traj_options.reserved */
typedef struct dril_traj_info {
    int32_t capacity, steps_enqueued, launches, longest, cut_by_max_steps, reserved[3];   /* Tcap, env steps enqueued, launch calls of the loop, max L, trajectories with bit 2;
                                          * reserved[DRIL_TRAJ_INFO_PATH]: what ran — 0 the step-granular launches, 1 the persistent kernel's recording mode, 2 the
                                          * recording mode of a plug-in's fused evaluation kernel */
} dril_traj_info;
#define DRIL_TRAJ_INFO_PATH 0            /* index into dril_traj_info.reserved */
int32_t dril_traj_options_default(dril_traj_options* o);   /* M = 1, deterministic, the rest 0 */
/* Tcap = max_steps > 0 ? min(max_steps, episode_len) : episode_len: the rows the output arrays are sized with */
int32_t dril_trajectory_capacity(const dril_handle* h, const dril_traj_options* o, int32_t* capacity);
int32_t dril_collect_trajectory_device(dril_handle* h, const dril_traj_options* o,
                                       float* observations,  /* (D, Tcap+1, M) column-major: trajectory m, row t at ((m*(Tcap+1)+t)*D); rows > lengths[m] are 0 */
                                       void* actions,        /* i32 (Tcap, M) | f32 (A, Tcap, M); rows >= lengths[m] are 0 */
                                       float* rewards,       /* (Tcap, M) */
                                       int32_t* lengths,     /* (M): steps taken */
                                       uint8_t* end_flags,   /* (M): bit0 terminated, bit1 truncated, bit2 stopped by max_steps ("Max steps reached") */
                                       dril_traj_info* info  /* may be NULL; the five arrays may not */);

/* ---- train! ------------------------------------------------------------------ */
/* iterations = max_steps / (T*E*world) of {set lr, collect_rollout!, ppo update}: ppo.jl:154-298.
 * stats / fps arrays need `iterations` entries (may be NULL) */
int32_t dril_train(dril_handle* h, int64_t max_steps, dril_ppo_stats* stats, double* fps, int32_t* iterations_done);

/* ---- populations: many small PPO agents per launch (new; the reference has no counterpart: defined as P calls of train!, docs/population.md) ---------------- */
/* A population is a set of ordinary PPO handles joined for batched launches: where P solo iterations launch rollout_duo_kernel and ppo_update_small_kernel P times,
 * a population launches rollout_duo_pop_kernel once and ppo_update_small_pop_kernel once per `cap` members (dril_population_info).  The per-member device code and
 * arguments are those of the solo kernels, so every member is BIT-IDENTICAL to the same handle driven alone with dril_collect_rollout / dril_ppo_update / dril_train.
 * Ownership: the members stay the caller's.  Between population calls every verb works on a member (dril_get_params, dril_policy_from_handle,
 * dril_set_learning_rate, dril_debug_set_noise / _set_permutation, ...; dril_evaluate_agent_device too, though the whole population is evaluated by one call of
 * dril_population_evaluate_device below); the population keeps no copy of member state and reads each handle
 * when it builds the member's argument block.  dril_destroy of a joined member is refused (DRIL_ERR_INVALID_ARG): dril_population_destroy first.  A population and
 * its members are driven from one host thread.
 * Equal across members (they fix the kernel instance and the grid): env_kind (built-in kinds), n_envs, n_steps, batch_size, epochs, hidden dims, activation, device,
 * normalize_advantage.  Free per member: seed, learning rate, gamma, gae_lambda, clip_range, clip_range_vf, ent_coef, vf_coef, max_grad_norm, target_kl (and their
 * has_ flags), Adam betas / eps, monitor_window, parameters, optimiser state.
 * dril_population_join refuses, naming the member index and the reason in dril_population_last_error(NULL), and leaves every handle as it was:
 * Device env plug-in handles (DRIL_ENV_MODULE) join too when their solo iteration is the one-launch form on both sides: dril_rollout_fused_enable and
 * dril_update_fused_enable on and available, and a code object built with DRIL_ENV_PLUGIN_ROLLOUT_POP (include/device/dril_env_rollout_pop.h).  The population then
 * launches the plug-in's dril_env_plugin_rollout_pop once and ppo_update_generic_small_pop_kernel once per chunk of optimiser steps, with no cap on members; equal
 * across such members are also the code object (size and hash of the file), ScalingWrapperEnv on / off and the net's layers; plug-in and built-in members do not mix
 * (DRIL_ERR_INVALID_ARG).  dril_population_evaluate_device evaluates plug-in members one by one (docs/population.md, "Plug-in members").
 *   DRIL_ERR_UNSUPPORTED  an external handle, a world, a device env plug-in handle without both opt-ins or without the population entry; a normalising handle; a generic or wide net; batch_size > 64; world_size > 1;
 *                         a handle whose iteration is not one rollout_duo_kernel launch + one ppo_update_small_kernel launch (DRIL_GRAD_VARIANT, DRIL_FORCE_STEPWISE, ...)
 *   DRIL_ERR_INVALID_ARG  n < 1 or n > DRIL_POPULATION_MAX, a null entry, the same handle twice, a handle already in a population, mixed kinds / shapes / devices
 * A member that cannot take the batched launch in one iteration (a latched or out-of-range exact-f32 forward / update, a redo after a non-finite f16 step, a
 * pair of workgroups that was not co-resident) runs ALONE through the solo code after the batched launches and is counted in dril_population_info.
 * Errors: a member's error (DRIL_ERR_NAN_IN_GRADS, ...) does not stop the other members' iteration; the call returns the first failing member's status,
 * dril_population_last_error names the member, the member's own dril_last_error says what a solo call would have said.  dril_population_train stops after the
 * iteration in which a member failed. */
#define DRIL_POPULATION_MAX 4096   /* members of one population; a verb runs ceil(n / cap) update launches */
typedef struct dril_population dril_population;
struct dril_population_info {     /* (a struct tag: dril_population_info is also the verb that fills it) */
    int32_t members;
    int32_t cap;                       /* members per ppo_update_small_pop_kernel launch: num_cus / 4 (two workgroups per member, one per CU, at most half the chip) */
    int32_t last_rollout_launches, last_update_launches;   /* batched kernel launches of the last population call (an update of S optimiser steps: ceil(S / DRIL_SMALL_CHUNK) x ceil(n / cap)) */
    int32_t last_solo_rollouts, last_solo_updates;         /* members run alone through the solo code in the last call */
    int64_t total_rollout_launches, total_update_launches, total_solo_rollouts, total_solo_updates;   /* the same since join */
    double last_launches_per_iteration;                    /* batched launches of the last call / the iterations it ran (collect_rollout and ppo_update count as one) */
    double last_rollout_ms, last_update_ms;                /* HIP-event time of the batched kernels of the last call (member 0's cfg.profile_events != 0, else 0) */
    int64_t reserved[4];
};
int32_t dril_population_join(dril_handle** members, int32_t n, dril_population** out);
int32_t dril_population_destroy(dril_population* p);            /* members stay alive and usable */
const char* dril_population_last_error(const dril_population* p);   /* NULL: the last refusal of dril_population_join on this thread */
/* dril_collect_rollout / dril_ppo_update of every member; fps / out: n entries, may be NULL */
int32_t dril_population_collect_rollout(dril_population* p, double* fps);
int32_t dril_population_ppo_update(dril_population* p, dril_ppo_stats* out);
/* dril_train of every member: iterations = max_steps / (T*E) of {set lr, collect, update}; stats / fps: [iteration][member], iterations x n entries (may be NULL) */
int32_t dril_population_train(dril_population* p, int64_t max_steps, dril_ppo_stats* stats, double* fps, int32_t* iterations_done);
int32_t dril_population_info(const dril_population* p, struct dril_population_info* out);
/* dril_evaluate_agent_device of every member, in ONE evaluate_pop_kernel launch and ONE look at the members' counters per K env steps (docs/population.md, "Evaluation").
 * Equal to solo: out[m], member m's episode rewards / lengths and member_info[m] (path, launches, steps_enqueued, events) are byte for byte what
 *   dril_evaluate_agent_device(member m, o, ...) returns for that handle alone.  One options struct serves all members: has_seed = 0 uses each member's own env seed
 *   in force, has_seed = 1 gives every member the same seed (common random numbers across members); poll_steps, deterministic and n_eval_episodes are the solo
 *   verb's.  K is the solo verb's, and equal for all members (n_envs and the env kind are).
 * Leaves nothing behind, per member: the solo verb's set-aside and put-back (the same functions), on error paths too.  A population that evaluates between two
 *   iterations continues bit-identically to one that does not.
 * One look per K steps for the whole population: the members' counters are one population-owned device array (EvalAcct.counter of member m points at word m; the
 *   other accounting buffers are the handle's own).  Per round: the argument blocks built in pinned memory (T = 0 for a member that has seen n_eval_episodes events,
 *   else T = K and its own step0), one copy to the device, one launch, one copy of the n counters home, one synchronise.  Then every member's event list is copied
 *   home, its state put back, one more synchronise, and the host's reduction per member.  The bound on an evaluation that never ends is the solo verb's, per member.
 * Who runs solo (dril_evaluate_agent_device alone, after the batched loop; counted in solo_members): a member on the exact-f32 forward (max |W2| >= 350, or the
 *   latch); every member under o->force_step_granular or DRIL_FORCE_STEPWISE.  reserved[DRIL_EVAL_OPT_PERSISTENT] is accepted and changes nothing (members never normalise).
 * Errors: as the other population verbs — a failing member does not stop the others and its state is put back; the call returns the first failing member's status,
 *   dril_population_last_error names the member, its own dril_last_error says what the solo call would have said.  DRIL_ERR_INVALID_ARG, no member touched: null p, o
 *   or out, n_eval_episodes < 1, poll_steps < 0. */
typedef struct dril_population_eval_info {
    int32_t launches;        /* evaluate_pop_kernel launches of the call */
    int32_t looks;           /* counter copies + synchronises (== launches) */
    int32_t batched_members, solo_members;
    double  kernel_ms;       /* HIP-event time of the batched launches; 0 unless member 0 has profile_events */
    int64_t reserved[4];
} dril_population_eval_info;
/* out: n entries; episode_rewards / episode_lengths: [member][n_eval_episodes], may be NULL; member_info: n entries, may be NULL; info may be NULL */
int32_t dril_population_evaluate_device(dril_population* p, const dril_eval_options* o, dril_eval_stats* out,
                                        float* episode_rewards, int32_t* episode_lengths,
                                        dril_eval_info* member_info, dril_population_eval_info* info);

/* ---- multi-GPU (new; the reference is single-process) ------------------------- */
/* 128-byte ncclUniqueId from rank 0, distributed to the other ranks by the host */
int32_t dril_comm_unique_id(uint8_t id[128]);
/* RCCL communicator over cfg.world_size ranks; gradients and loss statistics are summed with one
 * ncclAllReduce per optimiser step on the handle's stream */
int32_t dril_comm_init(dril_handle* h, const uint8_t id[128]);
/* ranks the handle's communicator spans: ncclCommCount of the RCCL communicator (what RCCL itself saw, not cfg.world_size), the group
 * size of a loopback communicator, 1 without a communicator, -1 on error */
int32_t dril_comm_ranks(dril_handle* h);
/* all-reduces this handle has issued since dril_create (every call site counts: advantage moments, [grads || 8 sums], the per-epoch
 * moment table, NormalizeWrapperEnv's batch moments, the explained-variance sums) */
int64_t dril_comm_allreduce_calls(const dril_handle* h);
/* which device the handle lives on, for the banner every rank of a multi-GPU job prints before dril_comm_init and for RCCL failure messages:
 * "device <ordinal> of <visible count> visible: <name> <arch>, <CUs> CUs, PCI <bus id>, HIP_VISIBLE_DEVICES=... ROCR_VISIBLE_DEVICES=..." (new; no reference counterpart).
 * A failing ncclCommInitRank / ncclAllReduce puts ncclGetErrorString, ncclGetLastError and this line into dril_last_error. */
const char* dril_device_info(const dril_handle* h);
/* DEBUG / TEST: join n handles of THIS process, all on ONE device, with cfg.world_size == n and ranks 0..n-1, into a loopback
 * communicator (RCCL refuses two ranks per device).  Every all-reduce call site, count and dtype of the data-parallel path is unchanged;
 * the transport is an in-process rendezvous plus one kernel that sums the ranks' device buffers in rank order and writes the sum back to
 * all of them.  Each handle must then be driven from its own host thread, all making the same sequence of calls; a rank that waits
 * 120 s for the others fails with DRIL_ERR_RCCL.  (new: the reference has no distributed code) */
int32_t dril_debug_comm_loopback(dril_handle** handles, int32_t n);
/* DEBUG / TEST: bytes of device and pinned host memory that the handles, populations and running calls of this process hold through the library's owning buffers
 * (csrc/dril_devmem.h), process-wide.  Back at its earlier value once whatever was created since is destroyed; unlike hipMemGetInfo it does not see other tenants
 * of the card.  (The envs' own arrays and a deployment policy are not counted.) */
int64_t dril_debug_device_bytes_live(void);

/* ---- measurement ---------------------------------------------------------------- */
/* accumulated HIP-event time and count of the BRACKETED launches of one kernel class since the last reset (total_ms / launches = average launch);
 * dril_profile_launches: all launches of the class in the same window (= launches unless cfg.profile_events > 1 thinned the per-step classes) */
int32_t dril_profile_get(dril_handle* h, int32_t kernel_id, double* total_ms, int64_t* launches);
int32_t dril_profile_launches(dril_handle* h, int32_t kernel_id, int64_t* all_launches);
int32_t dril_profile_reset(dril_handle* h);
const char* dril_kernel_name(int32_t kernel_id);
int32_t dril_kernel_count(void);   /* DRIL_K_COUNT of the loaded library */
/* which gradient kernel the handle's LAST optimiser step ran and the arithmetic it computes in ("<kernel>: <arithmetic>"; "none yet" before the
 * first step): hidden [64,64] runs ppo_grad_pair_kernel (f16 matrix cores, fp32-equivalent two-piece operand split) on large minibatches and the f32-MFMA
 * ppo_grad_kernel on small ones, [128,128] and [256,256] ppo_grad_wide_split_kernel, everything else the generic path (docs/kernels/ppo_kernels.md;
 * DRIL_GRAD_VARIANT overrides the choice).  After a per-step kernel the text ends in "; grid G=<g> Gc=<gc>": the slabs (ppo_grad_pair_kernel: pairs) that step
 * gave the actor and the critic.  The pointer is the handle's: valid until the next call on it */
const char* dril_grad_kernel_info(const dril_handle* h);
const char* dril_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DRIL_HIP_H */
