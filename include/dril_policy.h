/*
 * dril_policy.h — C ABI of the deployment policies of libdril_hip.so: what a user runs AFTER training.
 *
 * Stands in for, in the reference checkout (KristianHolme/DRiL.jl):
 *   src/deployment/deployment_policy.jl         extract_policy, NeuralPolicy, NormWrapperPolicy
 *   src/environment_wrappers/normalizeWrapperEnv.jl:174-179   normalize_obs!
 *   src/spaces/default_adapters.jl              ClampAdapter, TanhScaleAdapter, DiscreteAdapter
 *
 * A policy object is light and immutable: the actor's parameters (and log_std), the action adapter's bounds and,
 * optionally, frozen observation statistics.  No critic, no optimiser state, no buffers, no envs.  It is a COPY:
 * training, or destroying, the handle it was taken from does not touch it, and taking or using it leaves that
 * handle exactly as it was.
 *
 * One call turns a batch of RAW observations into actions the env takes (what act! receives):
 *   normalise (when the policy carries statistics) -> every Dense layer -> distribution head -> adapter.
 * Up to a batch threshold this is ONE kernel launch (policy_act_kernel: plain f32 FMA, fixed summation order, the
 * result for one observation does not depend on what else is in the batch); above it the layer contractions of
 * the training paths run, followed by one head launch (docs/deployment.md has the measurement).
 *
 * Conventions are those of dril_hip.h: int32 status (enum dril_status), the library owns device memory and the
 * object, the caller owns host pointers for the duration of the call, calls are synchronous at return, weights are
 * (out x in) column-major as Lux.Dense stores them, observations are (obs_dim x batch) column-major.
 *
 * Thread safety: calls on DIFFERENT policy objects may run concurrently; calls on ONE policy object must be
 * serialised by the caller (it owns one stream and one set of staging buffers).
 */
#ifndef DRIL_POLICY_H
#define DRIL_POLICY_H

#include "dril_hip.h"
#include "dril_sac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DRIL_POLICY_ABI_VERSION 1u
#define DRIL_POLICY_MAX_ACTION_DIM 64
#define DRIL_POLICY_MAX_WIDTH 1024

typedef struct dril_policy dril_policy;

enum dril_policy_kind {
    DRIL_POLICY_CATEGORICAL = 0,            /* Discrete space, DiscreteAdapter: actions are int32, index + action_start        */
    DRIL_POLICY_DIAG_GAUSSIAN = 1,          /* Box space, ClampAdapter: clamp(raw, low, high) per dimension                    */
    DRIL_POLICY_SQUASHED_DIAG_GAUSSIAN = 2  /* Box space, TanhScaleAdapter: raw = tanh(..), env = scale(tanh(raw)) (SAC)       */
};

typedef struct dril_policy_desc {
    uint32_t abi_version;                   /* DRIL_POLICY_ABI_VERSION                                                        */
    int32_t kind;                           /* enum dril_policy_kind                                                          */
    int32_t obs_dim;                        /* 1 .. 1024                                                                      */
    int32_t action_dim;                     /* Categorical: number of actions; Box: dimensions.  1 .. 64                      */
    int32_t action_start;                   /* Categorical only: the Discrete space's first action                            */
    int32_t n_hidden;                       /* 1 .. 4                                                                         */
    int32_t hidden[4];                      /* widths 1 .. 1024                                                               */
    int32_t activation;                     /* as dril_config.activation: 0 tanh 1 relu 2 sigmoid 3 elu 4 leakyrelu 5 softplus 6 gelu 7 swish */
    int32_t has_norm;                       /* 1: NormWrapperPolicy — observations are normalised with the frozen statistics   */
    float clip_obs;                         /* has_norm: clamp((x - mean) / sqrt(var + epsilon), -clip_obs, clip_obs)          */
    float epsilon;
    int32_t device;
    int32_t reserved;
    float action_low[DRIL_POLICY_MAX_ACTION_DIM];   /* Box: per-dimension bounds; DiagGaussian with low >= high: no clamp in that dimension */
    float action_high[DRIL_POLICY_MAX_ACTION_DIM];
} dril_policy_desc;

/* ---- construction ------------------------------------------------------------------------------------------------
 * From host arrays.  actor_params: the actor net {W_1 b_1 ... W_{n_hidden+1} b_{n_hidden+1}} in the layout of the
 * actor's slice of dril_get_params / dril_sac_get_params, n floats (must equal the count the descriptor implies).
 * log_std: action_dim floats for the two Gaussian kinds, ignored (may be NULL) for Categorical.  obs_mean / obs_var:
 * obs_dim floats each when desc->has_norm, else ignored. */
int32_t dril_policy_create(const dril_policy_desc* desc, const float* actor_params, size_t n, const float* log_std,
                                    const float* obs_mean, const float* obs_var, dril_policy** out);
/* extract_policy(agent) (with_norm = 0) and extract_policy(agent, norm_env) (with_norm = 1) of a training handle: a
 * device-to-device snapshot of the actor (+ log_std), the adapter bounds (built-in env kind, plug-in descriptor or the
 * ext_ fields) and action_start; with_norm = 1 also takes the observation statistics, epsilon and clip_obs in force
 * (cfg.norm_obs handles and handles wrapped by the normalize_enable verbs) and is DRIL_ERR_NOT_INITIALISED when the
 * handle has no NormalizeWrapperEnv.  The handle is only read. */
int32_t dril_policy_from_handle(dril_handle* h, int32_t with_norm, dril_policy** out);
int32_t dril_policy_from_sac_handle(dril_sac_handle* h, int32_t with_norm, dril_policy** out);
int32_t dril_policy_destroy(dril_policy* p);
/* message of the last failed call on p; p == NULL: of the last failed construction on this thread */
const char* dril_policy_last_error(const dril_policy* p);

/* ---- acting ------------------------------------------------------------------------------------------------------
 * obs: batch raw observations, obs_dim floats each.  deterministic != 0: mode of the distribution (argmax / mean /
 * tanh(mean)); else a sample.  noise (sampling only): NULL = the policy's own Philox stream (seed, call counter); or
 * injected draws in the layout of the predict_actions verbs: Categorical one f64 uniform per observation, Gaussian
 * kinds action_dim f32 standard normals per observation.  raw_actions: the policy's action before the adapter;
 * env_actions: after it, what act! takes.  Categorical: int32 per observation (both arrays hold index +
 * action_start); Box kinds: action_dim f32 per observation.  Either output may be NULL, not both.
 * One host-to-device copy, one launch (batch <= threshold), one device-to-host copy and one stream wait, through
 * pinned staging buffers the policy owns and grows on demand. */
int32_t dril_policy_act(dril_policy* p, const float* obs, int64_t batch, int32_t deterministic, const void* noise,
                                 void* raw_actions, void* env_actions);
/* restarts the policy's own noise stream: same seed, same sequence of calls -> same draws */
int32_t dril_policy_set_seed(dril_policy* p, uint64_t seed);
/* batches up to `threshold` run policy_act_kernel; larger ones the layer contractions.  threshold <= 0 restores the
 * default (docs/deployment.md); the kernel itself takes any batch */
int32_t dril_policy_set_threshold(dril_policy* p, int64_t threshold);
/* enable != 0: the device work of every following act call is bracketed by HIP events (costs the call a few
 * microseconds); *last_ms, when not NULL, receives the device time of the last bracketed call (-1: none yet) */
int32_t dril_policy_kernel_time(dril_policy* p, int32_t enable, double* last_ms);

/* ---- inspection (everything needed to rebuild the policy elsewhere with the create verb) ------------------------- */
int32_t dril_policy_describe(const dril_policy* p, dril_policy_desc* out);
int64_t dril_policy_param_count(const dril_policy* p);   /* floats of the actor net; -1 on a NULL policy */
/* actor_params: n = param count floats; log_std: action_dim floats (Gaussian kinds; may be NULL) */
int32_t dril_policy_get_params(dril_policy* p, float* actor_params, size_t n, float* log_std);
/* obs_mean / obs_var: obs_dim floats each; DRIL_ERR_NOT_INITIALISED when the policy carries no statistics */
int32_t dril_policy_get_norm(dril_policy* p, float* obs_mean, float* obs_var);

#ifdef __cplusplus
}
#endif
#endif /* DRIL_POLICY_H */
