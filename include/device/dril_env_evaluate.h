// dril_env_evaluate.h — the FUSED EVALUATION of a device env plug-in: K env steps of evaluate_agent / collect_trajectory per launch.
//
// A plug-in author adds two lines to a source that ends in DRIL_ENV_PLUGIN(MyEnv):
//
//     #include "device/dril_env_evaluate.h"
//     DRIL_ENV_PLUGIN_EVALUATE(MyEnv)
//
// and the code object gains dril_env_plugin_evaluate, dril_env_plugin_evaluate_scaled (exactly when dril_env_plugin_scalable<MyEnv>(), the rule of the other _scaled
// kernels) and the descriptor dril_env_plugin_evaluate_desc.  dril_evaluate_agent_device and dril_collect_trajectory_device (include/dril_hip.h) launch it where the
// caller asks for the persistent form (path 2); the step-granular launches stay the default.  DrilEnvPluginDesc / Args, DrilEnvRolloutDesc / Args and their ABI numbers
// do not change, a source without this macro compiles to exactly the symbols it had, and the macro works with or without DRIL_ENV_PLUGIN_ROLLOUT in the same source.
//
// One launch does, for the envs of its workgroup, K steps of the loop of evaluation.jl:90-124 / trajectory_utils.jl:16-45: observe; per step the observation as the
// agent sees it (scaled in the _scaled kernel; normalised with FROZEN statistics when the argument block carries them — dril::normalize_obs, the wrapper's own line, mean
// and var read only), the actor forward, the action (mode or draw), the transition (dril_env_plugin_step_one: the ONE definition, monitor pointers null), and the step's
// raw reward and flag byte into row k of two (K x E) arrays.  The episode accounting (dril_eval_account.h) and the per-trajectory rule (dril_traj_record.h) stay in the
// library: one launch of its own over the K rows, so neither structure enters this ABI.
//
// The kernel is the fused rollout's (dril_env_rollout.h) with the critic taken out: a workgroup owns a tile of DRIL_ENV_ROLLOUT_TILE envs for the K steps, two LDS panels,
// the parameters staged into LDS when they fit, the actor through dril_rollout_net — the same k-ascending fmaf chain per (row, column), so an env's results do not depend
// on E, on its tile or on K.  The only synchronisation is the workgroup barrier: no grid barrier, no cooperative launch, no spin-wait, no atomics.
//
// Recording (n_record = M > 0), envs e < M: the launch's opening observation (before normalisation) into rec_obs0, per step the raw action into row k of rec_act and
// the observation after the step and BEFORE the auto-reset into row k of rec_obs.  The latter needs a step that does not reset, so the lane takes the step a second
// time first — dril_env_plugin_step_one again, on the block `shadow` (M-sized state and counters, fixed_len = 1, episode_len = INT32_MAX, filled by the library) given
// the pre-step state: what the step-granular verb does with separate launches.  The transition is not restated.
//
// With DRIL_ENV_PLUGIN_HOST the macro emits dril_env_plugin_host_evaluate (and _scaled): the same per-env functions in a serial loop.
#pragma once
#include "dril_env_rollout.h"
#include "dril_normalize.h"

#ifndef DRIL_ENV_EVALUATE_ABI
#define DRIL_ENV_EVALUATE_ABI 1u         // bumps whenever DrilEnvEvaluateDesc / DrilEnvEvaluateArgs or the meaning of a field changes
#endif

struct DrilEnvEvaluateDesc {
    uint32_t abi_version;                // DRIL_ENV_EVALUATE_ABI the plug-in was compiled against
    uint32_t args_size;                  // sizeof(DrilEnvEvaluateArgs) the plug-in was compiled against
    int32_t tile, threads, max_width, has_scaled, reserved[2];
};

// The argument block of the evaluation kernels (passed by value).  Pointers are device pointers.
struct DrilEnvEvaluateArgs {
    // the rollout's block, of which the evaluation reads: env (E, time limit, seed0, state and counters; obs: (E x D) scratch, the observation the env side hands
    // out; everything else null), T = K (the env steps of this launch), the net's shape, actor_off, log_std_off, params, act ((E): the step's raw action, i32 | f32 x A
    // — scratch), rew and flags ((K x E): row k = the raw reward and the flag byte — bit0 terminated, bit1 truncated — of the launch's step k).  The other words: 0
    DrilEnvRolloutArgs r;
    DrilEnvPluginArgs shadow;            // recording: the M shadow envs (E = M, fixed_len = 1, episode_len = INT32_MAX, own state and counters); unused when n_record == 0
    int32_t deterministic, n_record;     // deterministic: mode(d) instead of rand(d); n_record: M
    float norm_eps, norm_clip;
    const float* norm_mean; const float* norm_var;   // (D) each: the frozen RunningMeanStd of the observations, read only; null = no normaliser
    float* rec_obs0;                     // (M x D): the observation before the launch's first step, as the env side hands it out
    void* rec_act;                       // (K x M): raw actions
    float* rec_obs;                      // (K x M x D): the observation after step k, before the auto-reset
};

template <class Env> constexpr DrilEnvEvaluateDesc dril_env_evaluate_make_desc() {
    DrilEnvEvaluateDesc d{};
    d.abi_version = DRIL_ENV_EVALUATE_ABI; d.args_size = (uint32_t)sizeof(DrilEnvEvaluateArgs);
    d.tile = DRIL_ENV_ROLLOUT_TILE; d.threads = DRIL_ENV_ROLLOUT_THREADS; d.max_width = DRIL_ENV_ROLLOUT_MAX_WIDTH; d.has_scaled = dril_env_plugin_scalable<Env>() ? 1 : 0;
    return d;
}

// ---- per env: shared by the kernel and the host build ---------------------------------------------------------------------------------------------------------
// element d of the observation as the actor sees it
DRIL_ENV_FN inline float dril_evaluate_agent_obs(const DrilEnvEvaluateArgs& g, int d, float v) {
    return g.norm_mean ? dril::normalize_obs(v, g.norm_mean[d], g.norm_var[d], g.norm_eps, g.norm_clip) : v;
}
// the action of env e: z = the actor's output row (stride zs).  Deterministic: generic_policy_head_kernel's mode — the first maximum of expf(z - m) / s | the mean;
// else dril_rollout_head_one's draw (stream 1 at the env's gstep), without log-probability or value
template <class Env> DRIL_ENV_FN inline void dril_evaluate_head_one(const DrilEnvEvaluateArgs& g, int e, const float* z, int zs) {
    constexpr int A = Env::A;
    const uint64_t seed = g.r.env.seed0 + (uint64_t)e; const uint32_t gs = g.r.env.gstep[e];
    if constexpr (Env::discrete) {
        float m, s; dril::softmax_stats(z, A, m, s, zs);
        int act;
        if (g.deterministic) {
            act = 0; float best = expf(z[0] - m) / s;
            for (int k = 1; k < A; ++k) { const float p = expf(z[k * zs] - m) / s; if (p > best) { best = p; act = k; } }
        } else act = dril::categorical_draw(z, A, m, s, dril::env_noise_u01(seed, gs), zs);
        ((int32_t*)g.r.act)[e] = act + g.r.env.action_start;
    } else {
        const float* ls = g.r.params + g.r.log_std_off;
        float* x = (float*)g.r.act + (size_t)e * A;
        for (int k = 0; k < A; ++k) x[k] = g.deterministic ? z[k * zs] : dril::gauss_draw(z[k * zs], ls[k], dril::env_noise_randn(seed, gs, k));
    }
}
// the transition of env e at the launch's step k.  A recorded env (e < n_record) first takes the step on its shadow, which never resets: the raw action into row k of
// rec_act, the shadow's observation — after the step, before any reset — into row k of rec_obs
template <class Env, bool scaled> DRIL_ENV_FN inline void dril_evaluate_transition_one(const DrilEnvEvaluateArgs& g, int k, int e) {
    constexpr int S = Env::S, W = Env::discrete ? 1 : Env::A;
    const bool recorded = e < g.n_record;
    const size_t row = (size_t)k * g.n_record, live = (size_t)k * g.r.env.E;
    if (recorded) {
        for (int i = 0; i < W; ++i) ((uint32_t*)g.rec_act)[(row + e) * W + i] = ((const uint32_t*)g.r.act)[(size_t)e * W + i];
        for (int i = 0; i < S; ++i) g.shadow.state[(size_t)e * S + i] = g.r.env.state[(size_t)e * S + i];
    }
    // pass 0: the shadow (recorded envs only); pass 1: the env itself.  One call site, so that the env's step is expanded once
#if !defined(DRIL_ENV_PLUGIN_HOST)
#pragma unroll 1
#endif
    for (int pass = recorded ? 0 : 1; pass < 2; ++pass) {
        DrilEnvPluginArgs s = pass ? g.r.env : g.shadow;
        s.actions = g.r.act;
        s.rewards = pass ? g.r.rew + live : nullptr; s.flags = pass ? g.r.flags + live : nullptr;
        s.obs = pass ? g.r.env.obs : g.rec_obs + row * Env::D;
        dril_env_plugin_step_one<Env, scaled>(s, e);
    }
}

#if defined(DRIL_ENV_PLUGIN_HOST)
// ---- the host build: the same per-env functions in a serial loop --------------------------------------------------------------------------------------------
template <class Env, bool scaled> inline void dril_env_evaluate_host(const DrilEnvEvaluateArgs& g) {
    constexpr int D = Env::D;
    float x[DRIL_ENV_ROLLOUT_MAX_WIDTH], y[DRIL_ENV_ROLLOUT_MAX_WIDTH], seen[DRIL_ENV_ROLLOUT_MAX_WIDTH];
    for (int e = 0; e < g.r.env.E; ++e) {
        float* cur = g.r.env.obs + (size_t)e * D;
        dril_env_plugin_observe_one<Env, scaled>(g.r.env, e);
        if (e < g.n_record) for (int d = 0; d < D; ++d) g.rec_obs0[(size_t)e * D + d] = cur[d];
        for (int k = 0; k < g.r.T; ++k) {
            for (int d = 0; d < D; ++d) seen[d] = dril_evaluate_agent_obs(g, d, cur[d]);
            const float* z = dril_rollout_host_net(g.r, D, Env::A, g.r.actor_off, seen, x, y);
            dril_evaluate_head_one<Env>(g, e, z, 1);
            dril_evaluate_transition_one<Env, scaled>(g, k, e);
        }
    }
}
#define DRIL_ENV_EVALUATE_ENTRY(name) __attribute__((visibility("default"))) void dril_env_plugin_host_##name(const DrilEnvEvaluateArgs* g)
#define DRIL_ENV_EVALUATE_IMPL dril_env_evaluate_host
#define DRIL_ENV_EVALUATE_RUN(Env, scaled) DrilEnvEvaluateBody<Env, scaled>::run(*g)
#else
// ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------------
// the K steps of the workgroup's tile; P: the parameter vector the forward reads — global memory, or its copy in LDS
template <class Env, bool scaled> __device__ inline void dril_env_evaluate_steps(const DrilEnvEvaluateArgs& g, const float* P, float* p0, float* p1) {
    constexpr int TC = DRIL_ENV_ROLLOUT_TILE, D = Env::D;
    const int tid = threadIdx.x, E = g.r.env.E, e0 = blockIdx.x * TC;
    const int ncol = E - e0 < TC ? E - e0 : TC, e = e0 + tid;
    const bool mine = tid < ncol;                                                     // thread c steps env e0 + c
    if (mine) {
        dril_env_plugin_observe_one<Env, scaled>(g.r.env, e);                           // observations = observe(env), evaluation.jl:88
        if (e < g.n_record) for (int d = 0; d < D; ++d) g.rec_obs0[(size_t)e * D + d] = g.r.env.obs[(size_t)e * D + d];
    }
    __syncthreads();
    for (int k = 0; k < g.r.T; ++k) {
        // the tile's observations as the actor sees them, panel [d][c]: column c = env e0 + c; columns past the batch are zero
        for (int i = tid; i < D * TC; i += DRIL_ENV_ROLLOUT_THREADS) {
            const int c = i / D, d = i - c * D;
            p0[d * TC + c] = c < ncol ? dril_evaluate_agent_obs(g, d, g.r.env.obs[(size_t)(e0 + c) * D + d]) : 0.f;
        }
        __syncthreads();
        const float* out = dril_rollout_net<TC>(g.r, P, D, Env::A, g.r.actor_off, p0, p1);   // predict_actions, :92 (ends behind a barrier)
        if (mine) {
            dril_evaluate_head_one<Env>(g, e, out + tid, TC);
            dril_evaluate_transition_one<Env, scaled>(g, k, e);                       // act! + observe, :94-97
        }
        __syncthreads();
    }
}
template <class Env, bool scaled> __device__ inline void dril_env_evaluate_run(const DrilEnvEvaluateArgs& g) {
    constexpr int TC = DRIL_ENV_ROLLOUT_TILE;
    __shared__ float4 panels[2 * DRIL_ENV_ROLLOUT_MAX_WIDTH * TC / 4];
    __shared__ float4 staged[DRIL_ENV_ROLLOUT_STAGE_FLOATS / 4 + 1];
    float* p0 = (float*)panels; float* p1 = p0 + DRIL_ENV_ROLLOUT_MAX_WIDTH * TC;
    if (g.r.n_params <= DRIL_ENV_ROLLOUT_STAGE_FLOATS) {                                // small nets: the parameters are read K times, so they are staged into LDS once
        float* w = (float*)staged;
        for (int i = threadIdx.x; i < g.r.n_params; i += DRIL_ENV_ROLLOUT_THREADS) w[i] = g.r.params[i];
        dril_env_evaluate_steps<Env, scaled>(g, w, p0, p1);                        // (the first barrier inside comes before the first read)
    } else dril_env_evaluate_steps<Env, scaled>(g, g.r.params, p0, p1);
}
#define DRIL_ENV_EVALUATE_ENTRY(name) __global__ void __launch_bounds__(DRIL_ENV_ROLLOUT_THREADS) dril_env_plugin_##name(DrilEnvEvaluateArgs g)
#define DRIL_ENV_EVALUATE_IMPL dril_env_evaluate_run
#define DRIL_ENV_EVALUATE_RUN(Env, scaled) DrilEnvEvaluateBody<Env, scaled>::run(g)
#endif

// the body of an entry point; empty for a world (DrilEnvRolloutBody)
template <class Env, bool scaled, bool world = DrilEnvIsWorld<Env>::value> struct DrilEnvEvaluateBody { DRIL_ENV_FN static void run(const DrilEnvEvaluateArgs& g) { DRIL_ENV_EVALUATE_IMPL<Env, scaled>(g); } };
template <class Env, bool scaled> struct DrilEnvEvaluateBody<Env, scaled, true> { DRIL_ENV_FN static void run(const DrilEnvEvaluateArgs&) {} };

// the optional _scaled entry point: declared here, DEFINED as a friend of the specialisation that fits the env (the mechanism of DrilEnvRolloutScaledEntry)
#if defined(DRIL_ENV_PLUGIN_HOST)
typedef void (*DrilEnvEvaluateEntry)(const DrilEnvEvaluateArgs*);
#else
typedef void (*DrilEnvEvaluateEntry)(DrilEnvEvaluateArgs);
#endif
extern "C" { DRIL_ENV_EVALUATE_ENTRY(evaluate_scaled); }
template <class Env, bool scalable> struct DrilEnvEvaluateScaledEntry {};
template <class Env> struct DrilEnvEvaluateScaledEntry<Env, true> {
    friend DRIL_ENV_EVALUATE_ENTRY(evaluate_scaled) { DRIL_ENV_EVALUATE_RUN(Env, true); }
#if defined(DRIL_ENV_PLUGIN_HOST)
    static constexpr DrilEnvEvaluateEntry evaluate_scaled = &dril_env_plugin_host_evaluate_scaled;
#else
    static constexpr DrilEnvEvaluateEntry evaluate_scaled = &dril_env_plugin_evaluate_scaled;
#endif
};

#define DRIL_ENV_PLUGIN_EVALUATE(Env)                                                                                    \
    static_assert(DrilEnvRolloutCheck<Env>::ok, "");                                                                     \
    extern "C" {                                                                                                         \
    DRIL_ENV_ROLLOUT_DESC_QUAL extern const DrilEnvEvaluateDesc dril_env_plugin_evaluate_desc = dril_env_evaluate_make_desc<Env>(); \
    DRIL_ENV_EVALUATE_ENTRY(evaluate) { DRIL_ENV_EVALUATE_RUN(Env, false); }                                             \
    }                                                                                                                    \
    template struct DrilEnvEvaluateScaledEntry<Env, dril_env_plugin_scalable<Env>()>;
