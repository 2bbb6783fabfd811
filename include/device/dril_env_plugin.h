// dril_env_plugin.h — the device-side contract of a DEVICE ENV PLUG-IN: a user's own environment, compiled on its own into a gfx950 code object
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include my_env.hip -o my_env.hsaco
// and stepped on the device by libdril_hip.so (DRIL_ENV_MODULE, include/dril_hip.h) with no rebuild of the library and no host round trip per env step.
// The reference's whole env surface is "bring your own AbstractEnv" (interfaces/environments.jl); this is that seam for an env that lives next to the policy.
//
// An env author supplies the physics only:
//
//     #include "device/dril_env_plugin.h"
//     struct MyEnv {
//         static constexpr int  S = 9, D = 12, A = 3;      // state floats, observation dims, action dims (Discrete: number of actions)
//         static constexpr bool discrete = false;
//         static constexpr int  episode_len = 100;         // default max_steps; cfg.episode_len > 0 overrides
//         static constexpr float action_low[A] = {-1, -1, -1}, action_high[A] = {1, 1, 1};     // Box bounds per dimension (continuous envs only)
//         static constexpr const char* name = "MyEnv";
//         DRIL_ENV_FN static void  reset(const DrilEnvRng& rng, float* st);                      // initial state of an episode
//         DRIL_ENV_FN static void  observe(const float* st, float* obs);
//         DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated);   // returns the reward
//     };
//     DRIL_ENV_PLUGIN(MyEnv)
//
// Optionally the env declares its OBSERVATION SPACE, the Box of observation_space(env) (interfaces/environments.jl):
//         static constexpr float obs_low[D] = {...}, obs_high[D] = {...};                      // -INFINITY / INFINITY allowed per dimension
// DRIL_ENV_PLUGIN then emits one more kernel, dril_env_plugin_obs_space (one thread writes low[D] | high[D]; the library runs it once at load time), and — when
// in addition the env is continuous and every observation bound and every action bound is finite with low < high (dril_env_plugin_scalable) — the two kernels of
// ScalingWrapperEnv (scalingWrapperEnv.jl), dril_env_plugin_observe_scaled and dril_env_plugin_step_scaled: the same transition with the agent-facing spaces
// Box(-1, 1), the affine maps of device/dril_scaling.h applied inside the one launch.  An env without obs_low / obs_high emits exactly the descriptor and the three
// kernels it always did; the descriptor, the argument block and DRIL_ENV_PLUGIN_ABI are unchanged by any of this.
//
// Agents that share ONE state (they collide, cooperate or compete) do not fit "one env, one thread": device/dril_env_world.h is the second, optional form for them —
// a WORLD of N agents with one joint step, compiled into the same symbols and seen by the library as N rows per world (DRIL_ENV_PLUGIN_WORLD).
//
// Everything else — action adapters, step counters, truncation at the time limit, the BUF_FLAGS byte, terminal observation, MonitorWrapperEnv's sums, auto-reset —
// is the LIBRARY's transition (EnvCursor / env_advance / env_end_episode of dril_device.h) and is written once, here, in dril_env_plugin_step_one.
//
// With DRIL_ENV_PLUGIN_HOST defined the same file compiles with a plain C++17 compiler (no HIP headers): the qualifiers vanish, no kernels are emitted, and
// dril_env_plugin_host_reset / _observe / _step (and _obs_space / _observe_scaled / _step_scaled under the same conditions as the kernels) run the same wrapper
// over the E envs in a serial loop — for gdb, host sanitizers and CPU tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(DRIL_ENV_PLUGIN_HOST)
#define DRIL_ENV_FN
#else
#include <hip/hip_runtime.h>
#define DRIL_ENV_FN __device__
#endif
#include "dril_philox.h"
#include "dril_scaling.h"

#ifndef DRIL_ENV_PLUGIN_ABI
#define DRIL_ENV_PLUGIN_ABI 1u       // bumps whenever DrilEnvPluginDesc / DrilEnvPluginArgs or the meaning of a field changes
#endif
#define DRIL_ENV_PLUGIN_MAX_S 64     // state floats per env
#define DRIL_ENV_PLUGIN_MAX_D 1024   // observation dims (the generic kernels' limit)
#define DRIL_ENV_PLUGIN_MAX_A 64     // action dims / number of discrete actions

// What a code object says about itself; the library copies it out of the loaded module and checks it BEFORE it launches anything of the module.
struct DrilEnvPluginDesc {
    uint32_t abi_version;            // DRIL_ENV_PLUGIN_ABI the plug-in was compiled against
    uint32_t args_size;              // sizeof(DrilEnvPluginArgs) the plug-in was compiled against
    int32_t S, D, A, discrete, episode_len;
    int32_t agents;                  // 0: one env per row (DRIL_ENV_PLUGIN); N in 2..16: a WORLD of N agents per state (DRIL_ENV_PLUGIN_WORLD, dril_env_world.h).  The word was
                                     // `reserved` and is 0 in every code object built before worlds existed, which keeps its meaning: DRIL_ENV_PLUGIN_ABI stays 1
    float action_low[DRIL_ENV_PLUGIN_MAX_A], action_high[DRIL_ENV_PLUGIN_MAX_A];   // entries 0..A-1 (continuous); low >= high in a dimension = no clamp there
    char name[64];
};

// The ONE argument block of the three kernels (passed by value).  Pointers are device pointers; any destination of the step kernel may be null.
struct DrilEnvPluginArgs {
    int32_t E, episode_len, fixed_len, action_start;
    uint64_t seed0;                  // env e is seeded seed0 + e (seed0 = seed + rank * n_envs: the global env index)
    const void* actions;             // RAW policy actions, i32 (E) | f32 (A x E); the adapters are applied in the wrapper, the buffer keeps the raw action
    float* state;                    // (S x E), env-major
    int32_t* step_count; uint32_t* episode; uint32_t* gstep;
    float* rewards; uint8_t* terminated; uint8_t* truncated;   // (E)
    uint8_t* flags;                  // (E): bit0 terminated, bit1 truncated — row t of BUF_FLAGS during a collection
    float* terminal_obs;             // (D x E): written for truncated envs only
    float* obs;                      // (D x E): observe kernel: the observation; step kernel: the observation AFTER the step (of the fresh episode where one ended)
    float* mon_cur_ret; int32_t* mon_cur_len;   // MonitorWrapperEnv's running sums (null = no monitor)
    float* ep_ret; int32_t* ep_len;  // (E): return / length of the episode that finished in this step
};

struct DrilEnvWords { uint32_t w[4]; };
// Philox stream 0 of the library (the table in dril_device.h) and nothing else: key = the env's seed, counter (episode, 0, 0, block).
// block 0 holds the words the built-in envs reset from.
struct DrilEnvRng {
    uint64_t env_seed; uint32_t episode;
    DRIL_ENV_FN DrilEnvWords words(uint32_t block) const {
        DrilEnvWords r; dril::philox4x32_10((uint32_t)env_seed, (uint32_t)(env_seed >> 32), episode, 0u, 0u, block, r.w); return r;
    }
    DRIL_ENV_FN static float u01(uint32_t word) { return dril::u01_f32(word); }                      // [0, 1) from the top 24 bits
    DRIL_ENV_FN static float randn(uint32_t a, uint32_t b) { return dril::randn_f32(a, b); }         // Box-Muller on two words
};

template <class Env, class = void> struct DrilEnvHasBounds { static constexpr bool value = false; };
template <class Env> struct DrilEnvHasBounds<Env, decltype((void)Env::action_low[0], (void)Env::action_high[0], void())> { static constexpr bool value = true; };

// the optional observation space: static constexpr float obs_low[D], obs_high[D]
template <class Env, class = void> struct DrilEnvHasObsSpace { static constexpr bool value = false; };
template <class Env> struct DrilEnvHasObsSpace<Env, decltype((void)Env::obs_low[0], (void)Env::obs_high[0], void())> { static constexpr bool value = true; };
constexpr bool dril_env_plugin_finite_interval(float low, float high) { return low >= -3.402823466e38f && high <= 3.402823466e38f && low < high; }   // (a NaN fails every comparison)
// ScalingWrapperEnv needs Box / Box with finite, non-empty bounds in every dimension (scalingWrapperEnv.jl:22): a declared observation space and a continuous env
template <class Env> constexpr bool dril_env_plugin_scalable() {
    if constexpr (Env::discrete || !DrilEnvHasObsSpace<Env>::value || !DrilEnvHasBounds<Env>::value) return false;
    else {
        for (int i = 0; i < Env::D; ++i) if (!dril_env_plugin_finite_interval(Env::obs_low[i], Env::obs_high[i])) return false;
        for (int i = 0; i < Env::A; ++i) if (!dril_env_plugin_finite_interval(Env::action_low[i], Env::action_high[i])) return false;
        return true;
    }
}

template <class Env> struct DrilEnvPluginCheck {
    static_assert(Env::S >= 1 && Env::S <= DRIL_ENV_PLUGIN_MAX_S, "DRIL_ENV_PLUGIN: S (state floats per env) must be 1..64");
    static_assert(Env::D >= 1 && Env::D <= DRIL_ENV_PLUGIN_MAX_D, "DRIL_ENV_PLUGIN: D (observation dims) must be 1..1024");
    static_assert(Env::A >= 1 && Env::A <= DRIL_ENV_PLUGIN_MAX_A, "DRIL_ENV_PLUGIN: A (action dims, or number of discrete actions) must be 1..64");
    static_assert(Env::episode_len >= 1, "DRIL_ENV_PLUGIN: episode_len (the default time limit) must be >= 1");
    static_assert(Env::discrete || DrilEnvHasBounds<Env>::value, "DRIL_ENV_PLUGIN: a continuous env (discrete = false) must define static constexpr float action_low[A] and action_high[A]");
    template <class E2 = Env> static constexpr bool obs_space_sized() {
        if constexpr (DrilEnvHasObsSpace<E2>::value) return sizeof(E2::obs_low) == sizeof(float) * E2::D && sizeof(E2::obs_high) == sizeof(float) * E2::D; else return true;
    }
    static_assert(obs_space_sized(), "DRIL_ENV_PLUGIN: obs_low and obs_high must be float[D]");
    static constexpr bool ok = true;
};

template <class Env> constexpr DrilEnvPluginDesc dril_env_plugin_make_desc() {
    DrilEnvPluginDesc d{};
    d.abi_version = DRIL_ENV_PLUGIN_ABI; d.args_size = (uint32_t)sizeof(DrilEnvPluginArgs);
    d.S = Env::S; d.D = Env::D; d.A = Env::A; d.discrete = Env::discrete ? 1 : 0; d.episode_len = Env::episode_len;
    if constexpr (!Env::discrete && DrilEnvHasBounds<Env>::value) for (int i = 0; i < Env::A; ++i) { d.action_low[i] = Env::action_low[i]; d.action_high[i] = Env::action_high[i]; }
    for (int i = 0; i < 63 && Env::name[i]; ++i) d.name[i] = Env::name[i];
    return d;
}

// ---- the transition, per env ------------------------------------------------------------------------------------------------------------------------
template <class Env> DRIL_ENV_FN inline void dril_env_plugin_reset_one(const DrilEnvPluginArgs& a, int e) {
    float st[Env::S];
    Env::reset(DrilEnvRng{a.seed0 + (uint64_t)e, 0u}, st);
#pragma unroll
    for (int i = 0; i < Env::S; ++i) a.state[(size_t)e * Env::S + i] = st[i];
    a.step_count[e] = 0; a.episode[e] = 0; a.gstep[e] = 0;
}
// observe(env); scaled: observe(::ScalingWrapperEnv) (scalingWrapperEnv.jl:93-98) — the env's observation, then scale! per dimension
template <class Env, bool scaled> DRIL_ENV_FN inline void dril_env_plugin_emit_obs(const float* st, float* obs) {
    Env::observe(st, obs);
    if constexpr (scaled) {
#pragma unroll
        for (int i = 0; i < Env::D; ++i) obs[i] = dril::scale_to_unit(obs[i], Env::obs_low[i], Env::obs_high[i]);
    }
}
template <class Env, bool scaled = false> DRIL_ENV_FN inline void dril_env_plugin_observe_one(const DrilEnvPluginArgs& a, int e) {
    float st[Env::S];
#pragma unroll
    for (int i = 0; i < Env::S; ++i) st[i] = a.state[(size_t)e * Env::S + i];
    dril_env_plugin_emit_obs<Env, scaled>(st, a.obs + (size_t)e * Env::D);
}
// the declared observation space, low[D] | high[D], into a.obs (2 D floats): one env's worth of work, run once when the library loads the plug-in
template <class Env> DRIL_ENV_FN inline void dril_env_plugin_obs_space_one(const DrilEnvPluginArgs& a) {
    for (int i = 0; i < Env::D; ++i) { a.obs[i] = Env::obs_low[i]; a.obs[Env::D + i] = Env::obs_high[i]; }
}
// act! with auto-reset under MonitorWrapperEnv: the steps are those of env_step_kernel (load -> env_advance -> terminal observation -> env_end_episode -> store)
// scaled: act!(::ScalingWrapperEnv, action) (scalingWrapperEnv.jl:110-113) — the agent-facing action space is Box(-1, 1): ClampAdapter on it, then unscale! into the
// env's own bounds; every observation that leaves goes through scale!; reward, flags, counters, monitor sums and auto-reset are the env's own
template <class Env, bool scaled = false> DRIL_ENV_FN inline void dril_env_plugin_step_one(const DrilEnvPluginArgs& a, int e) {
    constexpr int S = Env::S, D = Env::D, A = Env::A;
    // 1. the cursor
    float st[S];
#pragma unroll
    for (int i = 0; i < S; ++i) st[i] = a.state[(size_t)e * S + i];
    int sc = a.step_count[e]; uint32_t ep = a.episode[e], gs = a.gstep[e];
    float mon_ret = a.mon_cur_ret ? a.mon_cur_ret[e] : 0.f; int mon_len = a.mon_cur_len ? a.mon_cur_len[e] : 0;
    // 2. to_env: DiscreteAdapter (a - action_start) | ClampAdapter per dimension (default_adapters.jl:4-11); the buffer keeps the raw action
    int act_i = 0; float act_f[Env::discrete ? 1 : A] = {};
    if constexpr (Env::discrete) act_i = ((const int32_t*)a.actions)[e] - a.action_start;
    else {
#pragma unroll
        for (int i = 0; i < A; ++i) {
            float v = ((const float*)a.actions)[(size_t)e * A + i];
            if constexpr (scaled) v = dril::unscale_from_unit(fminf(fmaxf(v, -1.0f), 1.0f), Env::action_low[i], Env::action_high[i]);
            else if (Env::action_low[i] < Env::action_high[i]) v = fminf(fmaxf(v, Env::action_low[i]), Env::action_high[i]);
            act_f[i] = v;
        }
    }
    // 3. the step
    bool term = false;
    const float rew = Env::step(st, act_f, act_i, &term);
    if (a.fixed_len) term = false;
    sc += 1; gs += 1;
    const bool trunc = sc >= a.episode_len;
    mon_ret += rew; mon_len += 1;
    // 4. results
    if (a.rewards) a.rewards[e] = rew;
    if (a.terminated) a.terminated[e] = term;
    if (a.truncated) a.truncated[e] = trunc;
    if (a.flags) a.flags[e] = (uint8_t)((term ? 1 : 0) | (trunc ? 2 : 0));
    // 5. terminal observation: of the state HERE, after the step and before the reset
    if (trunc && a.terminal_obs) dril_env_plugin_emit_obs<Env, scaled>(st, a.terminal_obs + (size_t)e * D);
    // 6. the episode ends: monitor, next episode
    if (term || trunc) {
        if (a.mon_cur_ret && a.ep_ret) { a.ep_ret[e] = mon_ret; a.ep_len[e] = mon_len; }
        ep += 1; sc = 0; Env::reset(DrilEnvRng{a.seed0 + (uint64_t)e, ep}, st);
        mon_ret = 0.f; mon_len = 0;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) a.state[(size_t)e * S + i] = st[i];
    a.step_count[e] = sc; a.episode[e] = ep; a.gstep[e] = gs;
    if (a.mon_cur_ret) { a.mon_cur_ret[e] = mon_ret; a.mon_cur_len[e] = mon_len; }
    // 7. the next observation
    if (a.obs) dril_env_plugin_emit_obs<Env, scaled>(st, a.obs + (size_t)e * D);
}

// ---- the optional entry points ----------------------------------------------------------------------------------------------------------------------
// An extern "C" definition inside the macro cannot depend on a constexpr condition, so the optional entry points are declared here and DEFINED as friends of a
// class template that DRIL_ENV_PLUGIN instantiates explicitly: the definitions exist in the specialisations that fit the env, and nowhere else.  A code object has
// dril_env_plugin_obs_space iff the env declares obs_low / obs_high, and the two _scaled kernels iff dril_env_plugin_scalable<Env>().
// (the friends' bodies are one call each: the work is in the function templates before them)
#if defined(DRIL_ENV_PLUGIN_HOST)
#define DRIL_ENV_PLUGIN_ENTRY(name) __attribute__((visibility("default"))) void dril_env_plugin_host_##name(const DrilEnvPluginArgs* a)
#define DRIL_ENV_PLUGIN_ENTRY_NAME(name) dril_env_plugin_host_##name
typedef const DrilEnvPluginArgs* DrilEnvPluginEntryArg;
template <class Env> inline void dril_env_plugin_run_obs_space(DrilEnvPluginEntryArg a) { dril_env_plugin_obs_space_one<Env>(*a); }
template <class Env> inline void dril_env_plugin_run_observe_scaled(DrilEnvPluginEntryArg a) { for (int e = 0; e < a->E; ++e) dril_env_plugin_observe_one<Env, true>(*a, e); }
template <class Env> inline void dril_env_plugin_run_step_scaled(DrilEnvPluginEntryArg a) { for (int e = 0; e < a->E; ++e) dril_env_plugin_step_one<Env, true>(*a, e); }
#else
// one thread per env, 256 threads per workgroup; the library launches ceil(E / 256) workgroups
#define DRIL_ENV_PLUGIN_BLOCK 256
#define DRIL_ENV_PLUGIN_ENTRY(name) __global__ void __launch_bounds__(DRIL_ENV_PLUGIN_BLOCK) dril_env_plugin_##name(DrilEnvPluginArgs a)
#define DRIL_ENV_PLUGIN_ENTRY_NAME(name) dril_env_plugin_##name
typedef DrilEnvPluginArgs DrilEnvPluginEntryArg;
template <class Env> __device__ inline void dril_env_plugin_run_obs_space(const DrilEnvPluginArgs& a) { if (blockIdx.x == 0 && threadIdx.x == 0) dril_env_plugin_obs_space_one<Env>(a); }
template <class Env> __device__ inline void dril_env_plugin_run_observe_scaled(const DrilEnvPluginArgs& a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e < a.E) dril_env_plugin_observe_one<Env, true>(a, e); }
template <class Env> __device__ inline void dril_env_plugin_run_step_scaled(const DrilEnvPluginArgs& a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e < a.E) dril_env_plugin_step_one<Env, true>(a, e); }
#endif
typedef void (*DrilEnvPluginEntry)(DrilEnvPluginEntryArg);
extern "C" { DRIL_ENV_PLUGIN_ENTRY(obs_space); DRIL_ENV_PLUGIN_ENTRY(observe_scaled); DRIL_ENV_PLUGIN_ENTRY(step_scaled); }
template <class Env, bool declared> struct DrilEnvPluginObsSpaceEntry {};
template <class Env> struct DrilEnvPluginObsSpaceEntry<Env, true> {
    friend DRIL_ENV_PLUGIN_ENTRY(obs_space) { dril_env_plugin_run_obs_space<Env>(a); }
    static constexpr DrilEnvPluginEntry obs_space = &DRIL_ENV_PLUGIN_ENTRY_NAME(obs_space);     // (the use that makes the friend's definition exist)
};
template <class Env, bool scalable> struct DrilEnvPluginScaledEntries {};
template <class Env> struct DrilEnvPluginScaledEntries<Env, true> {
    friend DRIL_ENV_PLUGIN_ENTRY(observe_scaled) { dril_env_plugin_run_observe_scaled<Env>(a); }
    friend DRIL_ENV_PLUGIN_ENTRY(step_scaled) { dril_env_plugin_run_step_scaled<Env>(a); }
    static constexpr DrilEnvPluginEntry observe_scaled = &DRIL_ENV_PLUGIN_ENTRY_NAME(observe_scaled), step_scaled = &DRIL_ENV_PLUGIN_ENTRY_NAME(step_scaled);
};
#define DRIL_ENV_PLUGIN_EMIT_OPTIONAL(Env)                                        \
    template struct DrilEnvPluginObsSpaceEntry<Env, DrilEnvHasObsSpace<Env>::value>; \
    template struct DrilEnvPluginScaledEntries<Env, dril_env_plugin_scalable<Env>()>;

#if defined(DRIL_ENV_PLUGIN_HOST)
#define DRIL_ENV_PLUGIN(Env)                                                                                                              \
    static_assert(DrilEnvPluginCheck<Env>::ok, "");                                                                                       \
    extern "C" {                                                                                                                          \
    extern const DrilEnvPluginDesc dril_env_plugin_desc = dril_env_plugin_make_desc<Env>();                                               \
    void dril_env_plugin_host_reset(const DrilEnvPluginArgs* a) { for (int e = 0; e < a->E; ++e) dril_env_plugin_reset_one<Env>(*a, e); }   \
    void dril_env_plugin_host_observe(const DrilEnvPluginArgs* a) { for (int e = 0; e < a->E; ++e) dril_env_plugin_observe_one<Env>(*a, e); } \
    void dril_env_plugin_host_step(const DrilEnvPluginArgs* a) { for (int e = 0; e < a->E; ++e) dril_env_plugin_step_one<Env>(*a, e); }   \
    }                                                                                                                                     \
    DRIL_ENV_PLUGIN_EMIT_OPTIONAL(Env)
#else
#define DRIL_ENV_PLUGIN(Env)                                                                                                              \
    static_assert(DrilEnvPluginCheck<Env>::ok, "");                                                                                       \
    extern "C" {                                                                                                                          \
    __device__ extern const DrilEnvPluginDesc dril_env_plugin_desc = dril_env_plugin_make_desc<Env>();                                    \
    __global__ void __launch_bounds__(DRIL_ENV_PLUGIN_BLOCK) dril_env_plugin_reset(DrilEnvPluginArgs a) {                                 \
        const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e < a.E) dril_env_plugin_reset_one<Env>(a, e); }                         \
    __global__ void __launch_bounds__(DRIL_ENV_PLUGIN_BLOCK) dril_env_plugin_observe(DrilEnvPluginArgs a) {                               \
        const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e < a.E) dril_env_plugin_observe_one<Env>(a, e); }                       \
    __global__ void __launch_bounds__(DRIL_ENV_PLUGIN_BLOCK) dril_env_plugin_step(DrilEnvPluginArgs a) {                                  \
        const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e < a.E) dril_env_plugin_step_one<Env>(a, e); }                          \
    }                                                                                                                                     \
    DRIL_ENV_PLUGIN_EMIT_OPTIONAL(Env)
#endif
