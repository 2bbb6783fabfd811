// dril_env_world.h — the second, optional form of a DEVICE ENV PLUG-IN: a WORLD of N agents that share one state and take one joint step.  It is the device form of
// MultiAgentParallelEnv (environment_wrappers/multiAgentParallelEnv.jl): there every simulation is a parallel env whose agents are its sub-envs, and all of them are
// stacked into one batch (vcat in observe, chunked actions in act!); here the library sees agent i of world w as ROW w N + i — the same stacking — and everything above
// the env side (policy forward, per-row action noise, rollout buffer, GAE, update, monitor, normaliser, evaluation accounting) works per row as it does for
// DRIL_ENV_PLUGIN.  One shared policy trains on agents that collide, cooperate or compete inside one state.
//
//     #include "device/dril_env_world.h"
//     struct MyWorld {
//         static constexpr int  N = 3;                 // agents per world, 2..16
//         static constexpr int  S = 12;                // state floats per WORLD, 1..256
//         static constexpr int  D = 8, A = 2;          // per agent: observation dims, action dims (Discrete: number of actions)
//         static constexpr bool discrete = false;
//         static constexpr int  episode_len = 50;
//         static constexpr float action_low[A] = {-1, -1}, action_high[A] = {1, 1};     // per agent; continuous worlds only
//         static constexpr const char* name = "MyWorld";
//         DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st);
//         DRIL_ENV_FN static void observe(const float* st, int agent, float* obs);
//         DRIL_ENV_FN static void step(float* st, const float* act_f /* N x A, agent-major */, const int* act_i /* N */,
//                                      float* rew /* N */, bool* terminated /* of the world */);
//     };
//     DRIL_ENV_PLUGIN_WORLD(MyWorld)
//
// THE ABI DOES NOT CHANGE.  The macro emits the symbols of DRIL_ENV_PLUGIN — dril_env_plugin_desc, dril_env_plugin_reset, dril_env_plugin_observe, dril_env_plugin_step —
// which take the same DrilEnvPluginArgs and the same launch geometry: E is the number of ROWS (a multiple of N; the library checks it), 256 threads per workgroup,
// ceil(E / 256) workgroups.  The descriptor's former `reserved` word is `agents`: N for a world, 0 for every code object built with DRIL_ENV_PLUGIN, before or after this
// header existed — so the word keeps the meaning it had in all of them, neither the descriptor nor the argument block changes size, and DRIL_ENV_PLUGIN_ABI stays 1.
// S in the descriptor is the world's; D and A are per agent.  A world emits no obs_space and no _scaled entry, and has no fused rollout / evaluation yet
// (DRIL_ENV_PLUGIN_ROLLOUT / DRIL_ENV_PLUGIN_EVALUATE on a world stop at a static_assert).
//
// Layout.  World w's state is the S floats at state + w S.  Every per-row array (actions, rewards, flags, observations, counters, monitor sums) is indexed by the row
// w N + i exactly as a classic plug-in indexes it by env.  step_count / episode / gstep stay per-row arrays; the N rows of a world always hold equal values.
// Seeds.  world_seed = seed0 + w N, the global row index of the world's agent 0 (seed0 = seed + rank n_envs): a world's stream depends neither on the rank layout nor on
// n_envs.  (The reference seeds sub-env i of a MultiAgentParallelEnv with seed + i - 1, which overlaps between neighbours: docs/deviations.md.)
// Threads.  reset and step: thread w < E / N owns world w.  observe: thread e < E owns row e (world e / N, agent e % N), so a world's rows may straddle two workgroups;
// nothing is shared between threads.  What a world computes does not depend on how many worlds there are or where it sits (batch invariance).
//
// The transition is written once, here, with the steps and the order of dril_env_plugin_step_one; termination and truncation are the WORLD's and go into all N rows.
// With DRIL_ENV_PLUGIN_HOST the header compiles with a plain C++17 compiler and exports dril_env_plugin_host_reset / _observe / _step: serial loops over the same
// per-world functions.
#pragma once
#include "dril_env_plugin.h"

#define DRIL_ENV_WORLD_MIN_N 2       // agents per world
#define DRIL_ENV_WORLD_MAX_N 16
#define DRIL_ENV_WORLD_MAX_S 256     // state floats per world
#define DRIL_ENV_WORLD_MAX_ACT 256   // N x A floats of one joint continuous action

template <class World> struct DrilEnvWorldCheck {
    static_assert(World::N >= DRIL_ENV_WORLD_MIN_N && World::N <= DRIL_ENV_WORLD_MAX_N, "DRIL_ENV_PLUGIN_WORLD: N (agents per world) must be 2..16");
    static_assert(World::S >= 1 && World::S <= DRIL_ENV_WORLD_MAX_S, "DRIL_ENV_PLUGIN_WORLD: S (state floats per world) must be 1..256");
    static_assert(World::D >= 1 && World::D <= DRIL_ENV_PLUGIN_MAX_D, "DRIL_ENV_PLUGIN_WORLD: D (observation dims per agent) must be 1..1024");
    static_assert(World::A >= 1 && World::A <= DRIL_ENV_PLUGIN_MAX_A, "DRIL_ENV_PLUGIN_WORLD: A (action dims per agent, or number of discrete actions) must be 1..64");
    static_assert(World::discrete || World::N * World::A <= DRIL_ENV_WORLD_MAX_ACT, "DRIL_ENV_PLUGIN_WORLD: N x A (floats of one joint continuous action) must be <= 256");
    static_assert(World::episode_len >= 1, "DRIL_ENV_PLUGIN_WORLD: episode_len (the default time limit) must be >= 1");
    static_assert(World::discrete || DrilEnvHasBounds<World>::value, "DRIL_ENV_PLUGIN_WORLD: a continuous world (discrete = false) must define static constexpr float action_low[A] and action_high[A]");
    static constexpr bool ok = true;
};

template <class World> constexpr DrilEnvPluginDesc dril_env_world_make_desc() {
    DrilEnvPluginDesc d = dril_env_plugin_make_desc<World>();
    d.agents = World::N;
    return d;
}

// ---- the transition, per world ------------------------------------------------------------------------------------------------------------------------
template <class World> DRIL_ENV_FN inline void dril_env_world_reset_one(const DrilEnvPluginArgs& a, int w) {
    constexpr int N = World::N, S = World::S;
    float st[S];
    World::reset(DrilEnvRng{a.seed0 + (uint64_t)w * N, 0u}, st);
    for (int i = 0; i < S; ++i) a.state[(size_t)w * S + i] = st[i];
    for (int i = 0; i < N; ++i) { const size_t r = (size_t)w * N + i; a.step_count[r] = 0; a.episode[r] = 0; a.gstep[r] = 0; }
}
// observe(env) of row e: agent e % N of world e / N, read from the world's state where it lies
template <class World> DRIL_ENV_FN inline void dril_env_world_observe_row(const DrilEnvPluginArgs& a, int e) {
    constexpr int N = World::N;
    const int w = e / N;
    World::observe(a.state + (size_t)w * World::S, e - w * N, a.obs + (size_t)e * World::D);
}
// act! of one world with auto-reset under MonitorWrapperEnv: dril_env_plugin_step_one's steps in its order, over the N rows of world w
template <class World> DRIL_ENV_FN inline void dril_env_world_step_one(const DrilEnvPluginArgs& a, int w) {
    constexpr int N = World::N, S = World::S, D = World::D, A = World::A;
    const size_t r0 = (size_t)w * N;                                               // the world's first row
    // 1. the cursor: the counters of agent 0's row (the N rows hold equal values), the monitor's sums per row
    float st[S];
    for (int i = 0; i < S; ++i) st[i] = a.state[(size_t)w * S + i];
    int sc = a.step_count[r0]; uint32_t ep = a.episode[r0], gs = a.gstep[r0];
    float mon_ret[N]; int mon_len[N];
    for (int i = 0; i < N; ++i) { mon_ret[i] = a.mon_cur_ret ? a.mon_cur_ret[r0 + i] : 0.f; mon_len[i] = a.mon_cur_len ? a.mon_cur_len[r0 + i] : 0; }
    // 2. to_env per agent: DiscreteAdapter (a - action_start) | ClampAdapter per dimension; the buffer keeps the raw action
    int act_i[N] = {}; float act_f[World::discrete ? 1 : N * A] = {};
    if constexpr (World::discrete) { for (int i = 0; i < N; ++i) act_i[i] = ((const int32_t*)a.actions)[r0 + i] - a.action_start; }
    else {
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int k = 0; k < A; ++k) {
                float v = ((const float*)a.actions)[(r0 + i) * A + k];
                if (World::action_low[k] < World::action_high[k]) v = fminf(fmaxf(v, World::action_low[k]), World::action_high[k]);
                act_f[i * A + k] = v;
            }
        }
    }
    // 3. the joint step
    float rew[N]; bool term = false;
    World::step(st, act_f, act_i, rew, &term);
    if (a.fixed_len) term = false;
    sc += 1; gs += 1;
    const bool trunc = sc >= a.episode_len;
    for (int i = 0; i < N; ++i) { mon_ret[i] += rew[i]; mon_len[i] += 1; }
    // 4. results: each agent its own reward, the world's flags into all N rows
    const uint8_t fl = (uint8_t)((term ? 1 : 0) | (trunc ? 2 : 0));
    for (int i = 0; i < N; ++i) {
        if (a.rewards) a.rewards[r0 + i] = rew[i];
        if (a.terminated) a.terminated[r0 + i] = term;
        if (a.truncated) a.truncated[r0 + i] = trunc;
        if (a.flags) a.flags[r0 + i] = fl;
    }
    // 5. terminal observation of every agent: of the state HERE, after the step and before the reset
    if (trunc && a.terminal_obs) for (int i = 0; i < N; ++i) World::observe(st, i, a.terminal_obs + (r0 + i) * D);
    // 6. the episode ends: monitor per row, next episode of the world
    if (term || trunc) {
        if (a.mon_cur_ret && a.ep_ret) for (int i = 0; i < N; ++i) { a.ep_ret[r0 + i] = mon_ret[i]; a.ep_len[r0 + i] = mon_len[i]; }
        ep += 1; sc = 0; World::reset(DrilEnvRng{a.seed0 + (uint64_t)r0, ep}, st);
        for (int i = 0; i < N; ++i) { mon_ret[i] = 0.f; mon_len[i] = 0; }
    }
    for (int i = 0; i < S; ++i) a.state[(size_t)w * S + i] = st[i];
    for (int i = 0; i < N; ++i) {
        a.step_count[r0 + i] = sc; a.episode[r0 + i] = ep; a.gstep[r0 + i] = gs;
        if (a.mon_cur_ret) { a.mon_cur_ret[r0 + i] = mon_ret[i]; a.mon_cur_len[r0 + i] = mon_len[i]; }
    }
    // 7. the next observation of every agent
    if (a.obs) for (int i = 0; i < N; ++i) World::observe(st, i, a.obs + (r0 + i) * D);
}

#if defined(DRIL_ENV_PLUGIN_HOST)
#define DRIL_ENV_PLUGIN_WORLD(World)                                                                                                      \
    static_assert(DrilEnvWorldCheck<World>::ok, "");                                                                                      \
    extern "C" {                                                                                                                          \
    extern const DrilEnvPluginDesc dril_env_plugin_desc = dril_env_world_make_desc<World>();                                              \
    void dril_env_plugin_host_reset(const DrilEnvPluginArgs* a) { for (int w = 0; w < a->E / World::N; ++w) dril_env_world_reset_one<World>(*a, w); } \
    void dril_env_plugin_host_observe(const DrilEnvPluginArgs* a) { for (int e = 0; e < a->E; ++e) dril_env_world_observe_row<World>(*a, e); } \
    void dril_env_plugin_host_step(const DrilEnvPluginArgs* a) { for (int w = 0; w < a->E / World::N; ++w) dril_env_world_step_one<World>(*a, w); } \
    }
#else
#define DRIL_ENV_PLUGIN_WORLD(World)                                                                                                      \
    static_assert(DrilEnvWorldCheck<World>::ok, "");                                                                                      \
    extern "C" {                                                                                                                          \
    __device__ extern const DrilEnvPluginDesc dril_env_plugin_desc = dril_env_world_make_desc<World>();                                   \
    __global__ void __launch_bounds__(DRIL_ENV_PLUGIN_BLOCK) dril_env_plugin_reset(DrilEnvPluginArgs a) {                                 \
        const int w = blockIdx.x * blockDim.x + threadIdx.x; if (w < a.E / World::N) dril_env_world_reset_one<World>(a, w); }             \
    __global__ void __launch_bounds__(DRIL_ENV_PLUGIN_BLOCK) dril_env_plugin_observe(DrilEnvPluginArgs a) {                               \
        const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e < a.E) dril_env_world_observe_row<World>(a, e); }                      \
    __global__ void __launch_bounds__(DRIL_ENV_PLUGIN_BLOCK) dril_env_plugin_step(DrilEnvPluginArgs a) {                                  \
        const int w = blockIdx.x * blockDim.x + threadIdx.x; if (w < a.E / World::N) dril_env_world_step_one<World>(a, w); }              \
    }
#endif
