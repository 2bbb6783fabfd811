// dril_env_rollout.h — the FUSED ROLLOUT of a device env plug-in: one launch per PPO collection.
//
// A plug-in author adds two lines to a source that ends in DRIL_ENV_PLUGIN(MyEnv):
//
//     #include "device/dril_env_rollout.h"
//     DRIL_ENV_PLUGIN_ROLLOUT(MyEnv)
//
// and the code object gains dril_env_plugin_rollout, dril_env_plugin_rollout_scaled (exactly when dril_env_plugin_scalable<MyEnv>(), the rule of the other _scaled
// kernels) and the descriptor dril_env_plugin_rollout_desc.  The library cannot link a separately compiled env into its own kernels, so the policy comes to the env:
// the kernel is instantiated by the plug-in's compile with Env inlined.  dril_rollout_fused_enable (include/dril_hip.h) switches a handle to it; the step-granular
// collection (policy launches + the plug-in's step kernel, per env step) stays the default.  DrilEnvPluginDesc, DrilEnvPluginArgs and DRIL_ENV_PLUGIN_ABI do not change,
// and a source without the second macro compiles to exactly the symbols it had.
//
// One launch does, for the envs of its workgroup, collect_trajectories (trajectory.jl:22-78) in the order of the library's step-granular loop: the opening observe;
// for t = 0 .. T-1 the observation into row t, critic and actor forward, the Categorical / DiagGaussian draw with its log-probability and the value into row t, the
// transition (dril_env_plugin_step_one: the ONE definition, called with an argument block that points at row t), V(terminal_observation) of the envs truncated in this
// step into row t of the bootstrap buffer; at the end V(observation after the last step).  GAE stays the library's launch.
//
// The kernel: a workgroup owns a tile of DRIL_ENV_ROLLOUT_TILE envs for all T steps.  The forward is policy_act_kernel's (dril_policy.hip): the tile's envs are the
// columns of two activation panels [width][tile] that ping-pong in LDS, lane = output row, weights streamed from global memory (L2-resident after the first step), plain
// f32 FMA with k ascending and one accumulator per (row, column) — so the rows of env e are the same bits whatever E is and whichever tile e falls into.  The critic
// and the actor run through the same loop: side by side in one pass while twice the widest hidden layer fits a panel, one after the other otherwise.  A workgroup reads back from global memory only what it wrote itself; the only synchronisation is the
// workgroup barrier: no grid barrier, no cooperative launch, no atomics, no spin-waits.  Workgroups beyond what is resident start when others have finished.
// A parameter vector of up to DRIL_ENV_ROLLOUT_STAGE_FLOATS floats (default 11 264 = 44 KB: both [64,64] nets) is copied into LDS once per launch and read from
// there — the same floats in the same order, so staging changes no result; larger nets stream from L2.
// The panels are sized statically by DRIL_ENV_ROLLOUT_MAX_WIDTH (default 256: 32 KB with a tile of 16), the widest layer (and observation) the kernel takes; the library
// refuses a wider net with a message that names the define.
//
// With DRIL_ENV_PLUGIN_HOST the macro emits dril_env_plugin_host_rollout (and _scaled): the same per-env functions — transition, head, the k-ascending fmaf chain of a
// dense row — in a serial loop over envs and steps, for gdb, host sanitizers and CPU tests.
#pragma once
#include "dril_env_plugin.h"
#include "dril_activations.h"
#include "dril_policy_head.h"

#ifndef DRIL_ENV_ROLLOUT_ABI
#define DRIL_ENV_ROLLOUT_ABI 1u          // bumps whenever DrilEnvRolloutDesc / DrilEnvRolloutArgs or the meaning of a field changes
#endif
#ifndef DRIL_ENV_ROLLOUT_MAX_WIDTH
#define DRIL_ENV_ROLLOUT_MAX_WIDTH 256   // widest hidden layer / observation / action row the LDS panels hold
#endif
#ifndef DRIL_ENV_ROLLOUT_TILE
#define DRIL_ENV_ROLLOUT_TILE 16         // envs per workgroup (a multiple of 4)
#endif
#ifndef DRIL_ENV_ROLLOUT_STAGE_FLOATS
#if DRIL_ENV_ROLLOUT_MAX_WIDTH * DRIL_ENV_ROLLOUT_TILE <= 4096
#define DRIL_ENV_ROLLOUT_STAGE_FLOATS 11264   // parameter vectors up to this many floats (44 KB: two [64,64] nets) are copied into LDS once per launch; with the
                                              // default panels a workgroup then holds 76 KB, so two of them share a CU's 160 KB
#else
#define DRIL_ENV_ROLLOUT_STAGE_FLOATS 0       // larger panels keep the LDS to themselves: the parameters stream from L2
#endif
#endif
#define DRIL_ENV_ROLLOUT_THREADS 256     // threads per workgroup: 4 waves; a wave owns 64 output rows x 4 columns at a time
#define DRIL_ENV_ROLLOUT_MAX_HIDDEN 4

struct DrilEnvRolloutDesc {
    uint32_t abi_version;                // DRIL_ENV_ROLLOUT_ABI the plug-in was compiled against
    uint32_t args_size;                  // sizeof(DrilEnvRolloutArgs) the plug-in was compiled against
    int32_t tile, threads, max_width, has_scaled, reserved[2];
};

// The argument block of the rollout kernels (passed by value).  Pointers are device pointers.
struct DrilEnvRolloutArgs {
    DrilEnvPluginArgs env;               // E, time limit, seed0, state and counters, monitor sums; terminated / truncated / terminal_obs / obs: the per-step arrays (E), all set
    int32_t T, n_hidden, activation, n_params;   // n_params: floats of the whole parameter vector (both nets and log_std)
    int32_t hidden[DRIL_ENV_ROLLOUT_MAX_HIDDEN];
    int32_t actor_off, critic_off, log_std_off, reserved2;   // into params; a net is {W_1 b_1 ... W_{n+1} b_{n+1}}, W column-major (out x in)
    const float* params;
    const void* noise;                   // null: stream 1 at the env's gstep; else the injected table, f64 (T x E) | f32 (T x E x A), row t E + e
    float* obs; void* act; float* rew; float* logp; float* val; float* boot; uint8_t* flags; float* last_values;   // the rollout buffers, row t = (t E + e)
    float* ep_ret; int32_t* ep_len;      // (T x E): MonitorWrapperEnv's finished episodes (null = no monitor)
};

// a world (device/dril_env_world.h: N agents per state) is told from an env by its N
template <class Env, class = void> struct DrilEnvIsWorld { static constexpr bool value = false; };
template <class Env> struct DrilEnvIsWorld<Env, decltype((void)Env::N, void())> { static constexpr bool value = true; };

template <class Env> struct DrilEnvRolloutCheck {
    static_assert(!DrilEnvIsWorld<Env>::value, "DRIL_ENV_PLUGIN_ROLLOUT / DRIL_ENV_PLUGIN_EVALUATE: a world (DRIL_ENV_PLUGIN_WORLD) has no fused rollout or evaluation yet: leave the macro out, the library collects and evaluates a world step-granular");
    static_assert(DRIL_ENV_ROLLOUT_TILE >= 4 && DRIL_ENV_ROLLOUT_TILE % 4 == 0 && DRIL_ENV_ROLLOUT_TILE <= DRIL_ENV_ROLLOUT_THREADS, "DRIL_ENV_PLUGIN_ROLLOUT: DRIL_ENV_ROLLOUT_TILE must be a multiple of 4 in 4..256");
    static_assert(Env::D <= DRIL_ENV_ROLLOUT_MAX_WIDTH && Env::A <= DRIL_ENV_ROLLOUT_MAX_WIDTH, "DRIL_ENV_PLUGIN_ROLLOUT: D and A must fit DRIL_ENV_ROLLOUT_MAX_WIDTH");
    static_assert(8 * DRIL_ENV_ROLLOUT_MAX_WIDTH * DRIL_ENV_ROLLOUT_TILE + 4 * DRIL_ENV_ROLLOUT_STAGE_FLOATS + 1024 <= 160 * 1024, "DRIL_ENV_PLUGIN_ROLLOUT: the two activation panels (8 x DRIL_ENV_ROLLOUT_MAX_WIDTH x DRIL_ENV_ROLLOUT_TILE bytes) and the staged parameters (4 x DRIL_ENV_ROLLOUT_STAGE_FLOATS bytes) must fit the 160 KB of LDS of a gfx950 CU");
    static constexpr bool ok = true;
};
template <class Env> constexpr DrilEnvRolloutDesc dril_env_rollout_make_desc() {
    DrilEnvRolloutDesc d{};
    d.abi_version = DRIL_ENV_ROLLOUT_ABI; d.args_size = (uint32_t)sizeof(DrilEnvRolloutArgs);
    d.tile = DRIL_ENV_ROLLOUT_TILE; d.threads = DRIL_ENV_ROLLOUT_THREADS; d.max_width = DRIL_ENV_ROLLOUT_MAX_WIDTH; d.has_scaled = dril_env_plugin_scalable<Env>() ? 1 : 0;
    return d;
}

// ---- per (row, columns) and per env: shared by the kernel and the host build ----------------------------------------------------------------------------
// rows [o] x NC columns of one Dense layer: acc_j = sum_k W[o][k] x[k][j], k ascending, one FMA per term.  W: the column-major (out x in) matrix at row o; x: the
// input at the unit's first column, xs floats from one k to the next
template <int NC> DRIL_ENV_FN inline void dril_rollout_dense_unit(const float* W, int O, int K, const float* x, int xs, float (&acc)[NC]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.f;
    constexpr int U = 16;                                                            // weight lines kept in flight
    int k = 0;
    for (; k + U <= K; k += U) {
        float w[U];
#pragma unroll
        for (int i = 0; i < U; ++i) w[i] = W[(size_t)(k + i) * O];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const float* xk = x + (size_t)(k + i) * xs;
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = __builtin_fmaf(w[i], xk[j], acc[j]);
        }
    }
    for (; k < K; ++k) {
        const float w = W[(size_t)k * O]; const float* xk = x + (size_t)k * xs;
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[j] = __builtin_fmaf(w, xk[j], acc[j]);
    }
}
DRIL_ENV_FN inline float dril_rollout_dense_finish(float acc, float bias, bool hidden, int activation) {
    const float v = acc + bias;
    return hidden ? dril::activation_forward(activation, v) : v;
}
// the sampling head of env e at step t, as generic_policy_head_kernel (mode 0): z = the actor's output row (stride zs), v = the critic's value
template <class Env> DRIL_ENV_FN inline void dril_rollout_head_one(const DrilEnvRolloutArgs& g, int t, int e, const float* z, int zs, float v) {
    constexpr int A = Env::A;
    const size_t b = (size_t)t * g.env.E + e;
    const uint64_t seed = g.env.seed0 + (uint64_t)e; const uint32_t gs = g.env.gstep[e];
    if constexpr (Env::discrete) {
        float m, s; dril::softmax_stats(z, A, m, s, zs);
        const double u = g.noise ? ((const double*)g.noise)[b] : dril::env_noise_u01(seed, gs);
        const int act = dril::categorical_draw(z, A, m, s, u, zs);
        ((int32_t*)g.act)[b] = act + g.env.action_start;
        g.logp[b] = dril::categorical_logp(z, act, m, s, zs);
    } else {
        const float* ls = g.params + g.log_std_off;
        float* x = (float*)g.act + b * A;
        for (int k = 0; k < A; ++k) {
            const float n01 = g.noise ? ((const float*)g.noise)[b * A + k] : dril::env_noise_randn(seed, gs, k);
            x[k] = dril::gauss_draw(z[k * zs], ls[k], n01);
        }
        g.logp[b] = dril::gauss_logpdf_rt(x, z, ls, A, zs);
    }
    g.val[b] = v;
}
// the transition of env e at step t: dril_env_plugin_step_one on an argument block that points at row t; true when the env was truncated (its terminal observation
// is in g.env.terminal_obs and wants a bootstrap value)
template <class Env, bool scaled> DRIL_ENV_FN inline bool dril_rollout_transition_one(const DrilEnvRolloutArgs& g, int t, int e) {
    const size_t k = (size_t)t * g.env.E;
    DrilEnvPluginArgs s = g.env;
    s.actions = Env::discrete ? (const void*)((const int32_t*)g.act + k) : (const void*)((const float*)g.act + k * Env::A);
    s.rewards = g.rew + k; s.flags = g.flags + k;
    if (g.ep_ret) { s.ep_ret = g.ep_ret + k; s.ep_len = g.ep_len + k; } else { s.ep_ret = nullptr; s.ep_len = nullptr; }
    dril_env_plugin_step_one<Env, scaled>(s, e);
    return g.env.truncated[e] != 0;
}
// layer l of a net that starts at `off`: its input and output widths and where its W sits (b follows W)
struct DrilRolloutLayer { int K, O, w; };
DRIL_ENV_FN inline DrilRolloutLayer dril_rollout_layer_of(const DrilEnvRolloutArgs& g, int D, int out, int off, int l) {
    DrilRolloutLayer r{D, 0, off};
    for (int i = 0;; ++i) {
        r.O = i == g.n_hidden ? out : g.hidden[i];
        if (i == l) return r;
        r.w += r.K * r.O + r.O; r.K = r.O;
    }
}

#if defined(DRIL_ENV_PLUGIN_HOST)
// ---- the host build: the same per-env functions in a serial loop -------------------------------------------------------------------------------------------
// net(x) of one env; x and y: DRIL_ENV_ROLLOUT_MAX_WIDTH floats each; returns where the output row is
inline const float* dril_rollout_host_net(const DrilEnvRolloutArgs& g, int D, int out, int off, const float* obs, float* x, float* y) {
    for (int k = 0; k < D; ++k) x[k] = obs[k];
    for (int l = 0; l <= g.n_hidden; ++l) {
        const DrilRolloutLayer L = dril_rollout_layer_of(g, D, out, off, l);
        const float* W = g.params + L.w; const float* bias = W + (size_t)L.K * L.O;
        for (int o = 0; o < L.O; ++o) { float acc[1]; dril_rollout_dense_unit<1>(W + o, L.O, L.K, x, 1, acc); y[o] = dril_rollout_dense_finish(acc[0], bias[o], l < g.n_hidden, g.activation); }
        float* t = x; x = y; y = t;
    }
    return x;
}
template <class Env, bool scaled> inline void dril_env_rollout_host(const DrilEnvRolloutArgs& g) {
    constexpr int D = Env::D;
    float x[DRIL_ENV_ROLLOUT_MAX_WIDTH], y[DRIL_ENV_ROLLOUT_MAX_WIDTH];
    for (int e = 0; e < g.env.E; ++e) {
        float* cur = g.env.obs + (size_t)e * D;
        dril_env_plugin_observe_one<Env, scaled>(g.env, e);
        for (int t = 0; t < g.T; ++t) {
            const size_t b = (size_t)t * g.env.E + e;
            for (int k = 0; k < D; ++k) g.obs[b * D + k] = cur[k];
            const float v = dril_rollout_host_net(g, D, 1, g.critic_off, cur, x, y)[0];
            const float* z = dril_rollout_host_net(g, D, Env::A, g.actor_off, cur, x, y);
            dril_rollout_head_one<Env>(g, t, e, z, 1, v);
            const bool trunc = dril_rollout_transition_one<Env, scaled>(g, t, e);
            g.boot[b] = trunc ? dril_rollout_host_net(g, D, 1, g.critic_off, g.env.terminal_obs + (size_t)e * D, x, y)[0] : 0.f;
        }
        g.last_values[e] = dril_rollout_host_net(g, D, 1, g.critic_off, cur, x, y)[0];
    }
}
#define DRIL_ENV_ROLLOUT_ENTRY(name) __attribute__((visibility("default"))) void dril_env_plugin_host_##name(const DrilEnvRolloutArgs* g)
#define DRIL_ENV_ROLLOUT_IMPL dril_env_rollout_host
#define DRIL_ENV_ROLLOUT_RUN(Env, scaled) DrilEnvRolloutBody<Env, scaled>::run(*g)
#define DRIL_ENV_ROLLOUT_DESC_QUAL
#else
// ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------------
// (always inlined: a code object may call the body from more than one kernel — dril_env_rollout_pop.h —, and an out-of-line copy would take the argument block and the
// parameter vector by generic pointers, turning the kernel's global and LDS accesses into flat ones; with one caller the compiler inlined them anyway)
#define DRIL_ENV_ROLLOUT_INLINE __attribute__((always_inline)) inline
// the tile's rows of a (E x D) array as panel [k][c]: column c = env e0 + c; columns past the batch, and columns with where[e] == 0, are zero
template <int TC> __device__ DRIL_ENV_ROLLOUT_INLINE void dril_rollout_load_panel(float* panel, const float* src, const uint8_t* where, int D, int e0, int ncol) {
    for (int i = threadIdx.x; i < D * TC; i += DRIL_ENV_ROLLOUT_THREADS) {
        const int c = i / D, k = i - c * D;
        float v = 0.f;
        if (c < ncol && (!where || where[e0 + c])) v = src[(size_t)(e0 + c) * D + k];
        panel[k * TC + c] = v;
    }
}
// net(panel `in`) for the tile's columns; both panels are clobbered; returns the panel whose rows 0 .. out-1 hold the output.  Ends behind a barrier
template <int TC> __device__ DRIL_ENV_ROLLOUT_INLINE const float* dril_rollout_net(const DrilEnvRolloutArgs& g, const float* P, int D, int out, int off, float* in, float* other) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int K = D, w = off;
    for (int l = 0; l <= g.n_hidden; ++l) {
        const int O = l == g.n_hidden ? out : g.hidden[l];
        const float* __restrict__ W = P + w; const float* __restrict__ bias = W + (size_t)K * O;
        const int nrt = (O + 63) >> 6, units = nrt * (TC / 4);
        const bool hidden = l < g.n_hidden;
        for (int u = wave; u < units; u += DRIL_ENV_ROLLOUT_THREADS / 64) {           // unit = 64 rows x 4 columns
            const int cg = u / nrt, o = (u - cg * nrt) * 64 + lane, cb = cg * 4;
            if (o >= O) continue;
            float acc[4]; dril_rollout_dense_unit<4>(W + o, O, K, in + cb, TC, acc);
            const float bo = bias[o];
            float4 v;
            v.x = dril_rollout_dense_finish(acc[0], bo, hidden, g.activation); v.y = dril_rollout_dense_finish(acc[1], bo, hidden, g.activation);
            v.z = dril_rollout_dense_finish(acc[2], bo, hidden, g.activation); v.w = dril_rollout_dense_finish(acc[3], bo, hidden, g.activation);
            *(float4*)(other + o * TC + cb) = v;
        }
        __syncthreads();
        float* t = in; in = other; other = t;
        w += K * O + O; K = O;
    }
    return in;
}
// both nets on the panel `in` in ONE pass (their hidden layers have the same shapes): net z's activations are rows [z W, (z + 1) W) of a panel, so this form needs
// 2 x the widest hidden layer <= DRIL_ENV_ROLLOUT_MAX_WIDTH.  Returns the panel whose rows 0 .. A-1 hold the actor's output and row A the critic's value.  A (row,
// column) is the same chain of FMAs as in dril_rollout_net: which form ran changes no result.  Ends behind a barrier
template <int TC> __device__ DRIL_ENV_ROLLOUT_INLINE const float* dril_rollout_both(const DrilEnvRolloutArgs& g, const float* P, int D, int A, float* in, float* other) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int K = D, wa = g.actor_off, wc = g.critic_off;
    for (int l = 0; l <= g.n_hidden; ++l) {
        const bool hidden = l < g.n_hidden;
        const int Oa = hidden ? g.hidden[l] : A, Oc = hidden ? g.hidden[l] : 1;
        const int nra = (Oa + 63) >> 6, nr = nra + ((Oc + 63) >> 6), units = nr * (TC / 4);
        for (int u = wave; u < units; u += DRIL_ENV_ROLLOUT_THREADS / 64) {           // unit = 64 rows of one net x 4 columns
            const int cg = u / nr, r = u - cg * nr, z = r >= nra ? 1 : 0, o = (z ? r - nra : r) * 64 + lane, cb = cg * 4, O = z ? Oc : Oa;
            if (o >= O) continue;
            const float* __restrict__ W = P + (z ? wc : wa); const float* __restrict__ bias = W + (size_t)K * O;
            float acc[4]; dril_rollout_dense_unit<4>(W + o, O, K, in + (l == 0 ? 0 : z * K * TC) + cb, TC, acc);
            const float bo = bias[o];
            float4 v;
            v.x = dril_rollout_dense_finish(acc[0], bo, hidden, g.activation); v.y = dril_rollout_dense_finish(acc[1], bo, hidden, g.activation);
            v.z = dril_rollout_dense_finish(acc[2], bo, hidden, g.activation); v.w = dril_rollout_dense_finish(acc[3], bo, hidden, g.activation);
            *(float4*)(other + ((z ? Oa : 0) + o) * TC + cb) = v;
        }
        __syncthreads();
        float* t = in; in = other; other = t;
        wa += K * Oa + Oa; wc += K * Oc + Oc; K = Oa;
    }
    return in;
}
// all T steps of the workgroup's tile; P: the parameter vector the forward reads — global memory, or its copy in LDS (the address space is known at each call site)
template <class Env, bool scaled> __device__ DRIL_ENV_ROLLOUT_INLINE void dril_env_rollout_steps(const DrilEnvRolloutArgs& g, const float* P, float* p0, float* p1, float* values, int* any_truncated) {
    constexpr int TC = DRIL_ENV_ROLLOUT_TILE, D = Env::D;
    const int tid = threadIdx.x, E = g.env.E, e0 = blockIdx.x * TC;
    const int ncol = E - e0 < TC ? E - e0 : TC, e = e0 + tid;
    const bool mine = tid < ncol;                                                     // thread c steps env e0 + c
    int widest = 0; for (int l = 0; l < g.n_hidden; ++l) widest = g.hidden[l] > widest ? g.hidden[l] : widest;
    const bool both = 2 * widest <= DRIL_ENV_ROLLOUT_MAX_WIDTH && Env::A + 1 <= DRIL_ENV_ROLLOUT_MAX_WIDTH;   // the two nets fit a panel side by side
    if (mine) dril_env_plugin_observe_one<Env, scaled>(g.env, e);                     // new_obs = observe(env), trajectory.jl:32
    __syncthreads();
    for (int t = 0; t <= g.T; ++t) {                                                  // t == T: V(new_obs) for rollout-limited tails, :65-70
        const size_t row = (size_t)t * E;
        bool trunc = false;
        // pass 0: V(obs);  pass 1: the actor, the draw, the transition;  pass 2: V(terminal_observation) of the envs truncated in this step, :57-61.
        // both: pass 1 runs both nets side by side and pass 0 is left out
#pragma unroll 1
        for (int pass = (both && t < g.T) ? 1 : 0; pass < 3; ++pass) {
            if (pass == 2 && !*any_truncated) { if (mine) g.boot[row + e] = 0.f; break; }
            const bool first = pass == 0 || (both && pass == 1);
            dril_rollout_load_panel<TC>(p0, pass == 2 ? g.env.terminal_obs : g.env.obs, pass == 2 ? g.env.truncated : nullptr, D, e0, ncol);
            if (first && t < g.T) for (int i = tid; i < ncol * D; i += DRIL_ENV_ROLLOUT_THREADS) g.obs[(row + e0) * D + i] = g.env.obs[(size_t)e0 * D + i];   // the observation -> row t
            __syncthreads();
            if (first && tid == 0) *any_truncated = 0;
            const float* out = (both && pass == 1) ? dril_rollout_both<TC>(g, P, D, Env::A, p0, p1)
                                                   : dril_rollout_net<TC>(g, P, D, pass == 1 ? Env::A : 1, pass == 1 ? g.actor_off : g.critic_off, p0, p1);
            if (pass == 0) {
                if (t == g.T) { if (mine) g.last_values[e] = out[tid]; return; }
                if (tid < TC) values[tid] = out[tid];
            } else if (pass == 1) {
                if (mine) {
                    dril_rollout_head_one<Env>(g, t, e, out + tid, TC, both ? out[Env::A * TC + tid] : values[tid]);  // get_action_and_values, :41
                    trunc = dril_rollout_transition_one<Env, scaled>(g, t, e);        // to_env + act! + observe, :43-45
                    if (trunc) *any_truncated = 1;
                }
            } else if (mine) g.boot[row + e] = trunc ? out[tid] : 0.f;
            __syncthreads();
        }
    }
}
template <class Env, bool scaled> __device__ DRIL_ENV_ROLLOUT_INLINE void dril_env_rollout_run(const DrilEnvRolloutArgs& g) {
    constexpr int TC = DRIL_ENV_ROLLOUT_TILE;
    __shared__ float4 panels[2 * DRIL_ENV_ROLLOUT_MAX_WIDTH * TC / 4];
    __shared__ float4 staged[DRIL_ENV_ROLLOUT_STAGE_FLOATS / 4 + 1];
    __shared__ float values[TC];
    __shared__ int any_truncated;
    float* p0 = (float*)panels; float* p1 = p0 + DRIL_ENV_ROLLOUT_MAX_WIDTH * TC;
    if (g.n_params <= DRIL_ENV_ROLLOUT_STAGE_FLOATS) {                                // small nets: the parameters are read T times, so they are staged into LDS once
        float* w = (float*)staged;
        for (int i = threadIdx.x; i < g.n_params; i += DRIL_ENV_ROLLOUT_THREADS) w[i] = g.params[i];
        dril_env_rollout_steps<Env, scaled>(g, w, p0, p1, values, &any_truncated);    // (the first barrier inside comes before the first read)
    } else dril_env_rollout_steps<Env, scaled>(g, g.params, p0, p1, values, &any_truncated);
}
#define DRIL_ENV_ROLLOUT_ENTRY(name) __global__ void __launch_bounds__(DRIL_ENV_ROLLOUT_THREADS) dril_env_plugin_##name(DrilEnvRolloutArgs g)
#define DRIL_ENV_ROLLOUT_IMPL dril_env_rollout_run
#define DRIL_ENV_ROLLOUT_RUN(Env, scaled) DrilEnvRolloutBody<Env, scaled>::run(g)
#define DRIL_ENV_ROLLOUT_DESC_QUAL __device__
#endif

// the body of an entry point; for a world it is empty, so that DrilEnvRolloutCheck's static_assert is the one error of such a compile
template <class Env, bool scaled, bool world = DrilEnvIsWorld<Env>::value> struct DrilEnvRolloutBody { DRIL_ENV_FN static void run(const DrilEnvRolloutArgs& g) { DRIL_ENV_ROLLOUT_IMPL<Env, scaled>(g); } };
template <class Env, bool scaled> struct DrilEnvRolloutBody<Env, scaled, true> { DRIL_ENV_FN static void run(const DrilEnvRolloutArgs&) {} };

// the optional _scaled entry point: declared here, DEFINED as a friend of the specialisation that fits the env (the mechanism of DrilEnvPluginScaledEntries)
#if defined(DRIL_ENV_PLUGIN_HOST)
typedef void (*DrilEnvRolloutEntry)(const DrilEnvRolloutArgs*);
#else
typedef void (*DrilEnvRolloutEntry)(DrilEnvRolloutArgs);
#endif
extern "C" { DRIL_ENV_ROLLOUT_ENTRY(rollout_scaled); }
template <class Env, bool scalable> struct DrilEnvRolloutScaledEntry {};
template <class Env> struct DrilEnvRolloutScaledEntry<Env, true> {
    friend DRIL_ENV_ROLLOUT_ENTRY(rollout_scaled) { DRIL_ENV_ROLLOUT_RUN(Env, true); }
#if defined(DRIL_ENV_PLUGIN_HOST)
    static constexpr DrilEnvRolloutEntry rollout_scaled = &dril_env_plugin_host_rollout_scaled;
#else
    static constexpr DrilEnvRolloutEntry rollout_scaled = &dril_env_plugin_rollout_scaled;
#endif
};

#define DRIL_ENV_PLUGIN_ROLLOUT(Env)                                                                                     \
    static_assert(DrilEnvRolloutCheck<Env>::ok, "");                                                                     \
    extern "C" {                                                                                                         \
    DRIL_ENV_ROLLOUT_DESC_QUAL extern const DrilEnvRolloutDesc dril_env_plugin_rollout_desc = dril_env_rollout_make_desc<Env>(); \
    DRIL_ENV_ROLLOUT_ENTRY(rollout) { DRIL_ENV_ROLLOUT_RUN(Env, false); }                                                \
    }                                                                                                                    \
    template struct DrilEnvRolloutScaledEntry<Env, dril_env_plugin_scalable<Env>()>;
