// dril_sac_device.h — what the kernels of more than one unit of the SAC host code share (the units: dril_sac_handle.h): __device__ inline functions and the argument
// structs they take, no __global__ definition.  The SquashedDiagGaussian sample, the handle's Philox streams, the phase stamp, the grid constants of the gradient
// step that creation sizes buffers by, and the four pieces of a collected env step — head, push, the built-in Box envs' own thread, the evaluation's episode
// accounting — that the collection (dril_sac_collect.hip), the device-array verbs (dril_sac_ext.hip) and the evaluation (dril_sac_eval.hip) assemble into their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dril_internal.h"      // philox4x32_10 / randn_f32, EnvSpec / EnvCursor / env_advance / env_obs, MonitorArgs, wall_clock64
#include "dril_sac_adapter.h"   // sac_rand_box, sac_to_env
#include "dril_sac_eval.h"      // SacEvalEvent

namespace dril::sac {

// =================================================================================================================
// SquashedDiagGaussian (squashedDiagGaussian.jl:24-46) — per-sample scalar math, accurate libm
// =================================================================================================================
constexpr int kMaxA = 16;
constexpr float kLog2Pi = 1.8378770664093453f;
__device__ inline float softplus_f(float x) { return log1pf(expf(-fabsf(x))) + (x > 0.f ? x : 0.f); }   // Lux.softplus
// a = tanh(mu + exp(ls) * noise); returns logpdf(d, a) (:36-46), g = atanh(clamp(a))
__device__ inline float squashed_sample_logp(const float* mu, const float* ls, const float* noise, int A, float* a, float* g) {
    const float eps = 1.0e-6f, lo = -1.0f + eps, hi = 1.0f - eps;
    float lss = 0.f, dss = 0.f, corr = 0.f;
    for (int i = 0; i < A; ++i) {
        a[i] = tanhf(mu[i] + expf(ls[i]) * noise[i]);
        const float xc = a[i] < lo ? lo : (a[i] > hi ? hi : a[i]);
        g[i] = atanhf(xc);
        corr += 2.0f * (logf(2.0f) - g[i] - softplus_f(-2.0f * g[i]));
        lss += ls[i]; const float d = g[i] - mu[i]; dss += d * d * expf(-2.0f * ls[i]);
    }
    return -0.5f * (2.0f * lss + dss + (float)A * kLog2Pi) - corr;       // diagGaussian.jl:25-36 minus the correction
}

struct SacRng { uint64_t key; uint64_t u; };
__device__ inline float sac_noise(SacRng r, int stream, int i, int a) {
    uint32_t o[4];
    philox4x32_10((uint32_t)r.key, (uint32_t)(r.key >> 32), (uint32_t)r.u, (uint32_t)(r.u >> 32), (uint32_t)stream, (uint32_t)(i * 4 + a / 2), o);
    return (a & 1) ? randn_f32(o[2], o[3]) : randn_f32(o[0], o[1]);
}

// In-stream time stamps of dril_sac_iterate: the fps of every iteration's collection (off_policy_collection.jl:126-128) and the update / collection split of the
// profile need the time at the phase boundaries.  A HIP event per boundary costs the stream ~5 us each (three per iteration: 16 us of a 205 us iteration, seen as
// gaps in the rocprofv3 trace); instead the LAST kernel of a phase stores the constant-rate wall clock (s_memrealtime) when its highest-numbered workgroup is done —
// one store, no atomics, nothing waits.  Kernels of one stream run back to back, so a phase lasts from the previous phase's stamp to its own.
__device__ __forceinline__ void phase_stamp(unsigned long long* stamp) {
    if (stamp && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *stamp = wall_clock64();
}

// ---- grid shapes of the gradient step's kernels (dril_sac_update.hip) that dril_sac_create sizes the handle's buffers by --------------------------------
#ifndef DRIL_SAC_ADAM_BLOCKS
#define DRIL_SAC_ADAM_BLOCKS 1024
#endif
constexpr int kSacAdamBlocks = DRIL_SAC_ADAM_BLOCKS;   // grid cap of the two elementwise optimiser kernels (-DDRIL_SAC_ADAM_BLOCKS=<n>: a tuning switch; 256 -> 1 024 was measured)
constexpr int kHeadSamplesPerBlock = 1;   // fused head kernels: one workgroup per sample — the dot products of a sample run on separate waves, so a head is ~3 dependent memory round trips
constexpr int kOptL1MaxIn = 4, kOptL1Units = 16, kOptL1Groups = 16, kOptL1MaxB = 1024;      // first_layer_opt_block: a block owns kOptL1Units hidden units (2 B in floats of dynamic LDS: 32 KB at the cap)

// ---- collection (off_policy_collection.jl:28-96) ---------------------------------------------------------------------------
struct CollectHeadArgs {
    int E, A, use_random; float* mu; const float* log_std; const float* inj_noise; const uint32_t* gstep; uint64_t seed0;
    const float* low; const float* high;                              // Box bounds per action dimension, device table [A] each (built-in and external envs: their one pair in every entry)
    float* raw; float* envact;
    const float* h2; const float* w3; const float* b3; int H2;     // h2 != null: the actor's output layer mu = W3 h2 + b3 is evaluated HERE (sac_mu_rows) instead of in a launch of its own
    int deterministic;                                             // evaluation only (a collection leaves it 0): mode(d) = tanh(mean), squashedDiagGaussian.jl:48-50 — the sample with zero noise
};
// mu[e][a] = W3[a, :] . h2[e, :] + b3[a] for the kEnvsPerBlock envs of a 256-thread block (4096 envs = 256 blocks: every CU takes part in what is a latency-bound
// pass): each of the four waves takes kMuRows envs, the wave across the features — per 256-feature slice all rows' loads (one coalesced 1 KB line run each) are in
// flight together, then one butterfly sum per row (every lane ends with the total; fixed order => deterministic).  Result in mu_s[] (shared), valid after the
// caller's barrier.  Every thread of the block takes part whatever E is.
constexpr int kEnvsPerBlock = 16, kMuRows = kEnvsPerBlock / 4;
__device__ __forceinline__ void sac_mu_block(const CollectHeadArgs& g, int a, int e_block0, float* mu_s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, e0 = e_block0 + kMuRows * wave;
    const float* __restrict__ w = g.w3 + a;                          // W3 column-major (A x H2): W3[a + k A]
    float acc[kMuRows];
#pragma unroll
    for (int r = 0; r < kMuRows; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < g.H2; k0 += 256) {                         // H2 % 4 == 0 (host-checked): a lane's four features are inside the row or all outside
        const int k = k0 + 4 * lane;
        const bool in = k < g.H2;
        const int kk = in ? k : 0;                                    // out-of-range lanes re-read the row's start and multiply by zero weights: no branch around the loads
        float wk[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { const float x = w[(size_t)(kk + t) * g.A]; wk[t] = in ? x : 0.f; }
        float4 v[kMuRows];
#pragma unroll
        for (int r = 0; r < kMuRows; ++r) {
            const int e = e0 + r < g.E ? e0 + r : g.E - 1;           // rows past E re-read the last one (in bounds, unused)
            v[r] = *reinterpret_cast<const float4*>(g.h2 + (size_t)e * g.H2 + kk);
        }
#pragma unroll
        for (int r = 0; r < kMuRows; ++r) { acc[r] = fmaf(v[r].x, wk[0], acc[r]); acc[r] = fmaf(v[r].y, wk[1], acc[r]); acc[r] = fmaf(v[r].z, wk[2], acc[r]); acc[r] = fmaf(v[r].w, wk[3], acc[r]); }
    }
    const float b = g.b3[a];
#pragma unroll
    for (int r = 0; r < kMuRows; ++r) {
        float s2 = acc[r];
#pragma unroll
        for (int o = 32; o; o >>= 1) s2 += __shfl_xor(s2, o);
        if (lane == r) mu_s[kMuRows * wave + r] = s2 + b;
    }
}
// action component a of env e in the collection step: the noise (injected, or the env's stream at its global step: dril_device.h) -> the raw action the replay stores ->
// the action the env receives (*envact); the caller stores them
__device__ __forceinline__ void sac_collect_action(const CollectHeadArgs& g, int e, uint32_t gstep, int a, float mu, float* raw, float* envact) {
    float z, r, ev;
    if (g.deterministic) z = 0.f;                                                                // mode(d): the same expression as sac_squash_eval_kernel's deterministic branch
    else if (g.inj_noise) z = g.inj_noise[e * g.A + a];
    else z = g.use_random ? env_noise_u01_f32(g.seed0 + (uint64_t)e, gstep, a) : env_noise_randn(g.seed0 + (uint64_t)e, gstep, a);
    const float lo = g.low[a], hi = g.high[a];
    if (g.use_random) { r = sac_rand_box(z, lo, hi); ev = r; }                                   // rand(rng, act_space) per dimension: already env space, :50-53
    else {
        r = tanhf(mu + expf(g.log_std[a]) * z);                                                  // rand(SquashedDiagGaussian) squashedDiagGaussian.jl:24-27
        ev = sac_to_env(r, lo, hi);                                                              // to_env(TanhScaleAdapter) default_adapters.jl:13-21
    }
    *raw = r; *envact = ev;
}
// the head of the kEnvsPerBlock envs of a 256-thread block: the output layer by all four waves (g.h2 set), then one thread per env
__device__ __forceinline__ void sac_head_block(const CollectHeadArgs& g, float* mu_s) {
    const int e = blockIdx.x * kEnvsPerBlock + threadIdx.x;
    if (g.h2 && !g.use_random) {                                     // the output layer first (whole block: no early return before it)
        for (int a = 0; a < g.A; ++a) {
            sac_mu_block(g, a, blockIdx.x * kEnvsPerBlock, mu_s);
            __syncthreads();
            if (threadIdx.x < kEnvsPerBlock && e < g.E) g.mu[(size_t)e * g.A + a] = mu_s[threadIdx.x];
            __syncthreads();
        }
    }
    if (threadIdx.x >= kEnvsPerBlock || e >= g.E) return;
    const uint32_t gs = g.gstep[e];
    for (int a = 0; a < g.A; ++a) {
        float r, ev;
        sac_collect_action(g, e, gs, a, g.use_random ? 0.f : g.mu[(size_t)e * g.A + a], &r, &ev);
        g.raw[e * g.A + a] = r; g.envact[e * g.A + a] = ev;
    }
}
struct PushArgs {
    int E, D, A; long long cap, tail; const float *obs, *raw, *rew, *tobs, *nobs; const uint8_t *term, *trunc;
    float *rb_obs, *rb_next, *rb_act, *rb_rew; uint8_t *rb_term, *rb_trunc;
    unsigned long long* stamp;   // phase_stamp (null: none)
};
// push! of env e's transition into its ring slot: D / A the row widths, tobs / nobs / raw the env's rows (memory or registers)
__device__ __forceinline__ void sac_push_row(const PushArgs& g, int e, int D, int A, const float* tobs, const float* nobs, const float* raw, float rew, bool term, bool trunc) {
    const long long slot = (g.tail + e) % g.cap;
    for (int d = 0; d < D; ++d) {
        g.rb_obs[slot * D + d] = g.obs[(size_t)e * D + d];
        g.rb_next[slot * D + d] = trunc ? tobs[d] : nobs[d];                                    // truncated_observation | next observation
    }
    for (int a = 0; a < A; ++a) g.rb_act[slot * A + a] = raw[a];                                // unprocessed action, :72
    g.rb_rew[slot] = rew; g.rb_term[slot] = term; g.rb_trunc[slot] = trunc;
}
// push! of the n envs [e0, e0 + n) by a whole workgroup, memory to memory: the threads walk the flat (env, dim) index of each field, so a wave's stores into rb_obs /
// rb_next / rb_act are one contiguous run for any D / A (consecutive envs take consecutive ring slots; the run breaks once, where the ring wraps) instead of one lane
// per env with a D-float stride.  Same rows, same slots as sac_push_row.
__device__ __forceinline__ void sac_push_block(const PushArgs& g, int e0, int n) {
    const int D = g.D, A = g.A;
    for (int i = threadIdx.x; i < n * D; i += blockDim.x) {
        const int e = e0 + i / D, d = i % D;
        const long long slot = (g.tail + e) % g.cap;
        g.rb_obs[slot * D + d] = g.obs[(size_t)e * D + d];
        g.rb_next[slot * D + d] = g.trunc[e] ? g.tobs[(size_t)e * D + d] : g.nobs[(size_t)e * D + d];   // truncated_observation | next observation
    }
    for (int i = threadIdx.x; i < n * A; i += blockDim.x) {
        const int e = e0 + i / A, a = i % A;
        g.rb_act[((g.tail + e) % g.cap) * A + a] = g.raw[(size_t)e * A + a];                        // unprocessed action, :72
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int e = e0 + i;
        const long long slot = (g.tail + e) % g.cap;
        g.rb_rew[slot] = g.rew[e]; g.rb_term[slot] = g.term[e] != 0; g.rb_trunc[slot] = g.trunc[e] != 0;
    }
}
constexpr int kPushEnvsPerBlock = 64;
// the argument block of the kernels that take one env step of a built-in Box env per thread (sac_collect_env_kernel and its twins)
struct CollectEnvArgs { CollectHeadArgs head; PushArgs push; uint64_t seed0; int episode_len; float* state; int32_t* step_count; uint32_t* episode; uint32_t* gstep;
                        float* rew; uint8_t* term; uint8_t* trunc; float* tobs; float* nobs;
                        MonitorArgs mon; };   // MonitorWrapperEnv (dril_sac_monitor_enable): running sums, and row t of the collection's finished-episode block; all null = off
// the actor's output layer for the kEnvsPerBlock envs of the block (A = 1), then this thread's env: false = the thread owns no env
__device__ __forceinline__ bool sac_env_thread_mu(const CollectHeadArgs& g, float* mu_s, int* e_out, float* mu_out) {
    const int e = blockIdx.x * kEnvsPerBlock + threadIdx.x;          // 256 threads per kEnvsPerBlock envs: all four waves on the output layer, then one thread per env
    if (!g.use_random && g.h2) { sac_mu_block(g, 0, blockIdx.x * kEnvsPerBlock, mu_s); __syncthreads(); }   // same device function as the head kernel
    if (threadIdx.x >= kEnvsPerBlock || e >= g.E) return false;
    float mu_e = 0.f;
    if (!g.use_random) { if (g.h2) { mu_e = mu_s[threadIdx.x]; g.mu[e] = mu_e; } else mu_e = g.mu[e]; }
    *e_out = e; *mu_out = mu_e;
    return true;
}
// predict_actions -> act! with auto-reset -> observe of env e by its thread: what the collection and the evaluation of a built-in Box env share.  *raw the action the
// replay stores, to / no the terminal and the next observation (also written to c.tobs where truncated / c.nobs)
template <int KIND>
__device__ __forceinline__ StepOut sac_env_thread_step(const CollectEnvArgs& c, int e, float mu_e, float* raw, float* to, float* no) {
    constexpr int D = EnvSpec<KIND>::D;
    const CollectHeadArgs& g = c.head;
    const EnvArrays env{c.state, c.step_count, c.episode, c.gstep, c.mon.cur_ret, c.mon.cur_len};
    EnvCursor<KIND> cur; cur.load(env, e);
    // ---- the action (sac_collect_head_kernel, A = 1) ----
    float r, ev;
    sac_collect_action(g, e, cur.gs, 0, mu_e, &r, &ev);
    g.raw[e] = r; g.envact[e] = ev; *raw = r;
    // ---- act! with auto-reset (env_step_kernel) ----
    const StepOut so = env_advance<KIND>(cur, ev, 0, c.episode_len, false);
    c.rew[e] = so.rew; c.term[e] = so.term; c.trunc[e] = so.trunc;
    if (c.mon.cur_ret) c.mon.flags_out[e] = so.flags();
    env_obs<KIND>(cur.st, to);                                                          // terminal_observation (stored where truncated)
    if (so.trunc) {
#pragma unroll
        for (int i = 0; i < D; ++i) c.tobs[(size_t)e * D + i] = to[i];
    }
    env_end_episode<KIND>(cur, c.seed0 + (uint64_t)e, so, c.mon.cur_ret ? c.mon.ep_ret + e : nullptr, c.mon.ep_len + e);
    cur.store(env, e);
    // ---- observe (env_observe_kernel) ----
    env_obs<KIND>(cur.st, no);
#pragma unroll
    for (int i = 0; i < D; ++i) c.nobs[(size_t)e * D + i] = no[i];
    return so;
}

// ---- evaluate_agent on the device (evaluation.jl:90-124; the event list: dril_sac_eval.h) ----------------------------------------------------------
// The episode accounting of env e after its step, by the env's own thread: current_rewards[e] += reward in float32 and in step order, as the reference's host loop
// adds them; where the episode ended, one event through the list's counter (slots past the capacity are only counted) and the two sums restart.
struct EvalAcctArgs { int E; int32_t step; float* cur_ret; int32_t* cur_len; unsigned int* counter; SacEvalEvent* events; unsigned int cap; };
__device__ __forceinline__ void sac_eval_account(const EvalAcctArgs& a, int e, float rew, bool done) {
    float r = a.cur_ret[e] + rew; int32_t l = a.cur_len[e] + 1;
    if (done) {
        const unsigned int i = atomicAdd(a.counter, 1u);
        if (i < a.cap) a.events[i] = SacEvalEvent{a.step, e, r, l};
        r = 0.f; l = 0;
    }
    a.cur_ret[e] = r; a.cur_len[e] = l;
}

}  // namespace dril::sac
