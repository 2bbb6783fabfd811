// dril_sac_collect.hip — the collection of the SAC handle (collect_trajectories, off_policy_collection.jl:28-96): the head, push and env-step kernels, one collected
// step for a built-in Box env, for a device env plug-in and under NormalizeWrapperEnv, a whole collection, and the verbs dril_sac_debug_set_collect_noise,
// dril_sac_collect_rollout and dril_sac_collect_continue.  The actor's hidden layers of a step are dril_sac_net.hip (actor_hidden), the two wrappers dril_sac_wrap.hip.
// The units: dril_sac_handle.h.
#include <hip/hip_runtime.h>

#include <chrono>
#include <algorithm>
#include <string>

#include "dril_sac_handle.h"

using namespace dril;
using namespace dril::sac;

namespace {

// ---- collection (off_policy_collection.jl:28-96): the head, push and env-step kernels; their pieces are dril_sac_device.h ------------------------------------
__global__ __launch_bounds__(256) void sac_collect_head_kernel(CollectHeadArgs g) {
    __shared__ float mu_s[kEnvsPerBlock];
    sac_head_block(g, mu_s);
}
__global__ void sac_push_kernel(PushArgs g) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    phase_stamp(g.stamp);                                    // (within a microsecond of the kernel's end: the stamp feeds a per-iteration fps statistic)
    if (e >= g.E) return;
    sac_push_row(g, e, g.D, g.A, g.tobs + (size_t)e * g.D, g.nobs + (size_t)e * g.D, g.raw + e * g.A, g.rew[e], g.term[e] != 0, g.trunc[e] != 0);
}
__global__ __launch_bounds__(256) void sac_push_flat_kernel(PushArgs g) {
    const int e0 = blockIdx.x * kPushEnvsPerBlock;
    phase_stamp(g.stamp);
    sac_push_block(g, e0, min(kPushEnvsPerBlock, g.E - e0));                                        // grid = ceil(E / kPushEnvsPerBlock): n >= 1
}
// Collection over a device env plug-in, whose step kernel already returns the next observation: per env step {head, plug-in step, push}.  This kernel is the push of
// the PREVIOUS step and the head of THIS step of the same kEnvsPerBlock envs in one launch (p.E == 0: nothing to push yet), so n steps are n x {this, plug-in step}
// and one trailing sac_push_flat_kernel.  The push reads the previous step's e_raw rows before the head overwrites them (the barrier); everything else the two halves
// touch is disjoint, and a block reads and writes rows of its own envs only.
struct HeadPushArgs { CollectHeadArgs head; PushArgs push; };
__global__ __launch_bounds__(256) void sac_collect_head_push_kernel(HeadPushArgs c) {
    __shared__ float mu_s[kEnvsPerBlock];
    const int e0 = blockIdx.x * kEnvsPerBlock;
    if (c.push.E > 0) { sac_push_block(c.push, e0, min(kEnvsPerBlock, c.push.E - e0)); __syncthreads(); }   // (grid = ceil(E / kEnvsPerBlock), push.E == head.E: n >= 1)
    sac_head_block(c.head, mu_s);
}
// One env step of the collection for a DEVICE env in ONE launch: sac_collect_head_kernel -> env_step_kernel -> env_observe_kernel -> sac_push_kernel are all one thread per env
// on data of that env only (four dependent launches of 4 - 5 us and their boundaries per collected step).  The same four definitions in the same order — sac_collect_action,
// the EnvCursor transition (env_advance / env_end_episode, dril_device.h), env_obs, sac_push_row — and every intermediate buffer (e_raw, e_envact, e_rew, e_term, e_trunc,
// e_tobs, obs_nxt) still written: bit-identical to the four-launch sequence (A = 1: every device Box env).
template <int KIND>
__global__ __launch_bounds__(256) void sac_collect_env_kernel(CollectEnvArgs c) {
    constexpr int D = EnvSpec<KIND>::D;
    __shared__ float mu_s[kEnvsPerBlock];
    int e; float mu_e;
    if (!sac_env_thread_mu(c.head, mu_s, &e, &mu_e)) return;
    float r, to[D], no[D];
    const StepOut so = sac_env_thread_step<KIND>(c, e, mu_e, &r, to, no);
    // ---- push! (sac_push_kernel) ----
    sac_push_row(c.push, e, D, 1, to, no, &r, so.rew, so.term, so.trunc);
    phase_stamp(c.push.stamp);                                               // thread 0 of the last workgroup owns a live env (grid = ceil(E / kEnvsPerBlock)): the end of its work ~ the end of the phase
}

// ---- the twins of sac_collect_env_kernel that an evaluation and a trajectory recording enqueue (launch_eval_env / launch_traj_env below; the host code: -----------
// dril_sac_eval.hip).  They stand in this unit because all four kernels over sac_env_thread_step must be compiled together: how the compiler inlines the env's noise
// draw (Philox under env_noise_*) into one of them depends on which others of the unit call it, and apart these two come out ~450 code bytes longer, with Philox
// rounds computed twice (profiles/sac_units_resources.md)
// built-in Box envs: the twin of sac_collect_env_kernel with the accounting where that one has the push (the monitor pointers of `env` are null: an evaluation does
// not feed the training env's MonitorWrapperEnv).  nz.st != null: NormalizeWrapperEnv with training = false — the next observation normalised with the frozen
// statistics by the env's own thread, in place of the raw row
template <int KIND>
__global__ __launch_bounds__(256) void sac_eval_env_kernel(EvalEnvArgs c) {
    constexpr int D = EnvSpec<KIND>::D;
    __shared__ float mu_s[kEnvsPerBlock];
    int e; float mu_e;
    if (!sac_env_thread_mu(c.env.head, mu_s, &e, &mu_e)) return;
    float r, to[D], no[D];
    const StepOut so = sac_env_thread_step<KIND>(c.env, e, mu_e, &r, to, no);
    if (c.nz.st && c.nz.norm_obs) {
#pragma unroll
        for (int i = 0; i < D; ++i) c.env.nobs[(size_t)e * D + i] = nz_obs(no[i], c.nz.st[i], c.nz.st[D + i], c.nz.eps, c.nz.clip);
    }
    sac_eval_account(c.acct, e, so.rew, so.done());
}
// ---- collect_trajectory on the device (trajectory_utils.jl:3-49; dril_traj_record.h) -----------------------------------------------------------------
// built-in Box envs: the twin of sac_eval_env_kernel with the recording of envs 0..M-1 where that kernel has the accounting.  After the step the env's thread holds
// a whole row in registers: `to` is env_obs of the cursor after env_advance and before env_end_episode — the terminal state where the episode ended, and where it did
// not, env_end_episode returns at once and `no` is the same expression over the same state, the same floats — so `to` is the row's observation throughout; the env
// action is the word sac_env_thread_step stored for this env; reward and flags are the step's own.  One step per launch: the open / closed state of trajectory e is
// rec.length[e], loaded before the step.  Threads of envs >= M and of closed trajectories step like an evaluation and write nothing to the recording.
template <int KIND>
__global__ __launch_bounds__(256) void sac_traj_env_kernel(TrajEnvArgs c) {
    constexpr int D = EnvSpec<KIND>::D;
    __shared__ float mu_s[kEnvsPerBlock];
    int e; float mu_e;
    if (!sac_env_thread_mu(c.env.head, mu_s, &e, &mu_e)) return;
    const bool recorded = e < c.rec.M;
    int32_t length = recorded ? c.rec.length[e] : 0;
    float r, to[D], no[D];
    const StepOut so = sac_env_thread_step<KIND>(c.env, e, mu_e, &r, to, no);
    if (c.nz.st && c.nz.norm_obs) {
#pragma unroll
        for (int i = 0; i < D; ++i) c.env.nobs[(size_t)e * D + i] = nz_obs(no[i], c.nz.st[i], c.nz.st[D + i], c.nz.eps, c.nz.clip);
    }
    if (recorded) {
        const uint32_t act[1] = {traj_f2u(c.env.head.envact[e])};                       // (written by this thread in sac_env_thread_step)
        traj_record_env<D, 1>(c.rec, c.maps, c.t, e, act, so.rew, so.term, so.trunc, to, length);
    }
}

// ---- NormalizeWrapperEnv in a collection (argument blocks and the table shape: dril_sac_norm.h) -----------------------------------------------------------------
// ---- moments, built-in Box envs (A = 1) -----------------------------------------------------------------------------------------------------------------
// The twin of sac_collect_env_kernel without the push: the 16 env threads of a block sit in lanes 0 - 15 of wave 0, so the block's 2 D + 2 sums are four xor
// steps each and one row of the table per block (rows = ceil(E / kEnvsPerBlock)).  env.nobs points at the wrapper's old_obs: the raw next observation.
template <int KIND>
__global__ __launch_bounds__(256) void sac_norm_env_kernel(NormEnvArgs c) {
    constexpr int D = EnvSpec<KIND>::D, C = 2 * D + 2;
    __shared__ float mu_s[kEnvsPerBlock];
    int e = 0; float mu_e = 0.f;
    const bool own = sac_env_thread_mu(c.env.head, mu_s, &e, &mu_e);
    if (threadIdx.x >= 64) return;                                                       // (no barrier below: the other three waves only served the output layer)
    double acc[C];
#pragma unroll
    for (int i = 0; i < C; ++i) acc[i] = 0;
    if (own) {
        float r, to[D], no[D];
        const StepOut so = sac_env_thread_step<KIND>(c.env, e, mu_e, &r, to, no);
        if (c.upd_ret) {                                                                 // update_reward_stats! :167-171 (done envs go back to zero in the apply kernel)
            const float ret = c.returns[e] * c.gamma + so.rew;
            c.returns[e] = ret; acc[2 * D] = ret; acc[2 * D + 1] = (double)ret * ret;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) { acc[d] = no[d]; acc[D + d] = (double)no[d] * no[d]; }
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
        double v = acc[i];
#pragma unroll
        for (int o = kEnvsPerBlock / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (threadIdx.x == 0) c.partials[(size_t)blockIdx.x * C + i] = v;
    }
}

// the two grids of this unit: a 256-thread block per kEnvsPerBlock envs (the head kernels and the four env-kernel families), and per kPushEnvsPerBlock envs (the flat push)
dim3 env_grid(const dril_sac_handle* h) { return dim3((h->cfg.n_envs + kEnvsPerBlock - 1) / kEnvsPerBlock); }
dim3 push_flat_grid(const dril_sac_handle* h) { return dim3((h->cfg.n_envs + kPushEnvsPerBlock - 1) / kPushEnvsPerBlock); }

PushArgs push_args(dril_sac_handle* h, const float* obs, const float* nobs, unsigned long long* stamp) {
    const long long tail = (h->head + h->size) % h->cap;
    return PushArgs{h->cfg.n_envs, h->D, h->A, h->cap, tail, obs, h->e_raw, h->e_rew, h->e_tobs, nobs, h->e_term, h->e_trunc,
                    h->rb_obs, h->rb_next, h->rb_act, h->rb_rew, h->rb_term, h->rb_trunc, stamp};
}
// head -> act! + observe -> push! of one collection step over a device env plug-in (the actor's hidden layers are already enqueued).  `first` / `last`: the step's
// place in its collection — the fused form pushes step t's rows in the launch that computes the head of step t + 1, the last step's rows in a launch of their own,
// so the ring is complete when the collection returns.
int collect_step_module(dril_sac_handle* h, const CollectHeadArgs& ca, unsigned long long* stamp, bool first, bool last) {
    // the step's actions are the env-space actions of TanhScaleAdapter / rand(action_space), inside the Box by construction: the wrapper's ClampAdapter is a no-op on them
    const EnvStepOut out{h->e_rew, h->e_term, h->e_trunc, h->e_tobs, h->obs_nxt};
    const MonitorArgs mon = monitor_row(h); if (h->mon_window) h->mon_row += 1;                       // MonitorWrapperEnv: the wrapper of dril_env_plugin.h keeps the sums and writes this step's row
    if (!h->fused_head_push) {                                                                       // DRIL_SAC_NO_FUSED_HEAD_PUSH=1: three launches per step
        launch_collect_head(h, ca);
        SHIP(h, h->env.step(h->e_envact, out, mon, h->stream));
        hipLaunchKernelGGL(sac_push_flat_kernel, push_flat_grid(h), dim3(256), 0, h->stream, push_args(h, h->obs_cur, h->obs_nxt, stamp));
        SHIP(h, hipGetLastError());
        ring_advance(h); std::swap(h->obs_cur, h->obs_nxt);
        return DRIL_OK;
    }
    // after the previous step's swap obs_nxt holds that step's observation and obs_cur its next observation: the rows of the pending push
    HeadPushArgs hp{ca, push_args(h, h->obs_nxt, h->obs_cur, nullptr)};
    if (first) hp.push.E = 0; else ring_advance(h);
    hipLaunchKernelGGL(sac_collect_head_push_kernel, env_grid(h), dim3(256), 0, h->stream, hp);
    SHIP(h, h->env.step(h->e_envact, out, mon, h->stream));                                          // (overwrites obs_nxt: its old rows went into the ring one launch earlier)
    std::swap(h->obs_cur, h->obs_nxt);
    if (last) {
        hipLaunchKernelGGL(sac_push_flat_kernel, push_flat_grid(h), dim3(256), 0, h->stream, push_args(h, h->obs_nxt, h->obs_cur, stamp));
        ring_advance(h);
    }
    SHIP(h, hipGetLastError());
    return DRIL_OK;
}
// one collected step through the wrapper: {head, act!, raw observe, moments} then {merge, normalise, push}
int collect_step_norm(dril_sac_handle* h, const CollectHeadArgs& ca, unsigned long long* stamp) {
    const bool upd_obs = h->nz.cfg.training && h->nz.cfg.norm_obs, upd_ret = h->nz.cfg.training && h->nz.cfg.norm_reward;
    int rows = 0;
    const MonitorArgs mon = monitor_row(h); if (h->mon_window) h->mon_row += 1;                     // MonitorWrapperEnv sits inside the normaliser: raw rewards
    if (h->env.module) {
        launch_collect_head(h, ca);
        SHIP(h, h->env.step(h->e_envact, EnvStepOut{h->e_rew, h->e_term, h->e_trunc, h->e_tobs, h->nz_old_obs}, mon, h->stream));
        if (upd_obs || upd_ret) SDO(nz_moments(h, upd_obs, upd_ret, &rows));
    } else {                                                                                         // every built-in Box env has A = 1
        CollectEnvArgs ce = env_kernel_args(h, ca, PushArgs{}, mon); ce.nobs = h->nz_old_obs;
        const NormEnvArgs ne{ce, h->nz_returns, upd_ret ? 1 : 0, h->nz.cfg.gamma, h->nz.partials};
        const dim3 grid = env_grid(h), block(256);
        rows = (int)grid.x;
        SHIP(h, with_env_kind<KindShare::None>(BoxKinds{}, h->env.kind, [&](auto K) { hipLaunchKernelGGL(sac_norm_env_kernel<decltype(K)::value>, grid, block, 0, h->stream, ne); return hipGetLastError(); }));
    }
    NzApplyArgs a{}; a.w.raw = h->nz_old_obs; a.w.obs_out = h->obs_nxt;
    a.w.rew = h->e_rew; a.old_rew = h->nz_old_rew; a.w.returns = h->nz_returns; a.w.term = h->e_term; a.w.trunc = h->e_trunc; a.tobs = h->e_tobs;
    a.push = push_args(h, h->obs_cur, nullptr, stamp);
    SDO(nz_apply(h, a, rows, upd_obs, upd_ret));
    ring_advance(h); std::swap(h->obs_cur, h->obs_nxt);
    return DRIL_OK;
}

}  // namespace

namespace dril::sac {
int ensure_obs(dril_sac_handle* h) {
    if (!h->env.ready) return sfail(h, DRIL_ERR_NOT_INITIALISED, "dril_sac_env_reset has not been called");
    if (!h->obs_valid) {
        SHIP(h, h->env.observe(h->obs_cur, h->stream));
        h->obs_valid = true;
    }
    return DRIL_OK;
}
void ring_advance(dril_sac_handle* h) {                                                            // CircularBuffer: n_envs rows in, overwrite the oldest
    const long long over = h->size + h->cfg.n_envs - h->cap;
    if (over > 0) { h->head = (h->head + over) % h->cap; h->size = h->cap; } else h->size += h->cfg.n_envs;
}
// the env kernel's argument block of a built-in Box env (A = 1): head, push (collection only), the env arrays and the per-step results
CollectEnvArgs env_kernel_args(dril_sac_handle* h, const CollectHeadArgs& ca, const PushArgs& pa, const MonitorArgs& mon) {
    return CollectEnvArgs{ca, pa, h->env.seed0, h->env.episode_len, h->env.state, h->env.step_count, h->env.episode, h->env.gstep, h->e_rew, h->e_term, h->e_trunc, h->e_tobs, h->obs_nxt, mon};
}
// the launches another unit enqueues: the action head of all envs (a plug-in's evaluation step), the ring write of one env step (dril_sac_ext_push), and for a
// built-in Box kind (A = 1) the ONE launch of an evaluation / a trajectory step over the collection's grid
void launch_collect_head(dril_sac_handle* h, const CollectHeadArgs& ca) { hipLaunchKernelGGL(sac_collect_head_kernel, env_grid(h), dim3(256), 0, h->stream, ca); }
void launch_push(dril_sac_handle* h, const PushArgs& pa) { hipLaunchKernelGGL(sac_push_kernel, dim3((pa.E + 255) / 256), dim3(256), 0, h->stream, pa); }
hipError_t launch_eval_env(dril_sac_handle* h, const EvalEnvArgs& a) {
    const dim3 grid = env_grid(h), block(256);
    return with_env_kind<KindShare::None>(BoxKinds{}, h->env.kind, [&](auto K) { hipLaunchKernelGGL(sac_eval_env_kernel<decltype(K)::value>, grid, block, 0, h->stream, a); return hipGetLastError(); });
}
hipError_t launch_traj_env(dril_sac_handle* h, const TrajEnvArgs& a) {
    const dim3 grid = env_grid(h), block(256);
    return with_env_kind<KindShare::None>(BoxKinds{}, h->env.kind, [&](auto K) { hipLaunchKernelGGL(sac_traj_env_kernel<decltype(K)::value>, grid, block, 0, h->stream, a); return hipGetLastError(); });
}
// one step of collect_trajectories (off_policy_collection.jl:42-93) for all envs
int collect_step(dril_sac_handle* h, int use_random, const float* inj_noise, unsigned long long* stamp, bool first, bool last) {
    const int A = h->A;
    CollectHeadArgs ca; SDO(actor_hidden(h, use_random, inj_noise, &ca));
    if (h->nz.on) return collect_step_norm(h, ca, stamp);
    if (h->env.module) return collect_step_module(h, ca, stamp, first, last);
    const MonitorArgs mon = monitor_row(h); if (h->mon_window) h->mon_row += 1;                                   // MonitorWrapperEnv: this step's row of the collection's block (null: off)
    if (A == 1 && !h->external && h->fused_collect) {                                                            // every device Box env: head + act! + observe + push! in one launch
        const CollectEnvArgs ce = env_kernel_args(h, ca, push_args(h, h->obs_cur, h->obs_nxt, stamp), mon);
        const dim3 grid = env_grid(h), block(256);
        SHIP(h, with_env_kind<KindShare::None>(BoxKinds{}, h->env.kind, [&](auto K) { hipLaunchKernelGGL(sac_collect_env_kernel<decltype(K)::value>, grid, block, 0, h->stream, ce); return hipGetLastError(); }));
        ring_advance(h); std::swap(h->obs_cur, h->obs_nxt);
        return DRIL_OK;
    }
    launch_collect_head(h, ca);
    SHIP(h, h->env.step(h->e_envact, EnvStepOut{h->e_rew, h->e_term, h->e_trunc, h->e_tobs, h->obs_nxt}, mon, h->stream));   // act! :60, observe :61
    launch_push(h, push_args(h, h->obs_cur, h->obs_nxt, stamp));
    SHIP(h, hipGetLastError());
    ring_advance(h); std::swap(h->obs_cur, h->obs_nxt);
    return DRIL_OK;
}
// before the steps of a collection: the observation of the envs' present state (the raw one under NormalizeWrapperEnv) and MonitorWrapperEnv's block of n_steps rows
int collect_prepare(dril_sac_handle* h, int n_steps) {
    if (h->nz.on) SDO(nz_ensure_raw(h)); else SDO(ensure_obs(h));
    return monitor_begin(h, n_steps);
}
// cont: the steps continue the collection the previous call began (dril_sac_collect_continue) — under NormalizeWrapperEnv there is no second opening observe
int collect(dril_sac_handle* h, int n_steps, int use_random, double* fps, bool cont) {
    if (n_steps <= 0) return sfail(h, DRIL_ERR_INVALID_ARG, "n_steps must be positive");
    if (h->collect_noise && h->collect_noise_count != (size_t)n_steps * h->cfg.n_envs * h->A)
        return sfail(h, DRIL_ERR_INVALID_ARG, "injected collect noise must hold n_steps * n_envs * action_dim values");
    if (h->nz.on && cont && !h->obs_valid) return sfail(h, DRIL_ERR_NOT_INITIALISED, "dril_sac_collect_continue: no collection is in progress under NormalizeWrapperEnv (env reset, statistics set or wrapper switched since the last collected step): begin one with dril_sac_collect_rollout");
    SDO(collect_prepare(h, n_steps));
    const auto t0 = std::chrono::steady_clock::now();
    if (h->cfg.profile_events) hipEventRecord(h->ev_a, h->stream);
    if (h->nz.on && !cont) SDO(nz_collect_begin(h));                                              // NormalizeWrapperEnv: the observe collect_trajectories begins with
    for (int t = 0; t < n_steps; ++t)
        SDO(collect_step(h, use_random, h->collect_noise ? h->collect_noise + (size_t)t * h->cfg.n_envs * h->A : nullptr, nullptr, t == 0, t == n_steps - 1));
    SDO(monitor_end(h));                                                                          // MonitorWrapperEnv: this collection's finished episodes into the window
    if (h->cfg.profile_events) hipEventRecord(h->ev_b, h->stream);
    SDO(ssync(h));
    if (h->cfg.profile_events) { float ms = 0; if (hipEventElapsedTime(&ms, h->ev_a, h->ev_b) == hipSuccess) { h->collect_ms += ms; h->collect_steps += n_steps; } }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (fps) *fps = (double)n_steps * h->cfg.n_envs / (dt > 0 ? dt : 1e-9);                      // :126-128
    h->collect_noise.release(); h->collect_noise_count = 0;
    return DRIL_OK;
}
}  // namespace dril::sac

DRIL_EXPORT int32_t dril_sac_debug_set_collect_noise(dril_sac_handle* h, const float* noise, size_t count) {
    SNEED(h); SDO(ssync(h));
    h->collect_noise.release(); h->collect_noise_count = 0;
    if (!noise || !count) return DRIL_OK;
    SHIP(h, h->collect_noise.alloc_zero(count)); SHIP(h, hipMemcpy(h->collect_noise, noise, count * 4, hipMemcpyHostToDevice)); h->collect_noise_count = count;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_collect_rollout(dril_sac_handle* h, int32_t n_steps, int32_t use_random_actions, double* fps) {
    SNEED(h); S_NOT_EXTERNAL(h, "dril_sac_collect_rollout"); return collect(h, n_steps, use_random_actions != 0, fps);
}
DRIL_EXPORT int32_t dril_sac_collect_continue(dril_sac_handle* h, int32_t n_steps, int32_t use_random_actions, double* fps) {
    SNEED(h); S_NOT_EXTERNAL(h, "dril_sac_collect_continue"); return collect(h, n_steps, use_random_actions != 0, fps, true);
}
