// dril_sac_eval.hip — evaluate_agent (src/evaluation.jl:54-143) and collect_trajectory (src/utils/trajectory_utils.jl:3-49) with the handle's actor on the handle's
// envs, on the device, training state left untouched: dril_sac_evaluate_agent, dril_sac_trajectory_capacity, dril_sac_collect_trajectory and their kernels.  The hidden
// layers of a step are the collection's (actor_hidden, dril_sac_net.hip), a plug-in's action head is the collection's launch (launch_collect_head,
// dril_sac_collect.hip).  The units: dril_sac_handle.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dril_sac_handle.h"
#include "dril_traj_record.h"  // collect_trajectory on the device: the per-env recording sac_traj_env_kernel / sac_traj_record_kernel run (host-compilable)
#include "dril_traj_run.h"     // ... and its setup (blob layout, table of bounds, shadow envs, messages), shared with the PPO handle

using namespace dril;
using namespace dril::sac;

// ---- evaluate_agent on the device (evaluation.jl:90-124; the event list: dril_sac_eval.h; the accounting of one env: sac_eval_account, dril_sac_device.h) -------
namespace {
// a thread per (env, word) over M x max(D, W) lanes: row 0 of either path (t = 0, after the initial observe) and, on plug-ins, every step's row from the per-step
// arrays and the shadow envs' observation.  The rule itself is traj_record_lane
__global__ __launch_bounds__(256) void sac_traj_record_kernel(TrajRec r, TrajMaps x, TrajStep s, int32_t t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t lanes = r.D > r.W ? r.D : r.W;
    if (i >= (int64_t)r.M * lanes) return;
    traj_record_lane(r, x, s, t, (int32_t)(i / lanes), (int32_t)(i % lanes));
}
// plug-ins: after the plug-in's step kernel, over its per-step arrays.  One thread per env, flat index.
__global__ __launch_bounds__(256) void sac_eval_account_kernel(EvalAcctArgs a, const float* __restrict__ rew, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    sac_eval_account(a, e, rew[e], (term[e] | trunc[e]) != 0);
}

// plug-ins: the accounting launch that already follows the plug-in's step kernel also normalises the observation that kernel wrote, in place
__global__ __launch_bounds__(256) void sac_eval_account_norm_kernel(EvalAcctArgs a, const float* __restrict__ rew, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
                                                                    NzEvalArgs nz, int D, float* obs) {
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (i0 < a.E) sac_eval_account(a, i0, rew[i0], (term[i0] | trunc[i0]) != 0);
    for (long long i = i0; i < (long long)a.E * D; i += stride) { const int d = (int)(i % D); obs[i] = nz_obs(obs[i], nz.st[d], nz.st[D + d], nz.eps, nz.clip); }
}
}  // namespace

// ---- evaluate_agent (src/evaluation.jl:54-143) with the handle's actor on the handle's envs -------------------------------------------------------------------
namespace {
template <typename T> int ensure_buf(dril_sac_handle* h, DevBuf<T>& p, size_t n) { if (!p) SHIP(h, p.alloc_zero(n)); return DRIL_OK; }
// the buffers of an evaluation: allocated by the first one, kept; the event list grows with n_eval
int eval_buffers(dril_sac_handle* h, long long cap) {
    const size_t E = (size_t)h->cfg.n_envs;
    SDO(ensure_buf(h, h->ev_state, E * h->S)); SDO(ensure_buf(h, h->ev_obs, E * h->D)); SDO(ensure_buf(h, h->ev_sc, E)); SDO(ensure_buf(h, h->ev_ep, E)); SDO(ensure_buf(h, h->ev_gs, E));
    SDO(ensure_buf(h, h->ev_mon_ret, E)); SDO(ensure_buf(h, h->ev_mon_len, E)); SDO(ensure_buf(h, h->ev_cur_ret, E)); SDO(ensure_buf(h, h->ev_cur_len, E)); SDO(ensure_buf(h, h->ev_counter, 1));
    if (!h->ev_counter_host) SHIP(h, h->ev_counter_host.alloc(1));
    if (cap > 0) SHIP(h, h->ev_events.grow_zero((size_t)cap));
    return DRIL_OK;
}
// the env side of the handle, out (save) or back in (restore): simulator state, counters, the noise stream's position, the current observation, the monitor's sums
int eval_snapshot(dril_sac_handle* h, bool save) {
    const size_t E = (size_t)h->cfg.n_envs;
    auto cp = [&](void* snap, void* live, size_t bytes) { return save ? hipMemcpyAsync(snap, live, bytes, hipMemcpyDeviceToDevice, h->stream) : hipMemcpyAsync(live, snap, bytes, hipMemcpyDeviceToDevice, h->stream); };
    SHIP(h, cp(h->ev_state, h->env.state, E * h->S * 4)); SHIP(h, cp(h->ev_sc, h->env.step_count, E * 4)); SHIP(h, cp(h->ev_ep, h->env.episode, E * 4)); SHIP(h, cp(h->ev_gs, h->env.gstep, E * 4));
    SHIP(h, cp(h->ev_obs, h->obs_cur, E * h->D * 4));                                 // (restore: into whichever of the two observation buffers is current now)
    if (h->mon_window) { SHIP(h, cp(h->ev_mon_ret, h->mon_cur_ret, E * 4)); SHIP(h, cp(h->ev_mon_len, h->mon_cur_len, E * 4)); }
    return DRIL_OK;
}
// ---- the pieces both verbs run: the PPO handle's (dril_eval.hip, under the same names; docs/sac.md "Layout of the host code") over this handle's state ----
// set-aside: the verbs run on the handle's own envs — what a collection would continue from is kept here and put back by eval_finish, on every path
struct EvalKeep { uint64_t seed0; bool ready, obs_valid; };
int eval_set_aside(dril_sac_handle* h, EvalKeep& keep) { keep = EvalKeep{h->env.seed0, h->env.ready, h->obs_valid}; return eval_snapshot(h, true); }
int eval_put_back(dril_sac_handle* h, const EvalKeep& keep) { h->env.seed0 = keep.seed0; h->env.ready = keep.ready; h->obs_valid = keep.obs_valid; return eval_snapshot(h, false); }
// the end of either verb: the state is put back and the stream drained whatever the run returned (rc), and the run's error is the one reported
int eval_finish(dril_sac_handle* h, const EvalKeep& keep, int rc) {
    const std::string msg = h->err;
    int rr = eval_put_back(h, keep); if (rr == DRIL_OK) rr = ssync(h);
    if (rc != DRIL_OK) h->err = msg;
    return rc != DRIL_OK ? rc : rr;
}
// open the episode: the call's seed (env e seeded seed + e; its action noise is that env's stream from step 0), reset!(env), the counter zeroed, the first observation
// — raw, into obs_cur: the wrapper's old_obs is not these verbs' to write — handed to row0() (the recording's row 0 is the original observation), then normalised in
// place with the frozen statistics, nothing updated.  shadow (null: none): a plug-in recording's twins of envs 0..M-1, seeded alike
template <class Row0> int eval_open_episode(dril_sac_handle* h, bool has_seed, uint64_t seed, Row0&& row0, DeviceEnvs* shadow = nullptr) {
    if (has_seed) h->env.seed0 = seed;
    SHIP(h, h->env.reset(h->stream));
    h->env.ready = true; h->obs_valid = false;
    if (shadow) { shadow->seed0 = h->env.seed0; for (void* p : {(void*)shadow->step_count, (void*)shadow->episode, (void*)shadow->gstep}) SHIP(h, hipMemsetAsync(p, 0, (size_t)shadow->E * 4, h->stream)); }
    SHIP(h, hipMemsetAsync(h->ev_counter, 0, 4, h->stream));
    SDO(ensure_obs(h)); SDO(row0());
    if (h->nz.on) { NzApplyArgs a{}; a.w.raw = h->obs_cur; a.w.obs_out = h->obs_cur; SDO(nz_apply(h, a, 0, false, false)); }
    return DRIL_OK;
}
// the loop of either verb (eval_poll_loop of dril_eval.hip): enqueue(steps, launches) advances both; a chunk that would start at or past `bound` fails with (code, bound_msg)
struct EvalPoll { unsigned int seen = 0; long long steps = 0; int32_t launches = 0; };
template <class Enqueue> int eval_poll_loop(dril_sac_handle* h, int want, long long bound, int code, const char* bound_msg, EvalPoll& p, Enqueue&& enqueue) {
    for (p = EvalPoll{}; p.seen < (unsigned int)want; p.seen = *h->ev_counter_host) {
        if (p.steps >= bound) return sfail(h, code, bound_msg);
        SDO(enqueue(p.steps, p.launches));
        SHIP(h, hipMemcpyAsync(h->ev_counter_host, h->ev_counter, 4, hipMemcpyDeviceToHost, h->stream));
        SDO(ssync(h));
    }
    return DRIL_OK;
}
// The pieces of one env step that eval_step and traj_step share; what differs — the accounting, or shadow step, shadow observe and recording — sits between them.
// predict_actions(agent, observations; deterministic): the collection step's hidden layers; the output layer runs in the launch that takes `ca`
int eval_step_actor(dril_sac_handle* h, int deterministic, CollectHeadArgs& ca) { SDO(actor_hidden(h, 0, nullptr, &ca)); ca.deterministic = deterministic ? 1 : 0; return DRIL_OK; }
// NormalizeWrapperEnv with training = false (set_training(eval_env, false) after sync_normalization_stats!, :299-309): the statistics in force, frozen
NzEvalArgs eval_step_nz(const dril_sac_handle* h) { return NzEvalArgs{h->nz.on ? h->nz.half(h->nz.cur) : nullptr, h->nz.on ? h->nz.cfg.norm_obs : 0, h->nz.cfg.epsilon, h->nz.cfg.clip_obs}; }
// a plug-in: the action head into e_envact is launch_collect_head (dril_sac_collect.hip); act!(env, action) of the live envs (monitor pointers null: these episodes do not feed the window)
int eval_step_env(dril_sac_handle* h) { SHIP(h, h->env.step(h->e_envact, EnvStepOut{h->e_rew, h->e_term, h->e_trunc, h->e_tobs, h->obs_nxt}, MonitorArgs{}, h->stream)); return DRIL_OK; }
// a built-in Box kind (A = 1): head, act! and observe are ONE launch (launch_eval_env / launch_traj_env, dril_sac_collect.hip) over the collection's block without push and monitor
CollectEnvArgs eval_env_args(dril_sac_handle* h, const CollectHeadArgs& ca) { return env_kernel_args(h, ca, PushArgs{}, MonitorArgs{nullptr, nullptr, nullptr, nullptr, nullptr}); }
int eval_step_end(dril_sac_handle* h) { SHIP(h, hipGetLastError()); std::swap(h->obs_cur, h->obs_nxt); return DRIL_OK; }
// ---- the evaluation itself ----
// one env step of the evaluation, enqueued: the collection step's hidden layers, then head + act! + observe + accounting
int eval_step(dril_sac_handle* h, int deterministic, int32_t step, unsigned int cap) {
    const int E = h->cfg.n_envs;
    CollectHeadArgs ca; SDO(eval_step_actor(h, deterministic, ca));
    const EvalAcctArgs acct{E, step, h->ev_cur_ret, h->ev_cur_len, h->ev_counter, h->ev_events, cap}; const NzEvalArgs nz = eval_step_nz(h);
    if (h->env.module) {
        launch_collect_head(h, ca); SDO(eval_step_env(h));
        if (nz.st && nz.norm_obs) {                                                    // the accounting launch also normalises the observation the plug-in wrote, in place
            const long long nthr = std::max<long long>(E, std::min<long long>((long long)E * h->D, 256 * 1024));
            hipLaunchKernelGGL(sac_eval_account_norm_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, h->stream, acct, h->e_rew, h->e_term, h->e_trunc, nz, h->D, h->obs_nxt);
        } else hipLaunchKernelGGL(sac_eval_account_kernel, dim3((E + 255) / 256), dim3(256), 0, h->stream, acct, h->e_rew, h->e_term, h->e_trunc);
    } else {
        SHIP(h, launch_eval_env(h, EvalEnvArgs{eval_env_args(h, ca), acct, nz}));
    }
    return eval_step_end(h);
}
// reset!(env) .. the loop of evaluation.jl:90-122 on the device; the host looks at the event counter once per eval_poll steps
int eval_run(dril_sac_handle* h, int n_eval, int deterministic, uint64_t seed, std::vector<SacEvalEvent>& events) {
    const int E = h->cfg.n_envs; const long long cap = sac_eval_event_capacity(n_eval, E);
    SDO(eval_open_episode(h, true, seed, [] { return DRIL_OK; }));
    SHIP(h, hipMemsetAsync(h->ev_cur_ret, 0, (size_t)E * 4, h->stream)); SHIP(h, hipMemsetAsync(h->ev_cur_len, 0, (size_t)E * 4, h->stream));
    // every env finishes an episode within the time limit, so n_eval of them take at most ceil(n_eval / E) time limits; one more, and the steps enqueued past a look
    const long long max_steps = ((long long)(n_eval + E - 1) / E + 1) * (long long)h->cfg.episode_len + h->eval_poll;
    EvalPoll p;
    SDO(eval_poll_loop(h, n_eval, max_steps, DRIL_ERR_UNSUPPORTED, "dril_sac_evaluate_agent: no episode finishes", p, [&](long long& steps, int32_t&) -> int {
        for (int k = 0; k < h->eval_poll; ++k) SDO(eval_step(h, deterministic, (int32_t)(++steps), (unsigned int)cap));
        return DRIL_OK;
    }));
    events.resize((size_t)std::min<long long>(p.seen, cap));
    SHIP(h, hipMemcpy(events.data(), h->ev_events, events.size() * sizeof(SacEvalEvent), hipMemcpyDeviceToHost));
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_sac_evaluate_agent(dril_sac_handle* h, int32_t n_eval, int32_t deterministic, uint64_t seed, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths) {
    SNEED(h);
    if (h->external) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_evaluate_agent: the envs of DRIL_ENV_EXTERNAL live on the host: evaluate there with dril_sac_predict_actions");
    if (n_eval < 1 || !out) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_evaluate_agent: n_eval_episodes >= 1 and out != NULL");
    SDO(eval_buffers(h, sac_eval_event_capacity(n_eval, h->cfg.n_envs)));
    EvalKeep keep; SDO(eval_set_aside(h, keep));
    std::vector<SacEvalEvent> events;
    SDO(eval_finish(h, keep, eval_run(h, n_eval, deterministic, seed, events)));
    sac_eval_stats(events.data(), (int64_t)events.size(), n_eval, out, ep_rewards, ep_lengths);
    return DRIL_OK;
}

// ---- collect_trajectory (src/utils/trajectory_utils.jl:3-49) with the handle's actor on the handle's envs; docs/sac.md, "Trajectories" ---------------------------
// The evaluation's launches with the episode accounting replaced by a recording of envs 0..M-1.  Built-in Box kinds: one env launch per step (sac_traj_env_kernel),
// the env's own thread records from its registers.  Plug-ins: their code objects write terminal_obs where truncated only, so the M SHADOW envs of
// dril_collect_trajectory_device (its comment in dril_eval.hip; built by traj_setup, dril_traj_run.h) take every step a second time, with the same env actions, and
// their observe is the post-step, pre-reset observation sac_traj_record_kernel records.
namespace {
// the recording of one call.  No ClampAdapter (the boxes' clamp_* stay null): TanhScaleAdapter's actions are inside the Box by construction
int traj_prepare(dril_sac_handle* h, const dril_traj_options* o, int32_t Tcap, TrajRun& r) {
    const TrajLayout L = traj_layout((size_t)o->n_trajectories, (size_t)h->D, (size_t)h->A, (size_t)h->S, (size_t)Tcap);
    SHIP(h, traj_setup(h->env, h->stream, h->traj_blob, h->ev_counter, L, traj_env_boxes(h->env), o->final_original != 0, /*drain_before_free=*/true, r));
    return DRIL_OK;
}
// one env step, enqueued: the launches of eval_step without the accounting, and the recording of envs 0..M-1
int traj_step(dril_sac_handle* h, const TrajRun& r, int32_t t, int deterministic, int32_t* launches) {
    const int64_t f0 = h->fwd_launches; const int tag0 = h->col_tag; const NzEvalArgs nz = eval_step_nz(h);
    if (h->env.module) SHIP(h, hipMemcpyAsync(r.shadow.state, h->env.state, (size_t)r.rec.M * h->S * 4, hipMemcpyDeviceToDevice, h->stream));   // the pre-step state of envs 0..M-1 (env-major prefix)
    CollectHeadArgs ca; SDO(eval_step_actor(h, deterministic, ca));
    *launches += (int32_t)(h->fwd_launches - f0) + (h->col_tag != tag0 ? 2 : 0);   // (the f16-piece form of the hidden layers: sac_collect_l1_kernel + sac_collect_l2_kernel)
    if (h->env.module) {
        launch_collect_head(h, ca);
        SHIP(h, r.shadow.step(h->e_envact, EnvStepOut{r.sh_rew, r.sh_term, r.sh_trunc, r.sh_tobs, nullptr}, MonitorArgs{}, h->stream));   // the same step with the same actions' prefix, with no reset after it
        SHIP(h, r.shadow.observe(r.sh_obs, h->stream));                            // observe(env) of the env that did not auto-reset
        SDO(eval_step_env(h));                                                     // act!(env, action), :35
        SHIP(h, traj_record_launch(sac_traj_record_kernel, h->stream, r, TrajStep{h->e_envact, h->e_rew, h->e_term, h->e_trunc, r.sh_obs}, t));
        *launches += 6;                                                             // state copy, head, shadow step, shadow observe, live step, recording
        if (nz.st && nz.norm_obs) { NzApplyArgs a{}; a.w.raw = h->obs_nxt; a.w.obs_out = h->obs_nxt; SDO(nz_apply(h, a, 0, false, false)); *launches += 1; }   // the next observation under the frozen statistics, in place
    } else {
        SHIP(h, launch_traj_env(h, TrajEnvArgs{eval_env_args(h, ca), nz, r.rec, r.maps, t}));
        *launches += 1;
    }
    return eval_step_end(h);
}
// reset!(env) .. the loop of trajectory_utils.jl:16-45 on the device; the host looks at the finished-counter once per K steps and never enqueues a step past Tcap
int traj_run(dril_sac_handle* h, const dril_traj_options* o, TrajRun& r, float* observations, float* actions, float* rewards, int32_t* lengths, uint8_t* end_flags, dril_traj_info* info) {
    const int Tcap = r.rec.Tcap, K = o->poll_steps > 0 ? o->poll_steps : h->eval_poll;
    const auto row0 = [&]() -> int {                                               // the original observation, before the agent's copy is normalised
        SHIP(h, traj_record_launch(sac_traj_record_kernel, h->stream, r, TrajStep{nullptr, nullptr, nullptr, nullptr, h->obs_cur}, 0));
        return DRIL_OK;
    };
    SDO(eval_open_episode(h, o->has_seed != 0, o->seed, row0, h->env.module ? &r.shadow : nullptr));
    EvalPoll p;
    SDO(eval_poll_loop(h, r.rec.M, Tcap, DRIL_ERR_HIP, "dril_sac_collect_trajectory: a trajectory is still open after its capacity (internal)", p, [&](long long& steps, int32_t& launches) -> int {   // (step Tcap finalises every open one)
        for (int k = 0; k < K && steps < Tcap; ++k) SDO(traj_step(h, r, (int32_t)(++steps), o->deterministic ? 1 : 0, &launches));
        return DRIL_OK;
    }));
    const TrajCopyOut c = traj_copy_out(h->stream, r.rec, observations, (uint32_t*)actions, rewards, lengths, end_flags);
    if (const std::string msg = traj_report("dril_sac_collect_trajectory", c, Tcap, (int32_t)p.steps, p.launches, 0, info); !msg.empty()) return sfail(h, DRIL_ERR_HIP, msg);
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_sac_trajectory_capacity(const dril_sac_handle* h, const dril_traj_options* o, int32_t* capacity) {
    if (!h) return sfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    dril_sac_handle* hh = const_cast<dril_sac_handle*>(h);
    if (!o || !capacity || o->max_steps < 0) return sfail(hh, DRIL_ERR_INVALID_ARG, "dril_sac_trajectory_capacity: options and capacity != NULL, max_steps >= 0");
    if (h->external) return sfail(hh, DRIL_ERR_UNSUPPORTED, "dril_sac_trajectory_capacity: the envs of DRIL_ENV_EXTERNAL live on the host, with the caller");
    *capacity = traj_capacity(o->max_steps, h->env.episode_len);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_collect_trajectory(dril_sac_handle* h, const dril_traj_options* o, float* observations, float* actions, float* rewards, int32_t* lengths,
                                                uint8_t* end_flags, dril_traj_info* info) {
    SNEED(h);
    if (h->external) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_collect_trajectory: the envs of DRIL_ENV_EXTERNAL live on the host: record there, in a loop over dril_sac_predict_actions");
    if (const std::string msg = traj_options_error("dril_sac_collect_trajectory", o, observations && actions && rewards && lengths && end_flags, h->cfg.n_envs); !msg.empty()) return sfail(h, DRIL_ERR_INVALID_ARG, msg);
    int32_t Tcap = 0;
    if (const std::string msg = traj_size_error("dril_sac_collect_trajectory", o, h->env.episode_len, h->D, h->A, info, &Tcap); !msg.empty()) return sfail(h, DRIL_ERR_INVALID_ARG, msg);
    SDO(eval_buffers(h, 0));
    TrajRun run{}; SDO(traj_prepare(h, o, Tcap, run));
    // as dril_sac_evaluate_agent: what a collection would continue from is set aside here and put back by eval_finish, on every path
    EvalKeep keep; SDO(eval_set_aside(h, keep));
    return eval_finish(h, keep, traj_run(h, o, run, observations, actions, rewards, lengths, end_flags, info));
}
