// dril_eval.hip — evaluate_agent and collect_trajectory of the PPO handle (dril_handle.h): the host loop, the evaluation on the device with the training state set aside
// and put back, the recording of trajectories on the device, and the four small kernels of their accounting and recording.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "dril_handle.h"

#include "dril_traj_record.h"  // collect_trajectory on the device: the per-env recording traj_record_kernel runs (host-compilable)
#include "dril_traj_run.h"    // ... and its setup (blob layout, table of bounds, shadow envs, messages), shared with the SAC handle

using namespace dril;
using namespace dril::ppo;

// ---- evaluate_agent (src/evaluation.jl:54-143) ------------------------------------------------------------
namespace {
int evaluate_agent_loop(dril_handle* h, int32_t n_eval, int32_t deterministic, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths, bool raw) {
    const int E = h->cfg.n_envs;
    int rc = DRIL_OK;
    HIPCHK(h, h->env.reset(h->stream));   // reset!(env), :87
    if (h->mon_cur_ret) { HIPCHK(h, hipMemsetAsync(h->mon_cur_ret, 0, (size_t)E * 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->mon_cur_len, 0, (size_t)E * 4, h->stream)); }
    h->env.ready = true;
    std::vector<float> rew(E), cur_r(E, 0.f), er; std::vector<uint8_t> term(E), trunc(E); std::vector<int32_t> cur_l(E, 0), el;
    float* rew_n = h->e_rew_n;                                                   // wrapper-delivered rewards (see dril_env_step)
    rc = observe_dev(h, true); if (rc) return rc;                                // observations = observe(env), :88
    int steps = 0;
    while ((int)er.size() < n_eval) {
        PolicyArgs p = policy_args(h, h->e_obs, E, nullptr, h->e_act, nullptr, h->logp /*scratch*/, nullptr, 0);
        p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.deterministic = deterministic ? 1 : 0;
        p.logp = h->e_rew;                                                       // logprobs are not needed: park them in a scratch array
        HIPCHK(h, run_policy(h, p));   // predict_actions(agent, observations; deterministic), :92
        rc = step_dev(h, h->e_act, rew_n, nullptr); if (rc) return rc;           // act!(env, actions), :94
        HIPCHK(h, hipMemcpyAsync(rew.data(), raw ? h->e_rew : rew_n, (size_t)E * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(term.data(), h->e_term, E, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(trunc.data(), h->e_trunc, E, hipMemcpyDeviceToHost, h->stream));
        rc = observe_dev(h, true); if (rc) return rc;                            // observations = observe(env), :97
        rc = sync(h); if (rc) return rc;
        ++steps;
        for (int i = 0; i < E; ++i) {
            cur_r[i] += rew[i]; cur_l[i] += 1;                                   // :95-96
            if ((term[i] || trunc[i]) && (int)er.size() < n_eval) { er.push_back(cur_r[i]); el.push_back(cur_l[i]); cur_r[i] = 0.f; cur_l[i] = 0; }   // :100-121
        }
        if (steps > 100000000 / (E > 0 ? E : 1) + 100000) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_evaluate_agent: no episode finishes");
    }
    double mr = 0, ml = 0; for (int i = 0; i < n_eval; ++i) { mr += er[i]; ml += el[i]; }
    mr /= n_eval; ml /= n_eval;
    double vr = 0, vl = 0; for (int i = 0; i < n_eval; ++i) { vr += (er[i] - mr) * (er[i] - mr); vl += (el[i] - ml) * (el[i] - ml); }
    out->mean_reward = mr; out->mean_length = ml;
    out->std_reward = std::sqrt(vr / (n_eval - 1)); out->std_length = std::sqrt(vl / (n_eval - 1));     // Julia std: corrected; NaN for one episode
    out->n_episodes = n_eval; out->n_steps = steps;
    if (ep_rewards) std::memcpy(ep_rewards, er.data(), (size_t)n_eval * 4);
    if (ep_lengths) std::memcpy(ep_lengths, el.data(), (size_t)n_eval * 4);
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_evaluate_agent(dril_handle* h, int32_t n_eval, int32_t deterministic, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths) {
    NEED(h); NOT_EXTERNAL(h, "dril_evaluate_agent");
    if (n_eval < 1 || !out) return fail(h, DRIL_ERR_INVALID_ARG, "dril_evaluate_agent: n_eval_episodes >= 1 and out != NULL");
    const int E = h->cfg.n_envs;
    int rc = ensure_wimg(h); if (rc) return rc;
    if (h->env.module && h->pn.on) {                                                 // a plug-in env under dril_normalize_enable: the statistics in force, frozen; nothing of the wrapper moves
        const size_t ED = (size_t)E * h->D;
        DevBuf<float> keep; HIPCHK(h, keep.alloc(ED + 2 * (size_t)E));    // returns | old_rewards | old_obs
        const int training = h->pn.cfg.training;
        hipError_t e = hipMemcpyAsync(keep, h->env.disc_returns, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(keep + E, h->e_rew, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(keep + 2 * (size_t)E, h->e_obs_raw, ED * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) {
            h->pn.cfg.training = 0;                                              // set_training(eval_env, false): neither statistics nor `returns` are updated
            rc = evaluate_agent_loop(h, n_eval, deterministic, out, ep_rewards, ep_lengths, /*raw_rewards=*/true);
            h->pn.cfg.training = training;
            e = hipMemcpyAsync(h->env.disc_returns, keep, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h->e_rew, keep + E, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h->e_obs_raw, keep + 2 * (size_t)E, ED * 4, hipMemcpyDeviceToDevice, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
        keep.release();
        if (rc) return rc;
        HIPCHK(h, e);
        return DRIL_OK;
    }
    return evaluate_agent_loop(h, n_eval, deterministic, out, ep_rewards, ep_lengths, h->mon_cur_ret != nullptr);   // monitored: infos[i]["episode"]["r"] is the raw return
}

// ---- evaluate_agent on the device, training state left untouched (docs/evaluation.md) --------------------------------------------------------
// The loop of evaluate_agent_loop above with the host taken out of it: the episode accounting of dril_eval_account.h runs on the device, the host looks at ONE 4-byte
// counter every K env steps, and what the loop writes of the env side is set aside before and put back after.  Two forms of the K steps between two looks:
//   path 1  ONE launch of evaluate_kernel (dril_kernels.hip): built-in kinds on the fused shapes of width 64 / 128 / 256 with no normaliser — and, where the
//           options ask for it (DRIL_EVAL_OPT_PERSISTENT), under cfg.norm_* too: evaluate_modes_kernel reads the frozen statistics as an argument
//   path 0  per env step the launches run_policy / step_dev / observe_dev make, and eval_account_kernel over the step's reward and done arrays: everything else
//   path 2  on request, a plug-in handle whose code object carries a usable evaluation kernel (include/device/dril_env_evaluate.h): ONE launch of that kernel leaves the K
//           rows of raw rewards and flag bytes, ONE launch of eval_account_rows_kernel walks them: 2 launches per K env steps
namespace dril {   // (a named namespace: tools/kernel_resources.py lists the kernels by their names)
// path 2: a thread per env walks its K rows in step order.  Inside the launch events are unordered, as on path 1: the list has eval_event_capacity(n, E, K) slots
__global__ __launch_bounds__(256) void eval_account_rows_kernel(EvalAcct a, int32_t step0, int32_t K, const float* __restrict__ rew, const uint8_t* __restrict__ flags) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    float ret = a.cur_ret[e]; int32_t len = a.cur_len[e];
    for (int32_t k = 0; k < K; ++k) { const size_t i = (size_t)k * a.E + e; eval_account(a, step0 + k + 1, e, rew[i], flags[i] != 0, ret, len); }
    a.cur_ret[e] = ret; a.cur_len[e] = len;
}
// path 2, recording: the per-trajectory rule over the K rows, a thread per (env, word) as traj_record_kernel
__global__ __launch_bounds__(256) void traj_record_rows_kernel(TrajRec r, TrajMaps x, TrajRows s, int32_t t0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t lanes = r.D > r.W ? r.D : r.W;
    if (i >= (int64_t)r.M * lanes) return;
    traj_record_lane_rows(r, x, s, t0, (int32_t)(i / lanes), (int32_t)(i % lanes));
}
}  // namespace dril
namespace {
__global__ __launch_bounds__(256) void eval_account_kernel(EvalAcct a, int32_t step, const float* __restrict__ rew, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    eval_account_env(a, step, e, rew[e], (term[e] | trunc[e]) != 0);
}
// the default K of each path: UNMEASURED starting points (docs/evaluation.md, "Measured") — the SAC verb's min(time limit, 32) for the step-granular path, a guess for the
// persistent one.  No more than the time limit, after which every env has finished an episode
constexpr int kEvalPollStepwise = 32, kEvalPollPersistent = 64;
constexpr long long kEvalMaxLaunchEvents = 1ll << 22;   // E K of one evaluate_kernel launch: 64 MB of event slots at the most
// requested: the caller's opt-in (DRIL_EVAL_OPT_PERSISTENT / DRIL_TRAJ_OPT_PERSISTENT), which admits a normalised handle; without it, the rule every caller has had
bool eval_persistent_applies(const dril_handle* h, bool requested = false) {
    const int hd = h->cfg.hidden1;
    return !h->generic && !h->env.module && (!normalizing(h) || requested) && !h->force_stepwise && (hd == 64 || hd == 128 || hd == 256);   // (DRIL_FORCE_STEPWISE: the step-granular launches, as for the collection)
}
// evaluate_kernel's arguments from the handle (the rollout launcher's choices: fwd_exact, action_start, fixed_length_episodes); T and step0 are set per launch
void eval_kernel_args(const dril_handle* h, EvalKernelArgs& g, int deterministic) {
    RolloutArgs& a = g.r;
    a.params = h->params; a.state = h->env.state; a.step_count = h->env.step_count; a.episode = h->env.episode; a.gstep = h->env.gstep;
    a.E = h->cfg.n_envs; a.episode_len = h->env.episode_len; a.fixed_len = h->env.fixed_len; a.action_start = h->env.action_start; a.log_std_off = h->log_std_off;
    a.env_seed0 = h->env.seed0; a.actor = h->actor; a.critic = h->critic; a.exact_f32 = fwd_exact(h) ? 1 : 0;
    a.w2a_actor = a.exact_f32 ? h->w2a_actor : (const float*)h->w2pf_actor.get(); a.w2a_critic = nullptr;
    g.deterministic = deterministic ? 1 : 0;
}
// the frozen NormalizeWrapperEnv as evaluate_modes_kernel takes it: the halves of the statistics in force, read only.  raw: the accounting counts raw rewards
void eval_mode_norm(const dril_handle* h, EvalModeArgs& x, bool raw) {
    x.obs_stats = h->obs_rms + h->obs_par; x.ret_stats = h->ret_rms + h->ret_par;
    x.norm_obs = h->cfg.norm_obs ? 1 : 0; x.norm_reward = h->cfg.norm_reward ? 1 : 0; x.count_raw = raw ? 1 : 0;
    x.clip_obs = h->cfg.clip_obs; x.clip_reward = h->cfg.clip_reward; x.eps = h->cfg.norm_epsilon;
}
// path 2 applies: the request, a plug-in handle, a usable kernel for this net; DRIL_FORCE_STEPWISE wins, as everywhere
bool eval_fused_applies(const dril_handle* h, bool requested) {
    return requested && h->env.module && !h->force_stepwise && fused_evaluate_unavailable(h).empty();
}
// the argument block of a plug-in's evaluation kernel for launches of up to K steps, M recorded envs (shadow: their never-resetting twins; null when M == 0); the
// handle's blob is grown to hold the scratch.  The frozen statistics of dril_normalize_enable travel as pointers into the half in force and are only read
int eval_fused_args(dril_handle* h, DrilEnvEvaluateArgs& g, int deterministic, int K, int M, const DeviceEnvs* shadow) {
    const size_t E = (size_t)h->cfg.n_envs, D = (size_t)h->D, W = h->discrete ? 1 : (size_t)h->A, Ks = (size_t)K, Ms = (size_t)M;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_obs = take(E * D * 4), o_act = take(E * W * 4), o_rew = take(Ks * E * 4), o_flg = take(Ks * E);
    const size_t o_obs0 = take(Ms * D * 4), o_ract = take(Ks * Ms * W * 4), o_robs = take(Ks * Ms * D * 4);
    if (off > 0) HIPCHK(h, h->evalf_blob.grow(off));
    char* b = h->evalf_blob;
    g = DrilEnvEvaluateArgs{};
    g.r.env = h->env.args(); g.r.env.obs = (float*)(b + o_obs);                       // (after the call's seed is in force: seed0 is the one the reset used)
    g.r.T = K; g.r.n_hidden = h->gd.nh; g.r.activation = h->gd.act; g.r.n_params = h->P;
    for (int l = 0; l < h->gd.nh; ++l) g.r.hidden[l] = h->gd.H[l];
    g.r.actor_off = h->actor.w1; g.r.log_std_off = h->log_std_off; g.r.params = h->params;
    g.r.act = b + o_act; g.r.rew = (float*)(b + o_rew); g.r.flags = (uint8_t*)(b + o_flg);
    g.deterministic = deterministic ? 1 : 0; g.n_record = M;
    if (h->pn.on && h->pn.cfg.norm_obs) { g.norm_mean = h->pn.half(h->pn.cur); g.norm_var = g.norm_mean + h->pn.D; g.norm_eps = h->pn.cfg.epsilon; g.norm_clip = h->pn.cfg.clip_obs; }
    if (M > 0) { g.shadow = shadow->args(); g.rec_obs0 = (float*)(b + o_obs0); g.rec_act = b + o_ract; g.rec_obs = (float*)(b + o_robs); }
    return DRIL_OK;
}
void eval_keep_list(dril_handle* h, bool persistent, EvalKeep& k) {
    const size_t E = (size_t)h->cfg.n_envs, ED = E * h->D * 4;
    k.arrays = {{h->env.state, E * h->S * 4}, {h->env.step_count, E * 4}, {h->env.episode, E * 4}, {h->env.gstep, E * 4}, {h->env.disc_returns, E * 4}};
    if (persistent) return;                                                        // evaluate_kernel writes the envs alone (reset! zeroes `returns`)
    const std::pair<void*, size_t> step_arrays[] = {{h->e_obs, ED}, {h->e_rew, E * 4}, {h->e_tobs, ED}, {h->e_term, E}, {h->e_trunc, E}, {h->e_act, E * act_bytes_per(h)}};
    k.arrays.insert(k.arrays.end(), std::begin(step_arrays), std::end(step_arrays));
    if (normalizing(h) || h->pn.on) { k.arrays.push_back({h->e_obs_raw, ED}); k.arrays.push_back({h->e_rew_n, E * 4}); }
    if (normalizing(h)) { k.arrays.push_back({h->obs_rms, 2 * sizeof(RmsState)}); k.arrays.push_back({h->ret_rms, 2 * sizeof(RmsState)}); }   // both halves: a frozen apply copies in -> out and flips the parity
}
int eval_keep_copy(dril_handle* h, const EvalKeep& k, bool save) {
    size_t off = 0;
    for (const auto& a : k.arrays) {
        if (save) HIPCHK(h, hipMemcpyAsync(h->eval_snap + off, a.first, a.second, hipMemcpyDeviceToDevice, h->stream));
        else HIPCHK(h, hipMemcpyAsync(a.first, h->eval_snap + off, a.second, hipMemcpyDeviceToDevice, h->stream));
        off += (a.second + 15) & ~(size_t)15;
    }
    return DRIL_OK;
}
int eval_buffers(dril_handle* h, const EvalKeep& k, long long cap) {
    const size_t E = (size_t)h->cfg.n_envs;
    size_t bytes = 0; for (const auto& a : k.arrays) bytes += (a.second + 15) & ~(size_t)15;
    if (bytes > 0) HIPCHK(h, h->eval_snap.grow(bytes));
    if (!h->eval_cur_ret) HIPCHK(h, h->eval_cur_ret.alloc(E)); if (!h->eval_cur_len) HIPCHK(h, h->eval_cur_len.alloc(E)); if (!h->eval_counter) HIPCHK(h, h->eval_counter.alloc(1));
    if (!h->eval_counter_host) HIPCHK(h, h->eval_counter_host.alloc(1));
    if (cap > 0) HIPCHK(h, h->eval_events.grow((size_t)cap));
    return DRIL_OK;
}
// The pieces of one step-granular env step that the evaluation (eval_step_granular) and the recording (traj_step) share; what differs sits between them.
// wrapped: a NormalizeWrapperEnv (cfg.norm_* or dril_normalize_enable) is around the envs, its statistics frozen for the call
bool eval_wrapped(const dril_handle* h) { return normalizing(h) || h->pn.on; }
// predict_actions(agent, observations; deterministic), evaluation.jl:92 / trajectory_utils.jl:28
int eval_step_policy(dril_handle* h, int deterministic) {
    PolicyArgs p = policy_args(h, h->e_obs, h->cfg.n_envs, nullptr, h->e_act, nullptr, h->e_rew /*log-probabilities are not needed: parked where act! writes next*/, nullptr, 0);
    p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.deterministic = deterministic ? 1 : 0;
    HIPCHK(h, run_policy(h, p));
    return DRIL_OK;
}
// act!(env, actions), :94 / :35.  *rew: the rewards an accounting reads — raw (dril_evaluate_agent's rule; they stay in e_rew), else what the wrapper delivers
int eval_step_env(dril_handle* h, bool raw, const float** rew) {
    float* delivered = (h->env.module && !h->pn.on) ? nullptr : h->e_rew_n;
    *rew = (eval_wrapped(h) && !raw && delivered) ? delivered : h->e_rew;
    return eval_wrapped(h) ? step_dev(h, h->e_act, delivered, nullptr) : env_step_arrays(h, h->e_act);   // no wrapper: the raw step is the whole step (as dril_env_step)
}
// observations = observe(env), :88, :97 / :17, :24-26
int eval_step_observe(dril_handle* h) { if (eval_wrapped(h)) return observe_dev(h, true); HIPCHK(h, h->env.observe(h->e_obs, h->stream)); return DRIL_OK; }
// the launches of the three above.  g0: gws.launches before the policy (a generic shape's forward is several launches)
int32_t eval_step_launches(const dril_handle* h, int64_t g0) { return (h->generic ? (int32_t)(h->gws.launches - g0) : 1) + 2 + (eval_wrapped(h) ? (h->env.module ? 2 : 3) : 0); }
// one env step of path 0, enqueued: predict_actions -> act! -> accounting -> observe.  raw: the accounting reads the raw rewards (dril_evaluate_agent's rule)
int eval_step_granular(dril_handle* h, const EvalAcct& acct, int32_t step, int deterministic, bool raw, int32_t* launches) {
    const int E = h->cfg.n_envs; const int64_t g0 = h->gws.launches; const float* rew = nullptr;
    { int rc = eval_step_policy(h, deterministic); if (rc) return rc; }
    { int rc = eval_step_env(h, raw, &rew); if (rc) return rc; }
    hipLaunchKernelGGL(eval_account_kernel, dim3((E + 255) / 256), dim3(256), 0, h->stream, acct, step, rew, h->e_term, h->e_trunc);
    HIPCHK(h, hipGetLastError());
    { int rc = eval_step_observe(h); if (rc) return rc; }
    *launches += eval_step_launches(h, g0);
    return DRIL_OK;
}
// K: env steps between two looks at the counter — the ONE rule of both verbs on every path (the table of callers: docs/evaluation.md, "K").  poll_steps > 0 replaces
// the default and takes the same caps.  persistent: one launch runs the K steps (paths 1 and 2).  cap_events: E K of a launch is bounded by kEvalMaxLaunchEvents
// (the list it may fill: eval_event_capacity, dril_eval_account.h); the recording on path 1 does not ask for it.  cap_steps: Tcap, for the recording on path 2 alone
int eval_poll_steps(const dril_handle* h, int32_t poll_steps, bool persistent, bool cap_events, int cap_steps = INT32_MAX) {
    const int K = std::min(poll_steps > 0 ? poll_steps : std::max(1, std::min(h->env.episode_len, persistent ? kEvalPollPersistent : kEvalPollStepwise)), cap_steps);
    return cap_events ? (int)std::max<long long>(1, std::min<long long>(K, kEvalMaxLaunchEvents / std::max(1, h->cfg.n_envs))) : K;
}
// open the episode, for both verbs: the call's seed (env e of rank r: seed + r E + e), reset!(env) (evaluation.jl:87 / trajectory_utils.jl:10), the counter zeroed — the
// device word the kernels count in (the handle's own, or its word of a population's array).  shadow (null: none): a recording's twins of envs 0..M-1, seeded alike
int eval_open_episode(dril_handle* h, bool has_seed, uint64_t seed, unsigned int* counter, DeviceEnvs* shadow = nullptr) {
    if (has_seed) h->env.seed0 = seed + (uint64_t)h->cfg.rank * (uint64_t)h->cfg.n_envs;
    HIPCHK(h, h->env.reset(h->stream));
    h->env.ready = true;
    if (shadow) shadow->seed0 = h->env.seed0;
    if (shadow) for (void* p : {(void*)shadow->step_count, (void*)shadow->episode, (void*)shadow->gstep}) HIPCHK(h, hipMemsetAsync(p, 0, (size_t)shadow->E * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(counter, 0, 4, h->stream));
    return DRIL_OK;
}
}  // namespace
namespace dril::ppo {
// ---- the pieces of dril_evaluate_agent_device, in the order it runs them: prepare, set-aside, reset, enqueue, put-back, reduce.  dril_population_evaluate_device
// calls the same pieces per member (as pop_collect / pop_update call rollout_args / update_begin), so a member's evaluation is that of its handle alone ----
// prepare: which path runs, K, the list's capacity, what the call will set aside, the buffers
int eval_prepare(dril_handle* h, const dril_eval_options* o, EvalPlan& pl) {
    { int rc = ensure_wimg(h); if (rc) return rc; }
    pl.persistent = !o->force_step_granular && eval_persistent_applies(h, o->reserved[DRIL_EVAL_OPT_PERSISTENT] != 0);
    pl.fused = !o->force_step_granular && eval_fused_applies(h, o->reserved[DRIL_EVAL_OPT_PERSISTENT] != 0);   // path 2: a plug-in's own evaluation kernel (never both)
    pl.raw = (h->env.module && h->pn.on) || h->mon_cur_ret != nullptr;                  // dril_evaluate_agent's rule: raw returns under the monitor (and under a plug-in's normaliser)
    eval_keep_list(h, pl.persistent || pl.fused, pl.keep);                             // (path 2 writes the envs and scratch of its own: the per-step arrays are not touched)
    pl.K = eval_poll_steps(h, o->poll_steps, pl.persistent || pl.fused, /*cap_events=*/pl.persistent || pl.fused);
    pl.cap = eval_event_capacity(o->n_eval_episodes, h->cfg.n_envs, (pl.persistent || pl.fused) ? pl.K : 1);   // (path 0: one launch per env step)
    return eval_buffers(h, pl.keep, pl.cap);
}
// set-aside: the evaluation runs on the handle's own envs — what training would continue from is kept here and put back by eval_put_back, on every path
int eval_set_aside(dril_handle* h, EvalKeep& keep) {
    keep.seed0 = h->env.seed0; keep.ready = h->env.ready; keep.obs_par = h->obs_par; keep.ret_par = h->ret_par; keep.norm_training = h->cfg.norm_training;
    keep.pn_training = h->pn.cfg.training; keep.gws_launches = h->gws.launches;
    { int rc = eval_keep_copy(h, keep, true); if (rc) return rc; }
    h->cfg.norm_training = 0; h->pn.cfg.training = 0;                                  // set_training(env, false): the statistics in force, frozen; `returns` stands still
    keep.mon_cur_ret = std::move(h->mon_cur_ret);                                      // evaluation episodes do not enter the training env's MonitorWrapperEnv: its launches are not made
    return DRIL_OK;
}
int eval_reset(dril_handle* h, const dril_eval_options* o, unsigned int* counter, long long cap, EvalAcct& acct) {
    const int E = h->cfg.n_envs;
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, counter); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(h->eval_cur_ret, 0, (size_t)E * 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->eval_cur_len, 0, (size_t)E * 4, h->stream));
    acct = EvalAcct{E, h->eval_cur_ret, h->eval_cur_len, counter, h->eval_events, (unsigned int)cap};
    return DRIL_OK;
}
// every env finishes an episode within the time limit, so n of them take at most ceil(n / E) time limits; one more, and the steps enqueued past a look
long long eval_max_steps(const dril_handle* h, int n_eval, int K) {
    const int E = h->cfg.n_envs;
    return ((long long)(n_eval + E - 1) / E + 1) * (long long)h->env.episode_len + K;
}
// enqueue (path 1): the argument block of the launches of K steps; step0 is set per launch
void eval_persistent_args(const dril_handle* h, const dril_eval_options* o, int K, const EvalAcct& acct, EvalKernelArgs& g) {
    eval_kernel_args(h, g, o->deterministic); g.r.T = K; g.acct = acct;           // (after the seed of eval_reset: env_seed0 is the one the reset used)
}
// put-back: the host-side words, and the copies home enqueued (the caller drains the stream)
int eval_put_back(dril_handle* h, EvalKeep& keep) {
    h->env.seed0 = keep.seed0; h->env.ready = keep.ready; h->obs_par = keep.obs_par; h->ret_par = keep.ret_par; h->cfg.norm_training = keep.norm_training;
    h->pn.cfg.training = keep.pn_training; h->mon_cur_ret = std::move(keep.mon_cur_ret); h->gws.launches = keep.gws_launches;
    return eval_keep_copy(h, keep, false);
}
// reduce: the first n_eval_episodes events in (step, env) order
void eval_reduce(SacEvalEvent* events, int64_t n_events, const dril_eval_options* o, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths) { sac_eval_stats(events, n_events, o->n_eval_episodes, out, ep_rewards, ep_lengths); }
}  // namespace dril::ppo
namespace {
// the end of either verb, after eval_set_aside: the state is put back and the stream drained whatever the run returned (rc), and the run's error is the one reported
int eval_finish(dril_handle* h, EvalKeep& keep, const char* verb, int rc) {
    const std::string msg = h->err;
    int rr = eval_put_back(h, keep);
    if (rr == DRIL_OK) { const hipError_t e = hipStreamSynchronize(h->stream); if (e != hipSuccess) rr = fail(h, DRIL_ERR_HIP, std::string(verb) + ": " + hipGetErrorString(e)); }
    if (rc != DRIL_OK) { h->err = msg; return rc; }
    return rr;
}
// the loop of either verb on every path: until `want` episodes / trajectories are counted, enqueue a chunk of env steps, copy the 4-byte counter home, drain, read it.
// enqueue(steps, launches) -> status advances both by what it put into the stream.  A chunk that would start at or past `bound` steps fails with (code, bound_msg)
struct EvalPoll { unsigned int seen = 0; long long steps = 0; int32_t launches = 0; };
template <class Enqueue> int eval_poll_loop(dril_handle* h, int want, long long bound, int code, const char* bound_msg, EvalPoll& p, Enqueue&& enqueue) {
    p = EvalPoll{};
    while (p.seen < (unsigned int)want) {
        if (p.steps >= bound) return fail(h, code, bound_msg);
        { int rc = enqueue(p.steps, p.launches); if (rc) return rc; }
        HIPCHK(h, hipMemcpyAsync(h->eval_counter_host, h->eval_counter, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        p.seen = *h->eval_counter_host;
    }
    return DRIL_OK;
}
int eval_device_run(dril_handle* h, const dril_eval_options* o, const EvalPlan& pl, std::vector<SacEvalEvent>& events, dril_eval_info* info) {
    const bool persistent = pl.persistent, fused = pl.fused, raw = pl.raw; const int K = pl.K; const long long cap = pl.cap;
    const int E = h->cfg.n_envs, n_eval = o->n_eval_episodes;
    EvalAcct acct{};
    { int rc = eval_reset(h, o, h->eval_counter, cap, acct); if (rc) return rc; }
    EvalKernelArgs g{}; EvalModeArgs x{}; DrilEnvEvaluateArgs gf{};
    const bool modes = persistent && normalizing(h);                              // a frozen normaliser: evaluate_modes_kernel; otherwise evaluate_kernel as ever
    if (fused) { int rc = eval_fused_args(h, gf, o->deterministic, K, 0, nullptr); if (rc) return rc; }   // (the kernel opens every launch with its own observe)
    else if (persistent) {
        eval_persistent_args(h, o, K, acct, g);
        if (modes) eval_mode_norm(h, x, raw);
    } else { int rc = eval_step_observe(h); if (rc) return rc; }                  // observations = observe(env), :88
    EvalPoll p;
    const int rc = eval_poll_loop(h, n_eval, eval_max_steps(h, n_eval, K), DRIL_ERR_UNSUPPORTED, "dril_evaluate_agent_device: no episode finishes", p, [&](long long& steps, int32_t& launches) -> int {
        if (fused) {
            HIPCHK(h, h->env.launch_evaluate(gf, h->stream));
            hipLaunchKernelGGL(eval_account_rows_kernel, dim3((E + 255) / 256), dim3(256), 0, h->stream, acct, (int32_t)steps, (int32_t)K, gf.r.rew, gf.r.flags);
            HIPCHK(h, hipGetLastError());
            steps += K; launches += 2;
        }
        else if (persistent) { g.step0 = (int32_t)steps; HIPCHK(h, launch_evaluate(h->env.kind, h->cfg.hidden1, g, h->stream, modes ? &x : nullptr)); steps += K; launches += 1; }
        else for (int k = 0; k < K; ++k) { int rc = eval_step_granular(h, acct, (int32_t)(++steps), (o->deterministic ? 1 : 0), raw, &launches); if (rc) return rc; }
        return DRIL_OK;
    });
    if (rc) return rc;
    events.resize((size_t)std::min<long long>(p.seen, cap));
    HIPCHK(h, hipMemcpyAsync(events.data(), h->eval_events, events.size() * sizeof(SacEvalEvent), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (info) { info->path = fused ? 2 : persistent ? 1 : 0; info->launches = p.launches; info->steps_enqueued = (int32_t)p.steps; info->events = (int32_t)p.seen; }
    return DRIL_OK;
}
const char* const kEvalArgMsg = "dril_evaluate_agent_device: options and out != NULL, n_eval_episodes >= 1, poll_steps >= 0";
}  // namespace
DRIL_EXPORT int32_t dril_eval_options_default(dril_eval_options* o) {
    if (!o) return DRIL_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->n_eval_episodes = 10; o->deterministic = 1;                                     // evaluation.jl:57-58
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_evaluate_agent_device(dril_handle* h, const dril_eval_options* o, dril_eval_stats* out, float* ep_rewards, int32_t* ep_lengths, dril_eval_info* info) {
    NEED(h); NOT_EXTERNAL(h, "dril_evaluate_agent");
    if (!o || !out || o->n_eval_episodes < 1 || o->poll_steps < 0) return fail(h, DRIL_ERR_INVALID_ARG, kEvalArgMsg);
    if (info) std::memset(info, 0, sizeof(*info));
    EvalPlan pl;
    { int rc = eval_prepare(h, o, pl); if (rc) return rc; }
    { int rc = eval_set_aside(h, pl.keep); if (rc) return rc; }
    std::vector<SacEvalEvent> events;
    { int rc = eval_finish(h, pl.keep, "dril_evaluate_agent_device", eval_device_run(h, o, pl, events, info)); if (rc) return rc; }
    eval_reduce(events.data(), (int64_t)events.size(), o, out, ep_rewards, ep_lengths);
    return DRIL_OK;
}

// ---- collect_trajectory on the device, training state left untouched (trajectory_utils.jl:3-49; docs/evaluation.md, "Trajectories") ------------------------------
// The step-granular launches of the evaluation above, with the episode accounting replaced by a recording of envs 0..M-1.  What no existing kernel produces is the
// observation after the last step of a TERMINATED episode (the step kernels write terminal_obs where truncated, then auto-reset), so M SHADOW envs take every step
// a second time: a DeviceEnvs view of the same kind / plug-in with its own arrays, fixed_len = 1 (masks the terminated flag, nothing else) and an unreachable time
// limit, so it never resets.  Per env step it is given the live envs' pre-step state, takes the step with the same actions, and its observe is the post-step,
// pre-reset observation of every recorded env — the very float operations the live step ran before its auto-reset.  No kernel, argument block or code object changes.
namespace dril {   // (a named namespace: tools/kernel_resources.py lists the kernel by its name)
__global__ __launch_bounds__(256) void traj_record_kernel(TrajRec r, TrajMaps x, TrajStep s, int32_t t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t lanes = r.D > r.W ? r.D : r.W;                                   // a thread per (env, word): one step's rows are contiguous in the step-major recording
    if (i >= (int64_t)r.M * lanes) return;
    traj_record_lane(r, x, s, t, (int32_t)(i / lanes), (int32_t)(i % lanes));
}
}  // namespace dril
namespace {
// the setup shared with the SAC handle (dril_traj_run.h) with what this handle alone knows: `discrete`, and ClampAdapter on the agent-facing Box (Box(-1, 1) under ScalingWrapperEnv)
int traj_prepare(dril_handle* h, const dril_traj_options* o, int32_t Tcap, TrajRun& r) {
    const size_t W = h->discrete ? 1 : (size_t)h->A;
    std::vector<float> clamp_low(W, 0.f), clamp_high(W, 0.f);
    TrajBoxes boxes = traj_env_boxes(h->env); boxes.discrete = h->discrete; boxes.clamp_low = clamp_low.data(); boxes.clamp_high = clamp_high.data();
    const EnvKindInfo* ki = env_kind_info(h->env.kind);
    if (!h->env.module && !ki) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_collect_trajectory_device: no device env on this handle");
    if (h->env.module) { if (!h->discrete) h->env.agent_action_space(clamp_low.data(), clamp_high.data()); }
    else if (ki->box) { clamp_low[0] = ki->act_lo; clamp_high[0] = ki->act_hi; }
    const TrajLayout L = traj_layout((size_t)o->n_trajectories, (size_t)h->D, W, (size_t)h->S, (size_t)Tcap);
    HIPCHK(h, traj_setup(h->env, h->stream, h->traj_blob, h->eval_counter, L, boxes, o->final_original != 0, /*drain_before_free=*/false, r));
    return DRIL_OK;
}
// one env step, enqueued: the launches of eval_step_granular, and over the M recorded envs only a state copy, the shadow step, the shadow observe and the recording
int traj_step(dril_handle* h, const TrajRun& r, int32_t t, int deterministic, int32_t* launches) {
    const int64_t g0 = h->gws.launches; const float* raw_rew = nullptr;
    HIPCHK(h, hipMemcpyAsync(r.shadow.state, h->env.state, (size_t)r.rec.M * h->S * 4, hipMemcpyDeviceToDevice, h->stream));   // the pre-step state of envs 0..M-1 (env-major prefix)
    { int rc = eval_step_policy(h, deterministic); if (rc) return rc; }
    HIPCHK(h, r.shadow.step(h->e_act, EnvStepOut{r.sh_rew, r.sh_term, r.sh_trunc, r.sh_tobs, nullptr}, MonitorArgs{}, h->stream));   // the same step, with no reset after it
    HIPCHK(h, r.shadow.observe(r.sh_obs, h->stream));                              // observe(env) of the env that did not auto-reset
    { int rc = eval_step_env(h, /*raw=*/true, &raw_rew); if (rc) return rc; }      // (the wrapper's statistics frozen; the recording takes the raw rewards)
    HIPCHK(h, traj_record_launch(traj_record_kernel, h->stream, r, TrajStep{h->e_act, raw_rew, h->e_term, h->e_trunc, r.sh_obs}, t));
    { int rc = eval_step_observe(h); if (rc) return rc; }                          // the next obs_to_agent (normalize_obs!, :24-26)
    *launches += eval_step_launches(h, g0) + 4 + (h->env.module ? 0 : 1);          // (a built-in shadow step + observe: env_step_kernel, env_observe_kernel)
    return DRIL_OK;
}
const char* const kTrajStillOpenMsg = "dril_collect_trajectory_device: a trajectory is still open after its capacity (internal)";   // (step Tcap finalises every open one)
// the persistent form: evaluate_modes_kernel in its recording mode, K env steps per launch.  No shadow envs, no state copies, none of the per-step arrays: the lane
// that holds env m < M records it from its registers.  The last launch is shortened so that no step past Tcap is ever enqueued
int traj_persistent_run(dril_handle* h, const dril_traj_options* o, const TrajRun& r, EvalPoll& p) {
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, h->eval_counter); if (rc) return rc; }
    EvalKernelArgs g{}; EvalModeArgs x{};
    eval_kernel_args(h, g, o->deterministic);                                      // (after the call's seed is in force)
    if (normalizing(h)) eval_mode_norm(h, x, true);                                // (no accounting while recording: the reward row is the raw reward)
    x.record = 1; x.rec = r.rec; x.maps = r.maps;
    const int K = eval_poll_steps(h, o->poll_steps, /*persistent=*/true, /*cap_events=*/false);
    return eval_poll_loop(h, r.rec.M, r.rec.Tcap, DRIL_ERR_HIP, kTrajStillOpenMsg, p, [&](long long& steps, int32_t& launches) -> int {
        g.step0 = (int32_t)steps; g.r.T = std::min(K, r.rec.Tcap - (int)steps);
        HIPCHK(h, launch_evaluate(h->env.kind, h->cfg.hidden1, g, h->stream, &x)); steps += g.r.T; launches += 1;
        return DRIL_OK;
    });
}
// path 2: a plug-in's evaluation kernel in its recording mode, K env steps per launch, and ONE launch of the per-trajectory rule over the rows it leaves.  The shadow
// envs are those of the step-granular form, stepped inside the kernel by the recorded env's own lane.  The last launch is shortened: no step past Tcap is ever enqueued
int traj_fused_run(dril_handle* h, const dril_traj_options* o, TrajRun& r, EvalPoll& p) {
    const int E = h->cfg.n_envs, M = r.rec.M, Tcap = r.rec.Tcap;
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, h->eval_counter, &r.shadow); if (rc) return rc; }
    const int K = eval_poll_steps(h, o->poll_steps, /*persistent=*/true, /*cap_events=*/true, /*cap_steps=*/Tcap);
    DrilEnvEvaluateArgs g{};
    { int rc = eval_fused_args(h, g, o->deterministic, K, M, &r.shadow); if (rc) return rc; }
    const int64_t n = (int64_t)M * std::max(r.rec.D, r.rec.W);
    return eval_poll_loop(h, M, Tcap, DRIL_ERR_HIP, kTrajStillOpenMsg, p, [&](long long& steps, int32_t& launches) -> int {
        g.r.T = std::min(K, Tcap - (int)steps);
        HIPCHK(h, h->env.launch_evaluate(g, h->stream));
        const TrajRows rows{g.r.T, E, g.r.rew, g.r.flags, g.rec_obs0, (const uint32_t*)g.rec_act, g.rec_obs};
        hipLaunchKernelGGL(traj_record_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, r.rec, r.maps, rows, (int32_t)steps);
        HIPCHK(h, hipGetLastError());
        steps += g.r.T; launches += 2;
        return DRIL_OK;
    });
}
// the step-granular form: traj_step per env step, a look at the finished-counter every K steps
int traj_stepwise_run(dril_handle* h, const dril_traj_options* o, TrajRun& r, EvalPoll& p) {
    { int rc = eval_open_episode(h, o->has_seed != 0, o->seed, h->eval_counter, &r.shadow); if (rc) return rc; }
    { int rc = eval_step_observe(h); if (rc) return rc; }                          // observation = observe(env), :17
    HIPCHK(h, traj_record_launch(traj_record_kernel, h->stream, r, TrajStep{nullptr, nullptr, nullptr, nullptr, eval_wrapped(h) ? h->e_obs_raw : h->e_obs}, 0));   // row 0: the original observation
    const int K = eval_poll_steps(h, o->poll_steps, /*persistent=*/false, /*cap_events=*/false);
    return eval_poll_loop(h, r.rec.M, r.rec.Tcap, DRIL_ERR_HIP, kTrajStillOpenMsg, p, [&](long long& steps, int32_t& launches) -> int {
        for (int k = 0; k < K && steps < r.rec.Tcap; ++k) { int rc = traj_step(h, r, (int32_t)(++steps), (o->deterministic ? 1 : 0), &launches); if (rc) return rc; }
        return DRIL_OK;
    });
}
int traj_device_run(dril_handle* h, const dril_traj_options* o, TrajRun& r, int path, float* observations, void* actions, float* rewards, int32_t* lengths, uint8_t* end_flags, dril_traj_info* info) {
    EvalPoll p;
    { int rc = path == 2 ? traj_fused_run(h, o, r, p) : path == 1 ? traj_persistent_run(h, o, r, p) : traj_stepwise_run(h, o, r, p); if (rc) return rc; }
    const TrajCopyOut c = traj_copy_out(h->stream, r.rec, observations, (uint32_t*)actions, rewards, lengths, end_flags);
    if (const std::string msg = traj_report("dril_collect_trajectory_device", c, r.rec.Tcap, (int32_t)p.steps, p.launches, path, info); !msg.empty()) return fail(h, DRIL_ERR_HIP, msg);
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_traj_options_default(dril_traj_options* o) {
    if (!o) return DRIL_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->n_trajectories = 1; o->deterministic = 1;                                       // trajectory_utils.jl:6-8
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_trajectory_capacity(const dril_handle* h, const dril_traj_options* o, int32_t* capacity) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!o || !capacity || o->max_steps < 0) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_trajectory_capacity: options and capacity != NULL, max_steps >= 0");
    if (h->external) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_trajectory_capacity: the envs of DRIL_ENV_EXTERNAL live on the host, with the caller");
    *capacity = traj_capacity(o->max_steps, h->env.episode_len);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_collect_trajectory_device(dril_handle* h, const dril_traj_options* o, float* observations, void* actions, float* rewards, int32_t* lengths,
                                                   uint8_t* end_flags, dril_traj_info* info) {
    NEED(h); NOT_EXTERNAL(h, "dril_collect_trajectory_device");
    if (const std::string msg = traj_options_error("dril_collect_trajectory_device", o, observations && actions && rewards && lengths && end_flags, h->cfg.n_envs); !msg.empty()) return fail(h, DRIL_ERR_INVALID_ARG, msg);
    if (h->env.is_world() && o->n_trajectories % h->env.agents() != 0)
        return fail(h, DRIL_ERR_INVALID_ARG, "dril_collect_trajectory_device: the env is a world of " + std::to_string(h->env.agents()) + " agents and whole worlds are recorded: n_trajectories " + std::to_string(o->n_trajectories) + " is not a multiple of " + std::to_string(h->env.agents()));
    int32_t Tcap = 0;
    if (const std::string msg = traj_size_error("dril_collect_trajectory_device", o, h->env.episode_len, h->D, h->discrete ? 1 : h->A, info, &Tcap); !msg.empty()) return fail(h, DRIL_ERR_INVALID_ARG, msg);
    { int rc = ensure_wimg(h); if (rc) return rc; }
    // the opt-in one-launch form where evaluate_modes_kernel applies; elsewhere (generic shapes, plug-ins, DRIL_FORCE_STEPWISE) the request falls back silently
    const bool persistent = o->reserved[DRIL_TRAJ_OPT_PERSISTENT] != 0 && eval_persistent_applies(h, true);
    const bool fused = eval_fused_applies(h, o->reserved[DRIL_TRAJ_OPT_PERSISTENT] != 0);   // path 2: the recording mode of a plug-in's own evaluation kernel (never both)
    EvalKeep keep; eval_keep_list(h, persistent || fused, keep);
    { int rc = eval_buffers(h, keep, 0); if (rc) return rc; }
    TrajRun run{};
    { int rc = traj_prepare(h, o, Tcap, run); if (rc) return rc; }
    // as dril_evaluate_agent_device: what training would continue from is set aside here and put back by eval_finish, on every path (set_training(env, false), :12)
    { int rc = eval_set_aside(h, keep); if (rc) return rc; }
    return eval_finish(h, keep, "dril_collect_trajectory_device", traj_device_run(h, o, run, fused ? 2 : persistent ? 1 : 0, observations, actions, rewards, lengths, end_flags, info));
}
