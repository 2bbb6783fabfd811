// dril_rollout.hip — collect_rollout of the PPO handle (dril_handle.h): the one-launch collection of the built-in kinds, the step-granular loops of wrapped envs and of
// device env plug-ins, a plug-in's fused collection, GAE, and the verbs that read and write the rollout buffer.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>

#include "dril_handle.h"

using namespace dril;
using namespace dril::ppo;

// ---- rollout ---------------------------------------------------------------------------------------
namespace {
// step-granular collect_trajectories (trajectory.jl:22-78) for wrapped envs: three launches per env step on the handle's stream
//   policy_kernel (+ V(terminal_observation) of the previous step) -> norm_step_kernel -> norm_apply_kernel
int collect_rollout_stepwise(dril_handle* h) {
    const int E = h->cfg.n_envs, T = h->cfg.n_steps, D = h->D, A = h->A;
    const size_t ab = act_bytes_per(h);
    int nb = (E + 255) / 256; if (nb > h->rms_blocks) nb = h->rms_blocks;
    int rc = observe_dev(h, true); if (rc) return rc;                                      // new_obs = observe(env), trajectory.jl:32
    for (int t = 0; t < T; ++t) {
        const size_t k = (size_t)t * E;
        const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * (size_t)A)) : nullptr;
        PolicyArgs p = policy_args(h, h->e_obs, E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);
        p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.obs_out = h->obs + k * D;
        if (t > 0) { p.boot_obs = h->e_tobs; p.boot_where = h->e_trunc; p.boot_out = h->boot + (k - E); }   // :57-61 for step t-1
        HIPCHK(h, run_policy(h, p));   // get_action_and_values, :41
        NormStepArgs s{};
        s.E = E; s.episode_len = h->env.episode_len; s.fixed_len = h->env.fixed_len; s.action_start = h->env.action_start;
        s.seed0 = h->env.seed0; s.gamma = h->cfg.norm_gamma; s.update_ret = (h->cfg.norm_reward && h->cfg.norm_training) ? 1 : 0;
        s.actions = (const char*)h->act + k * ab; s.state = h->env.state; s.step_count = h->env.step_count; s.episode = h->env.episode; s.gstep = h->env.gstep;
        s.disc_returns = h->env.disc_returns; s.rew_raw = h->e_rew; s.term = h->e_term; s.trunc = h->e_trunc; s.flags_out = h->flags + k;
        s.tobs_raw = h->e_tobs; s.obs_raw = h->e_obs_raw; s.partials = h->rms_partials;
        if (h->mon_cur_ret) { s.mon_cur_ret = h->mon_cur_ret; s.mon_cur_len = h->mon_cur_len; s.ep_ret = h->ep_ret + k; s.ep_len = h->ep_len + k; }
        HIPCHK(h, launch_norm_step(h->env.kind, s, nb, h->stream));                              // to_env + act!, :43-44
        NormApplyArgs ap{};
        ap.E = E; ap.D = D; ap.update_obs = (h->cfg.norm_obs && h->cfg.norm_training) ? 1 : 0; ap.update_ret = s.update_ret;
        ap.norm_obs = h->cfg.norm_obs; ap.norm_reward = h->cfg.norm_reward;
        int nba = nb;
        { int rcg = global_partials(h, ap.update_obs || ap.update_ret, ap.partials, nba, ap.n_stats); if (rcg) return rcg; }
        ap.nblocks = nba;
        ap.obs_in = h->obs_rms + h->obs_par; ap.obs_out = h->obs_rms + (h->obs_par ^ 1); ap.ret_in = h->ret_rms + h->ret_par; ap.ret_out = h->ret_rms + (h->ret_par ^ 1);
        ap.rew_raw = h->e_rew; ap.rew_out = h->rew + k; ap.disc_returns = h->env.disc_returns; ap.term = h->e_term; ap.trunc = h->e_trunc; ap.tobs = h->e_tobs;
        ap.obs_raw = h->e_obs_raw; ap.obs_n = h->e_obs; ap.clip_obs = h->cfg.clip_obs; ap.clip_reward = h->cfg.clip_reward; ap.eps = h->cfg.norm_epsilon;
        HIPCHK(h, launch_norm_apply(ap, h->stream));                                                 // new_obs = observe(env), :45
        h->obs_par ^= 1; h->ret_par ^= 1;
    }
    PolicyArgs l = policy_args(h, h->e_obs, E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);
    l.boot_obs = h->e_tobs; l.boot_where = h->e_trunc; l.boot_out = h->boot + (size_t)(T - 1) * E;
    HIPCHK(h, run_policy(h, l));       // V(new_obs) for rollout-limited tails, :65-70
    return monitor_collect_rollout(h);
}

// the same collection in ONE launch of rollout_norm_kernel (dril_norm_rollout_enable), after the opening observe(env) that the loop above starts with: it leaves env state,
// counters, disc_returns, the statistics' half in force, the per-step arrays, last_values and the monitor's sums as that loop leaves them
int collect_rollout_norm(dril_handle* h) {
    int rc = observe_dev(h, true); if (rc) return rc;                                      // new_obs = observe(env), trajectory.jl:32
    const NormRolloutArgs g = norm_rollout_args(h);
    HIPCHK(h, launch_rollout_norm(h->env.kind, g, h->stream));
    norm_rollout_done(h);
    return monitor_collect_rollout(h);
}

// step-granular collect_trajectories for a device env plug-in: two launch groups per env step,
//   policy (generic forward + sampling head, + V(terminal_observation) of the previous step) -> the plug-in's step kernel
// which writes reward and BUF_FLAGS byte straight into row t, the terminal observation and the next observation into the per-step arrays (one env launch where
// the built-in generic path has norm_step_kernel + norm_apply_kernel).  Noise: stream 1 at gstep, or the injected table, exactly as collect_rollout_stepwise.
int collect_rollout_module(dril_handle* h) {
    const int E = h->cfg.n_envs, T = h->cfg.n_steps, D = h->D, A = h->A;
    const size_t ab = act_bytes_per(h);
    h->rollout_launches += 1 + T;                                                                 // the opening observe and T step kernels; run_policy counts its own
    HIPCHK(h, h->env.observe(h->e_obs, h->stream));                                               // new_obs = observe(env), trajectory.jl:32
    for (int t = 0; t < T; ++t) {
        const size_t k = (size_t)t * E;
        const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * (size_t)A)) : nullptr;
        PolicyArgs p = policy_args(h, h->e_obs, E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);
        p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.obs_out = h->obs + k * D;
        if (t > 0) { p.boot_obs = h->e_tobs; p.boot_where = h->e_trunc; p.boot_out = h->boot + (k - E); }   // :57-61 for step t-1
        HIPCHK(h, run_policy(h, p));                                                       // get_action_and_values, :41
        HIPCHK(h, h->env.step((const char*)h->act + k * ab, EnvStepOut{h->rew + k, h->e_term, h->e_trunc, h->e_tobs, h->e_obs}, monitor_rollout_args(h, k), h->stream));   // to_env + act! + observe, :43-45
    }
    PolicyArgs l = policy_args(h, h->e_obs, E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);
    l.boot_obs = h->e_tobs; l.boot_where = h->e_trunc; l.boot_out = h->boot + (size_t)(T - 1) * E;
    HIPCHK(h, run_policy(h, l));                                                           // V(new_obs) for rollout-limited tails, :65-70
    return monitor_collect_rollout(h);
}

// the fused collection (dril_rollout_fused_enable): ONE launch of the plug-in's own rollout kernel (include/device/dril_env_rollout.h) does what the loop of
// collect_rollout_module does in 6+ launches per env step, and leaves env state, counters, monitor sums and the per-step arrays as that loop leaves them
int collect_rollout_module_fused(dril_handle* h) {
    const DrilEnvRolloutArgs g = module_rollout_args(h);
    h->rollout_launches += 1;
    HIPCHK(h, h->env.launch_rollout(g, h->stream));
    return monitor_collect_rollout(h);
}

void* buf_ptr(dril_handle* h, int which, size_t* bytes) {
    const size_t N = (size_t)h->N;
    switch (which) {
    case DRIL_BUF_OBSERVATIONS: *bytes = N * h->D * 4; return h->obs;
    case DRIL_BUF_ACTIONS: *bytes = N * act_bytes_per(h); return h->act;
    case DRIL_BUF_REWARDS: *bytes = N * 4; return h->rew;
    case DRIL_BUF_ADVANTAGES: *bytes = N * 4; return h->adv;
    case DRIL_BUF_RETURNS: *bytes = N * 4; return h->ret;
    case DRIL_BUF_LOGPROBS: *bytes = N * 4; return h->logp;
    case DRIL_BUF_VALUES: *bytes = N * 4; return h->val;
    case DRIL_BUF_FLAGS: *bytes = N; return h->flags;
    case DRIL_BUF_BOOTSTRAP: *bytes = N * 4; return h->boot;
    case DRIL_BUF_LAST_VALUES: *bytes = (size_t)h->cfg.n_envs * 4; return h->last_values;
    }
    *bytes = 0; return nullptr;
}
}  // namespace
namespace dril::ppo {
int compute_gae(dril_handle* h) {
    if (++h->gae_tag == 0) h->gae_tag = 1;                                            // 0 = "never written" (the carry words are zero at allocation)
    prof_begin(h, DRIL_K_GAE);
    HIPCHK(h, launch_gae(h->cfg.n_envs, h->cfg.n_steps, h->cfg.gamma, h->cfg.gae_lambda, h->rew, h->val, h->flags, h->boot, h->last_values,
                         h->adv, h->ret, h->gae_carry, h->gae_tag, h->gae_err, h->stream));
    prof_end(h);
    return DRIL_OK;
}
// "" when the handle's net fits the plug-in's fused evaluation kernel (path 2 of the evaluation / trajectory verbs), else why not
std::string fused_evaluate_unavailable(const dril_handle* h) {
    if (!h->env.module) return "the fused evaluation is a kernel of a device env plug-in (DRIL_ENV_MODULE): the built-in envs evaluate with the library's own evaluate_kernel, host envs (DRIL_ENV_EXTERNAL) step on the host";
    if (h->env.is_world()) return std::string("env plug-in \"") + h->env.desc.name + "\" is a world of " + std::to_string(h->env.agents()) + " agents: worlds have no fused evaluation yet (DRIL_ENV_PLUGIN_EVALUATE refuses a world at compile time); the evaluation and trajectory verbs run step-granular (path 0)";
    const EnvModuleEvaluate& r = h->env.evaluate;
    if (!r.reason.empty()) return std::string("env plug-in \"") + h->env.desc.name + "\": " + r.reason;
    const int W = r.desc.max_width;
    if (h->D > W) return "the observation has " + std::to_string(h->D) + " dims, the plug-in's fused evaluation was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->D) + " or more";
    for (int l = 0; l < h->gd.nh; ++l) if (h->gd.H[l] > W) return "hidden layer " + std::to_string(l + 1) + " is " + std::to_string(h->gd.H[l]) + " wide, the plug-in's fused evaluation was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->gd.H[l]) + " or more";
    if (h->env.scaling && !r.fn_scaled) return "ScalingWrapperEnv is on, but the code object has no dril_env_plugin_evaluate_scaled kernel: rebuild it with this library's include/device/dril_env_evaluate.h";
    return "";
}

// the argument block of the plug-in's fused rollout kernel, read from the handle as it stands (collect_rollout_module_fused, and a population for each of its members)
DrilEnvRolloutArgs module_rollout_args(const dril_handle* h) {
    DrilEnvRolloutArgs g{};
    g.env = h->env.args();
    g.env.terminated = h->e_term; g.env.truncated = h->e_trunc; g.env.terminal_obs = h->e_tobs; g.env.obs = h->e_obs;
    g.env.mon_cur_ret = h->mon_cur_ret; g.env.mon_cur_len = h->mon_cur_len;
    g.T = h->cfg.n_steps; g.n_hidden = h->gd.nh; g.activation = h->gd.act; g.n_params = h->P;
    for (int l = 0; l < h->gd.nh; ++l) g.hidden[l] = h->gd.H[l];
    g.actor_off = h->actor.w1; g.critic_off = h->critic.w1; g.log_std_off = h->log_std_off;
    g.params = h->params; g.noise = h->noise_set ? h->noise_dev : nullptr;
    g.obs = h->obs; g.act = h->act; g.rew = h->rew; g.logp = h->logp; g.val = h->val; g.boot = h->boot; g.flags = h->flags; g.last_values = h->last_values;
    if (h->mon_cur_ret) { g.ep_ret = h->ep_ret; g.ep_len = h->ep_len; }
    return g;
}
// "" when the handle's net fits the plug-in's fused rollout kernel, else why not
std::string fused_rollout_unavailable(const dril_handle* h) {
    if (!h->env.module) return "the fused rollout is the collection kernel of a device env plug-in (DRIL_ENV_MODULE): the built-in envs collect with the library's own rollout_kernel, host envs (DRIL_ENV_EXTERNAL) step on the host";
    if (h->env.is_world()) return std::string("env plug-in \"") + h->env.desc.name + "\" is a world of " + std::to_string(h->env.agents()) + " agents: worlds have no fused rollout yet (DRIL_ENV_PLUGIN_ROLLOUT refuses a world at compile time); collect step-granular, which is the default";
    const EnvModuleRollout& r = h->env.rollout;
    if (!r.reason.empty()) return std::string("env plug-in \"") + h->env.desc.name + "\": " + r.reason;
    const int W = r.desc.max_width;
    if (h->D > W) return "the observation has " + std::to_string(h->D) + " dims, the plug-in's fused rollout was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->D) + " or more";
    for (int l = 0; l < h->gd.nh; ++l) if (h->gd.H[l] > W) return "hidden layer " + std::to_string(l + 1) + " is " + std::to_string(h->gd.H[l]) + " wide, the plug-in's fused rollout was compiled for widths up to " + std::to_string(W) + ": rebuild it with -DDRIL_ENV_ROLLOUT_MAX_WIDTH=" + std::to_string(h->gd.H[l]) + " or more";
    if (h->env.scaling && !r.fn_scaled) return "ScalingWrapperEnv is on, but the code object has no dril_env_plugin_rollout_scaled kernel: rebuild it with this library's include/device/dril_env_rollout.h";
    return "";
}

// a collection that is ONE launch of the fused rollout kernel of a built-in kind (generic nets have no fused rollout kernel, wrapped envs step through the wrapper's kernels)
bool rollout_fused_applies(const dril_handle* h) { return !(normalizing(h) || h->force_stepwise || h->generic); }
// the argument block of that launch, read from the handle as it stands (collect_rollout, and a population for each of its members)
RolloutArgs rollout_args(const dril_handle* h) {
    RolloutArgs a{};
    a.params = h->params; a.state = h->env.state; a.step_count = h->env.step_count; a.episode = h->env.episode; a.gstep = h->env.gstep;
    a.obs = h->obs; a.act = h->act; a.rew = h->rew; a.logp = h->logp; a.val = h->val; a.boot = h->boot; a.flags = h->flags; a.last_values = h->last_values;
    a.noise = h->noise_set ? h->noise_dev : nullptr;
    a.E = h->env.E; a.T = h->cfg.n_steps; a.episode_len = h->env.episode_len; a.fixed_len = h->env.fixed_len;
    a.action_start = h->env.action_start; a.log_std_off = h->log_std_off; a.env_seed0 = h->env.seed0; a.actor = h->actor; a.critic = h->critic;
    a.exact_f32 = fwd_exact(h) ? 1 : 0;
    a.w2a_actor = a.exact_f32 ? h->w2a_actor : (const float*)h->w2pf_actor.get(); a.w2a_critic = a.exact_f32 ? h->w2a_critic : (const float*)h->w2pf_critic.get();
    a.mon_cur_ret = h->mon_cur_ret; a.mon_cur_len = h->mon_cur_len; a.ep_ret = h->ep_ret; a.ep_len = h->ep_len;
    return a;
}
std::string norm_rollout_unavailable(const dril_handle* h) {
    if (h->env.module) return "the handle steps a device env plug-in (DRIL_ENV_MODULE): its NormalizeWrapperEnv is dril_normalize_enable and its one-launch collection dril_rollout_fused_enable; this verb is for the built-in env kinds";
    if (h->external) return "the envs of a DRIL_ENV_EXTERNAL handle are the caller's: its NormalizeWrapperEnv is dril_ext_normalize_enable and its collection the dril_ext_* verbs; this verb is for the built-in env kinds";
    if (!normalizing(h)) return "the handle has no NormalizeWrapperEnv (cfg.norm_obs = cfg.norm_reward = 0): its collection already is one launch of the rollout kernel; create it with norm_obs and / or norm_reward";
    if (h->generic) return "the handle runs the generic layer-by-layer kernels (hidden_dims other than two equal tanh layers of 32 / 64 / 128 / 256, or DRIL_FORCE_GENERIC): rollout_norm_kernel is built for hidden_dims [64,64]; collect step-granular, which is the default";
    if (h->wide || h->cfg.hidden1 != 64) return "hidden_dims [" + std::to_string(h->cfg.hidden1) + "," + std::to_string(h->cfg.hidden2) + "]: rollout_norm_kernel is built for hidden_dims [64,64] alone; collect step-granular, which is the default";
    if (h->cfg.n_envs > kNormRolloutMaxEnvs) return "n_envs = " + std::to_string(h->cfg.n_envs) + ": one workgroup couples at most " + std::to_string(kNormRolloutMaxEnvs) + " envs through LDS; use n_envs <= " + std::to_string(kNormRolloutMaxEnvs) + ", or collect step-granular, which is the default";
    if (h->cfg.world_size > 1 || comm_ready(h)) return "the handle is part of a data-parallel job (world_size > 1 or a ready communicator): its batch moments are an all-reduce per env step, which one launch cannot hold; collect step-granular, which is the default";
    if (h->force_stepwise) return "DRIL_FORCE_STEPWISE is set: every collection of this handle runs the step-granular launches; unset it and create the handle again";
    return "";
}
bool norm_rollout_applies(const dril_handle* h) { return h->norm_rollout && !fwd_exact(h) && norm_rollout_unavailable(h).empty(); }
NormRolloutArgs norm_rollout_args(const dril_handle* h) {
    NormRolloutArgs g{};
    g.r = rollout_args(h);
    g.disc_returns = h->env.disc_returns; g.obs_rms = h->obs_rms; g.ret_rms = h->ret_rms; g.obs_par = h->obs_par; g.ret_par = h->ret_par;
    g.update_obs = (h->cfg.norm_obs && h->cfg.norm_training) ? 1 : 0; g.update_ret = (h->cfg.norm_reward && h->cfg.norm_training) ? 1 : 0;
    g.norm_obs = h->cfg.norm_obs; g.norm_reward = h->cfg.norm_reward;
    g.gamma = h->cfg.norm_gamma; g.clip_obs = h->cfg.clip_obs; g.clip_reward = h->cfg.clip_reward; g.eps = h->cfg.norm_epsilon;
    g.e_obs = h->e_obs; g.e_obs_raw = h->e_obs_raw; g.e_rew = h->e_rew; g.e_term = h->e_term; g.e_trunc = h->e_trunc; g.e_tobs = h->e_tobs;
    return g;
}
// the kernel flipped both ping-pong pairs once per env step, as the loop's host does
void norm_rollout_done(dril_handle* h) {
    h->obs_par ^= h->cfg.n_steps & 1; h->ret_par ^= h->cfg.n_steps & 1;
    h->norm_rollout_path = 1; h->norm_rollout_launches = 3 + (h->mon_cur_ret ? 2 : 0);     // observe (2), the kernel, the monitor's window (2)
}
int collect_rollout(dril_handle* h, double* fps, bool do_sync) {
    if (!h->env.ready) return fail(h, DRIL_ERR_NOT_INITIALISED, "dril_collect_rollout before dril_env_reset");
    { int rcw = ensure_wimg(h); if (rcw) return rcw; }
    if (!rollout_fused_applies(h)) {                                    // step-granular launches
        const auto t0s = std::chrono::steady_clock::now();
        if (fps) HIPCHK(h, hipStreamSynchronize(h->stream));
        prof_begin(h, DRIL_K_ROLLOUT);
        h->rollout_launches = 0; h->gws.launches = 0;
        if (h->fused_rollout) { const std::string why = fused_rollout_unavailable(h); if (!why.empty()) { prof_end(h); return fail(h, DRIL_ERR_UNSUPPORTED, "dril_collect_rollout with the fused rollout on: " + why); } }
        const bool one_launch = !h->env.module && norm_rollout_applies(h);
        int rcs = h->env.module ? (h->fused_rollout ? collect_rollout_module_fused(h) : h->pn.on ? collect_rollout_module_norm(h) : collect_rollout_module(h))
                                : one_launch ? collect_rollout_norm(h) : collect_rollout_stepwise(h);
        h->rollout_launches += h->gws.launches + (h->mon_cur_ret ? 1 : 0);
        if (!h->env.module && !h->generic && normalizing(h)) {           // what dril_norm_rollout_info reports: observe (2), the kernel or 3 per env step + the last values, the monitor's window (2)
            h->norm_rollout_path = one_launch ? 1 : 0;
            h->norm_rollout_launches = 2 + (one_launch ? 1 : 3 * (int64_t)h->cfg.n_steps + 1) + (h->mon_cur_ret ? 2 : 0);
            if (h->norm_rollout && !one_launch && fwd_exact(h)) h->norm_rollout_fallbacks += 1;
        }
        prof_end(h);
        if (rcs) return rcs;
        if (fps) { HIPCHK(h, hipStreamSynchronize(h->stream)); const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0s).count(); *fps = (double)h->N / (dt > 0 ? dt : 1e-12); }
        h->noise_set = false;
        rcs = compute_gae(h); if (rcs) return rcs;
        return do_sync ? sync(h) : DRIL_OK;
    }
    const RolloutArgs a = rollout_args(h);
    const auto t0 = std::chrono::steady_clock::now();
    if (fps) HIPCHK(h, hipStreamSynchronize(h->stream));
    prof_begin(h, DRIL_K_ROLLOUT);
    HIPCHK(h, launch_rollout(h->env.kind, h->cfg.hidden1, a, h->stream));
    prof_end(h);
    if (fps) {   // fps = steps / wall time of collect_trajectories, rollout_buffer.jl:60-64
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *fps = (double)h->N / (dt > 0 ? dt : 1e-12);
    }
    h->noise_set = false;
    { int rcm = monitor_collect_rollout(h); if (rcm) return rcm; }
    int rc = compute_gae(h); if (rc) return rc;
    return do_sync ? sync(h) : DRIL_OK;
}
}  // namespace dril::ppo
DRIL_EXPORT int32_t dril_rollout_fused_enable(dril_handle* h, int32_t on) {
    NEED(h);
    if (on) {
        std::string why = fused_rollout_unavailable(h);
        if (why.empty() && h->pn.on) why = "NormalizeWrapperEnv is on (dril_normalize_enable): its running statistics couple all envs at every step, which is what a workgroup per tile of envs gives up; collect step-granular, or switch the wrapper off with dril_normalize_enable(h, NULL) first";
        if (!why.empty()) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_rollout_fused_enable: " + why);
    }
    h->fused_rollout = on != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_rollout_fused_info(const dril_handle* h, dril_fused_rollout_info* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_rollout_fused_info: null out pointer");
    std::memset(out, 0, sizeof(*out));
    const std::string why = fused_rollout_unavailable(h);
    out->available = why.empty() ? 1 : 0; out->enabled = h->fused_rollout ? 1 : 0; out->last_collection_launches = h->rollout_launches;
    if (h->env.module && h->env.rollout.has_desc) { out->tile = h->env.rollout.desc.tile; out->threads = h->env.rollout.desc.threads; out->max_width = h->env.rollout.desc.max_width; }
    std::snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_norm_rollout_enable(dril_handle* h, int32_t on) {
    NEED(h);
    if (on) { const std::string why = norm_rollout_unavailable(h); if (!why.empty()) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_norm_rollout_enable: " + why); }
    h->norm_rollout = on != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_norm_rollout_info(const dril_handle* h, dril_norm_rollout_report* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_norm_rollout_info: null out pointer");
    std::memset(out, 0, sizeof(*out));
    const std::string why = norm_rollout_unavailable(h);
    out->available = why.empty() ? 1 : 0; out->enabled = h->norm_rollout ? 1 : 0; out->max_envs = kNormRolloutMaxEnvs;
    out->last_collection_path = h->norm_rollout_path; out->last_collection_launches = h->norm_rollout_launches; out->total_stepwise_fallbacks = h->norm_rollout_fallbacks;
    std::snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_evaluate_fused_info(const dril_handle* h, dril_fused_evaluate_info* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return fail(const_cast<dril_handle*>(h), DRIL_ERR_INVALID_ARG, "dril_evaluate_fused_info: null out pointer");
    std::memset(out, 0, sizeof(*out));
    const std::string why = fused_evaluate_unavailable(h);
    out->available = why.empty() ? 1 : 0;
    if (h->env.module && h->env.evaluate.has_desc) { out->tile = h->env.evaluate.desc.tile; out->threads = h->env.evaluate.desc.threads; out->max_width = h->env.evaluate.desc.max_width; }
    std::snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_collect_rollout(dril_handle* h, double* fps) { NEED(h); NOT_EXTERNAL(h, "dril_collect_rollout"); return collect_rollout(h, fps, true); }
DRIL_EXPORT int32_t dril_debug_set_noise(dril_handle* h, const void* noise, size_t count) {
    NEED(h);
    if (!noise) { h->noise_set = false; return DRIL_OK; }
    const size_t need = (size_t)h->N * (h->discrete ? 1 : (size_t)h->A);
    if (count != need) return fail(h, DRIL_ERR_INVALID_ARG, "dril_debug_set_noise: count must be n_envs*n_steps (*action_dim)");
    const size_t bytes = need * (h->discrete ? 8 : 4);
    if (!h->noise_dev) HIPCHK(h, h->noise_dev.alloc(bytes));
    HIPCHK(h, hipMemcpyAsync(h->noise_dev, noise, bytes, hipMemcpyHostToDevice, h->stream));
    h->noise_set = true;
    return sync(h);
}
DRIL_EXPORT int32_t dril_buffer_copy_out(dril_handle* h, int32_t which, void* host, size_t bytes) {
    NEED(h); size_t b; void* p = buf_ptr(h, which, &b);
    if (!p || !host || b != bytes) return fail(h, DRIL_ERR_INVALID_ARG, "dril_buffer_copy_out: bad id or byte count");
    HIPCHK(h, hipMemcpyAsync(host, p, b, hipMemcpyDeviceToHost, h->stream)); return sync(h);
}
DRIL_EXPORT int32_t dril_buffer_copy_in(dril_handle* h, int32_t which, const void* host, size_t bytes) {
    NEED(h); size_t b; void* p = buf_ptr(h, which, &b);
    if (!p || !host || b != bytes) return fail(h, DRIL_ERR_INVALID_ARG, "dril_buffer_copy_in: bad id or byte count");
    HIPCHK(h, hipMemcpyAsync(p, host, b, hipMemcpyHostToDevice, h->stream)); return sync(h);
}
DRIL_EXPORT int32_t dril_compute_gae(dril_handle* h) {
    NEED(h); int rc = compute_gae(h); if (rc) return rc;
    int gave_up = 0; HIPCHK(h, hipMemcpyAsync(&gave_up, h->gae_err, 4, hipMemcpyDeviceToHost, h->stream));
    rc = sync(h); if (rc) return rc;
    if (gave_up) { (void)hipMemsetAsync(h->gae_err, 0, 4, h->stream); return fail(h, DRIL_ERR_HIP, "gae_scan_kernel: a chunk's predecessor did not publish its carry within the spin limit"); }
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_gae(int32_t E, int32_t T, float gamma, float lam, const float* rewards, const float* values, const uint8_t* flags,
                             const float* bootstrap, const float* last_values, float* advantages, float* returns) {
    if (E < 1 || T < 1 || !rewards || !values || !flags || !bootstrap || !last_values || !advantages || !returns)
        return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_gae: bad argument");
    const size_t N = (size_t)E * T;
    DevBuf<float> d_r, d_v, d_b, d_l, d_a, d_ret; DevBuf<uint8_t> d_f; DevBuf<unsigned long long> d_c; DevBuf<int> d_e;
    HIPCHK(nullptr, d_r.alloc(N)); HIPCHK(nullptr, d_v.alloc(N)); HIPCHK(nullptr, d_b.alloc(N)); HIPCHK(nullptr, d_l.alloc((size_t)E)); HIPCHK(nullptr, d_a.alloc(N)); HIPCHK(nullptr, d_ret.alloc(N)); HIPCHK(nullptr, d_f.alloc(N));
    HIPCHK(nullptr, hipMemcpy(d_r, rewards, N * 4, hipMemcpyHostToDevice)); HIPCHK(nullptr, hipMemcpy(d_v, values, N * 4, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_b, bootstrap, N * 4, hipMemcpyHostToDevice)); HIPCHK(nullptr, hipMemcpy(d_l, last_values, (size_t)E * 4, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_f, flags, N, hipMemcpyHostToDevice));
    const size_t words = (size_t)gae_chunks(T) * E; int gave_up = 0;
    HIPCHK(nullptr, d_c.alloc(words)); HIPCHK(nullptr, hipMemset(d_c, 0, words * 8)); HIPCHK(nullptr, d_e.alloc(1)); HIPCHK(nullptr, hipMemset(d_e, 0, 4));
    HIPCHK(nullptr, launch_gae(E, T, gamma, lam, d_r, d_v, d_f, d_b, d_l, d_a, d_ret, d_c, 1u, d_e, nullptr));
    HIPCHK(nullptr, hipDeviceSynchronize());
    HIPCHK(nullptr, hipMemcpy(&gave_up, d_e, 4, hipMemcpyDeviceToHost));
    if (gave_up) return fail(nullptr, DRIL_ERR_HIP, "gae_scan_kernel: a chunk's predecessor did not publish its carry within the spin limit");
    HIPCHK(nullptr, hipMemcpy(advantages, d_a, N * 4, hipMemcpyDeviceToHost)); HIPCHK(nullptr, hipMemcpy(returns, d_ret, N * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
