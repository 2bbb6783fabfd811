// dril_api.hip — the C ABI of libdril_hip.so (include/dril_hip.h): handle, device memory, launch sequencing.
// One HIP stream per handle; kernels of one PPO iteration are enqueued back-to-back with no host sync
// (KL early-stop and NaN detection are device flags the later kernels test), RCCL all-reduces ride the
// same stream.  This unit: create / destroy, the parameter, optimiser-state, env and policy verbs, dril_train, profiling and info, and the helpers every unit launches
// through.  The handle itself, the other units of its host code and what crosses between them: dril_handle.h.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dril_handle.h"

#include "dril_policy_internal.h"   // dril_policy_from_handle: the snapshot this handle gives a deployment policy (dril_policy.hip)

using namespace dril;
using namespace dril::ppo;

namespace {

// cfg.profile_events = k >= 1: the per-iteration classes (rollout, GAE, pack, moments, explained variance) are bracketed at every launch; the classes launched once per
// OPTIMISER STEP (gradient, reduce, Adam, all-reduce) at every k-th launch — a hipEventRecord costs the stream ~3.5 us and an iteration of configs[1] holds 960 such launches
// (measured round 4, same box: 350.4 / 346.9 ms with all of them bracketed, 343.7 / 343.3 with none / every 8th; hipEventDisableSystemFence changes nothing)
bool prof_per_step(int kid) { return kid == DRIL_K_PPO_GRAD || kid == DRIL_K_GRAD_REDUCE || kid == DRIL_K_ADAM || kid == DRIL_K_ALLREDUCE; }

// ---- MonitorWrapperEnv helpers ----
MonitorArgs monitor_step_args(dril_handle* h) {   // one env step: finished episodes land in the E-sized step arrays
    MonitorArgs m{}; if (h->mon_cur_ret) { m.cur_ret = h->mon_cur_ret; m.cur_len = h->mon_cur_len; m.ep_ret = h->e_ep_ret; m.ep_len = h->e_ep_len; m.flags_out = h->e_flags; }
    return m;
}
int monitor_collect_step(dril_handle* h) {
    if (!h->mon_cur_ret) return DRIL_OK;
    HIPCHK(h, launch_monitor_collect(h->e_flags, h->e_ep_ret, h->e_ep_len, h->cfg.n_envs, 1, h->cfg.monitor_window, h->mon_cnt, h->mon_ring_ret, h->mon_ring_len, h->mon_meta, h->stream));
    return DRIL_OK;
}
}  // namespace

namespace dril::ppo {
// ---- what the other units call (dril_handle.h) ----
thread_local std::string g_create_error;

void prof_resolve(dril_handle* h) {   // stream must be drained
    for (auto& p : h->prof_pending) {
        float ms = 0; if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { h->prof_ms[p.kid] += ms; h->prof_n[p.kid] += 1; }
        h->prof_pool.push_back({p.a, p.b});
    }
    h->prof_pending.clear();
}
void prof_begin(dril_handle* h, int kid) {
    h->prof_open = false;
    if (!h->cfg.profile_events) return;
    const int64_t i = h->prof_all[kid]++;
    if (prof_per_step(kid) && h->cfg.profile_events > 1 && i % h->cfg.profile_events) return;
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (!h->prof_pool.empty()) { ev = h->prof_pool.back(); h->prof_pool.pop_back(); }
    else { hipEventCreate(&ev.first); hipEventCreate(&ev.second); }
    hipEventRecord(ev.first, h->stream);
    h->prof_pending.push_back({kid, ev.first, ev.second});
    h->prof_open = true;
}
void prof_end(dril_handle* h) {
    if (!h->prof_open) return;
    hipEventRecord(h->prof_pending.back().b, h->stream);
    h->prof_open = false;
}
int sync(dril_handle* h) { HIPCHK(h, hipStreamSynchronize(h->stream)); prof_resolve(h); return DRIL_OK; }

// wide nets: (re)build the pre-tiled W2 / W2' images after every parameter change (enqueued on the handle's stream)
int ensure_wimg(dril_handle* h) {
    if (!h->wide || !h->wimg_dirty) return DRIL_OK;
    HIPCHK(h, launch_build_wimg(h->params, h->actor, h->cfg.hidden1, h->w2a_actor, h->w2ta_actor, h->stream));
    HIPCHK(h, launch_build_wimg(h->params, h->critic, h->cfg.hidden1, h->w2a_critic, h->w2ta_critic, h->stream));
    {                                             // the pre-split f16 fragment streams: ppo_grad_wide_split_kernel, and the forward of rollout / policy kernels
        HIPCHK(h, launch_build_wimg_split(h->params, h->actor, h->cfg.hidden1, h->w2p_actor, h->w2tp_actor, h->w2pf_actor, h->stream));
        HIPCHK(h, launch_build_wimg_split(h->params, h->critic, h->cfg.hidden1, h->w2p_critic, h->w2tp_critic, h->w2pf_critic, h->stream));
    }
    h->wimg_dirty = false;
    return DRIL_OK;
}

// fused per-kind kernels for the device envs, the layer-by-layer generic path for DRIL_ENV_EXTERNAL
hipError_t run_policy(dril_handle* h, const PolicyArgs& a) {
    if (!h->generic) return launch_policy(h->cfg.env_kind, h->cfg.hidden1, a, 8 * h->num_cus, h->stream);
    if (a.boot_where) {                       // V(terminal_observation) of the previous env step (fused into policy_kernel on the fused path): critic over all rows, kept where truncated
        PolicyArgs b = a; b.obs = a.boot_obs; b.noise = nullptr; b.actions = nullptr; b.values = h->gen_tmp; b.logp = nullptr; b.entropy = nullptr; b.mode = 2;
        b.obs_out = nullptr; b.boot_obs = nullptr; b.boot_where = nullptr; b.boot_out = nullptr; b.gstep = nullptr;
        hipError_t e = generic_policy(h->gd, b, h->gws, h->stream); if (e != hipSuccess) return e;
        e = generic_select(a.B, a.boot_where, h->gen_tmp, a.boot_out, h->stream); if (e != hipSuccess) return e;
        h->gws.launches += 1;
    }
    PolicyArgs q = a; q.boot_obs = nullptr; q.boot_where = nullptr; q.boot_out = nullptr;
    return generic_policy(h->gd, q, h->gws, h->stream);
}

PolicyArgs policy_args(dril_handle* h, const float* obs, int64_t B, const void* noise, void* actions, float* values, float* logp,
                       float* entropy, int mode) {
    PolicyArgs a{};
    a.params = h->params; a.obs = obs; a.B = B; a.noise = noise; a.actions = actions; a.values = values; a.logp = logp; a.entropy = entropy;
    a.mode = mode; a.action_start = h->cfg.action_start; a.log_std_off = h->log_std_off; a.seed = h->cfg.seed; a.call_counter = h->policy_calls;
    a.actor = h->actor; a.critic = h->critic;
    a.exact_f32 = fwd_exact(h) ? 1 : 0;
    a.w2a_actor = a.exact_f32 ? h->w2a_actor : (const float*)h->w2pf_actor.get(); a.w2a_critic = a.exact_f32 ? h->w2a_critic : (const float*)h->w2pf_critic.get();   // wide nets: W2 operand of the forward
    return a;
}

MonitorArgs monitor_rollout_args(dril_handle* h, size_t k) {   // row k / E of a step-granular rollout over a plug-in: the BUF_FLAGS byte always, finished episodes with the monitor on
    MonitorArgs m{}; m.flags_out = h->flags + k; if (h->mon_cur_ret) { m.cur_ret = h->mon_cur_ret; m.cur_len = h->mon_cur_len; m.ep_ret = h->ep_ret + k; m.ep_len = h->ep_len + k; }
    return m;
}
int monitor_collect_rollout(dril_handle* h) {
    if (!h->mon_cur_ret) return DRIL_OK;
    HIPCHK(h, launch_monitor_collect(h->flags, h->ep_ret, h->ep_len, h->cfg.n_envs, h->cfg.n_steps, h->cfg.monitor_window, h->mon_cnt, h->mon_ring_ret, h->mon_ring_len, h->mon_meta, h->stream));
    return DRIL_OK;
}

// act!(env, actions) through the E-sized per-step arrays (dril_env_step, dril_evaluate_agent, the step-granular verbs), and MonitorWrapperEnv's window after it
int env_step_arrays(dril_handle* h, const void* actions) {
    HIPCHK(h, h->env.step(actions, EnvStepOut{h->e_rew, h->e_term, h->e_trunc, h->e_tobs, nullptr}, monitor_step_args(h), h->stream));
    return monitor_collect_step(h);
}

// data-parallel runs: NormalizeWrapperEnv's batch moments cover every env of the job (the reference has ONE vector env, normalizeWrapperEnv.jl:21-26):
// this rank's partial table is folded to one row, RCCL sums the rows, and the apply kernels merge that row with n_stats = world * E.  One 128-byte
// all-reduce per env step; every rank applies the identical update, so the running statistics stay bit-identical across ranks
int global_partials(dril_handle* h, bool update, const double*& partials, int& nb, long long& n_stats) {
    partials = h->rms_partials; n_stats = 0;
    const int world = comm_ready(h) ? h->cfg.world_size : 1;
    if (!update || !(world > 1 || (comm_ready(h) && h->force_allreduce))) return DRIL_OK;
    HIPCHK(h, launch_fold_partials(h->rms_partials, nb, h->rms_red, h->stream));
    int rc = rccl_allreduce(h, h->rms_red, 16, kNcclFloat64); if (rc) return rc;
    partials = h->rms_red; nb = 1; n_stats = (long long)h->cfg.n_envs * world;
    return DRIL_OK;
}

// ---- step-granular env verbs on device (NormalizeWrapperEnv.observe / act!, normalizeWrapperEnv.jl:123-165) ----
int observe_dev(dril_handle* h, bool update_stats) {
    const int E = h->cfg.n_envs;
    if (h->env.module && h->pn.on) return pn_observe(h, update_stats);                 // a plug-in env under dril_normalize_enable
    if (h->env.module) { HIPCHK(h, h->env.observe(h->e_obs, h->stream)); return DRIL_OK; }   // a plug-in env without the wrapper: the observation as it is
    int nb = (E + 255) / 256; if (nb > h->rms_blocks) nb = h->rms_blocks;
    HIPCHK(h, launch_obs_partials(h->env.kind, E, h->env.state, h->e_obs_raw, h->rms_partials, nb, h->stream));
    NormObsArgs a{};
    a.E = E; a.D = h->D; a.update = (update_stats && h->cfg.norm_training && h->cfg.norm_obs) ? 1 : 0;
    { int rcg = global_partials(h, a.update != 0, a.partials, nb, a.n_stats); if (rcg) return rcg; }
    a.nblocks = nb;
    a.raw = h->e_obs_raw; a.in = h->obs_rms + h->obs_par; a.out = h->obs_rms + (h->obs_par ^ 1);
    a.obs_n = h->e_obs; a.clip = h->cfg.clip_obs; a.eps = h->cfg.norm_epsilon; a.norm_obs = h->cfg.norm_obs;
    HIPCHK(h, launch_norm_obs_apply(a, h->stream));
    h->obs_par ^= 1;
    return DRIL_OK;
}
// actions: device pointer (stored/raw policy actions; the kernels apply the adapters); rew_out/flags_out: device destinations
int step_dev(dril_handle* h, const void* actions, float* rew_out, uint8_t* flags_out) {
    const int E = h->cfg.n_envs;
    if (h->env.module && h->pn.on) return pn_step(h, actions, rew_out ? rew_out : h->e_rew_n);
    { int rcs = env_step_arrays(h, actions); if (rcs) return rcs; }
    if (h->env.module) {                                                               // plug-in env without the wrapper: the raw step is the whole step
        if (rew_out && rew_out != h->e_rew) HIPCHK(h, hipMemcpyAsync(rew_out, h->e_rew, (size_t)E * 4, hipMemcpyDeviceToDevice, h->stream));
        return DRIL_OK;
    }
    int nb = (E + 255) / 256; if (nb > h->rms_blocks) nb = h->rms_blocks;
    const int upd = (h->cfg.norm_reward && h->cfg.norm_training) ? 1 : 0;
    HIPCHK(h, launch_rew_partials(E, h->e_rew, h->env.disc_returns, h->cfg.norm_gamma, upd, h->rms_partials, nb, h->stream));
    NormRewArgs a{};
    a.E = E; a.D = h->D; a.update = upd; a.norm_obs = h->cfg.norm_obs; a.norm_reward = h->cfg.norm_reward;
    { int rcg = global_partials(h, upd != 0, a.partials, nb, a.n_stats); if (rcg) return rcg; }
    a.nblocks = nb;
    a.rew_raw = h->e_rew; a.in = h->ret_rms + h->ret_par; a.out = h->ret_rms + (h->ret_par ^ 1);
    a.obs_stats = h->obs_rms + h->obs_par; a.rew_out = rew_out; a.disc_returns = h->env.disc_returns; a.term = h->e_term; a.trunc = h->e_trunc;
    a.tobs = h->e_tobs; a.clip_obs = h->cfg.clip_obs; a.clip_reward = h->cfg.clip_reward; a.eps = h->cfg.norm_epsilon; a.flags_out = flags_out;
    HIPCHK(h, launch_norm_rew_apply(a, h->stream));
    h->ret_par ^= 1;
    return DRIL_OK;
}
}  // namespace dril::ppo

namespace {
int reset_optimizer(dril_handle* h) {
    HIPCHK(h, hipMemsetAsync(h->adam_m, 0, sizeof(float) * h->P, h->stream));
    HIPCHK(h, hipMemsetAsync(h->adam_v, 0, sizeof(float) * h->P, h->stream));
    const float bt[4] = {h->cfg.adam_beta1, h->cfg.adam_beta2, h->cfg.adam_beta1, h->cfg.adam_beta2};
    HIPCHK(h, hipMemcpyAsync(h->bt, bt, sizeof(bt), hipMemcpyHostToDevice, h->stream));
    h->adam_steps = 0;
    return sync(h);
}
}  // namespace

// ================================================================================================
DRIL_EXPORT int32_t dril_config_default(dril_config* c, int32_t env_kind) {
    if (!c || env_kind < DRIL_ENV_CARTPOLE || env_kind > DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "bad cfg/env_kind");
    std::memset(c, 0, sizeof(*c));
    c->abi_version = DRIL_ABI_VERSION; c->env_kind = env_kind; c->n_envs = 4; c->n_steps = 2048; c->hidden1 = c->hidden2 = 64;
    const EnvKindInfo* k = env_kind_info(env_kind);
    c->episode_len = k ? k->default_episode_len /* the Gymnasium time limit */ : env_kind == DRIL_ENV_MODULE ? 0 /* the descriptor's */ : 200; c->action_start = 1;
    c->gamma = 0.99f; c->gae_lambda = 0.95f; c->clip_range = 0.2f; c->ent_coef = 0.0f; c->vf_coef = 0.5f;
    c->max_grad_norm = 0.5f; c->has_max_grad_norm = 1; c->normalize_advantage = 1; c->batch_size = 64; c->epochs = 10;
    c->learning_rate = 3.0e-4f; c->adam_beta1 = 0.9f; c->adam_beta2 = 0.999f; c->adam_eps = 1.0e-5f;
    c->clip_obs = c->clip_reward = 10.0f; c->norm_gamma = 0.99f; c->norm_epsilon = 1.0e-8f; c->seed = 42; c->world_size = 1;
    return DRIL_OK;
}

DRIL_EXPORT int32_t dril_env_module_describe(const char* code_object_path, int32_t device, dril_env_module_info* out) {
    if (!out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_env_module_describe: null out");
    hipModule_t mod = nullptr; DrilEnvPluginDesc d{}; std::string msg;
    const int rc = load_env_module(code_object_path, device, &mod, &d, msg);
    if (rc) return fail(nullptr, rc, "dril_env_module_describe: " + msg);
    (void)hipModuleUnload(mod);
    fill_module_info(d, out);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_info_of(const dril_handle* h, dril_env_module_info* out) {
    if (!h || !out) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle / out");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_env_module_info_of: the handle was not created with dril_create_with_env_module");
    fill_module_info(h->env.desc, out);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_obs_space(const char* code_object_path, int32_t device, float* low, float* high, int32_t* declared) {
    std::string msg; const int rc = describe_module_obs_space(code_object_path, device, low, high, declared, msg);
    return rc ? fail(nullptr, rc, "dril_env_module_obs_space: " + msg) : DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_obs_space_of(const dril_handle* h, float* low, float* high, int32_t* declared) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_env_module_obs_space_of: the handle was not created with dril_create_with_env_module");
    const int D = h->env.desc.D;
    if (low) std::memcpy(low, h->env.obs_low.data(), (size_t)D * 4);
    if (high) std::memcpy(high, h->env.obs_high.data(), (size_t)D * 4);
    if (declared) *declared = h->env.obs_declared ? 1 : 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_agents(const char* code_object_path, int32_t device, int32_t* agents) {
    if (!agents) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_env_module_agents: null agents");
    hipModule_t mod = nullptr; DrilEnvPluginDesc d{}; std::string msg;
    const int rc = load_env_module(code_object_path, device, &mod, &d, msg);
    if (rc) return fail(nullptr, rc, "dril_env_module_agents: " + msg);
    (void)hipModuleUnload(mod);
    *agents = d.agents ? d.agents : 1;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_env_module_agents_of(const dril_handle* h, int32_t* agents) {
    if (!h || !agents) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle / agents");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_env_module_agents_of: the handle was not created with dril_create_with_env_module");
    *agents = h->env.agents();
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_scaling_enable(dril_handle* h, int32_t on) {
    NEED(h);
    std::string msg; const int rc = h->env.set_scaling(on != 0, msg);
    return rc ? fail(h, rc, "dril_scaling_enable: " + msg) : DRIL_OK;
}
DRIL_EXPORT int32_t dril_agent_spaces(const dril_handle* h, float* obs_low, float* obs_high, float* action_low, float* action_high, int32_t* scaling) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!h->env.module) return fail(const_cast<dril_handle*>(h), DRIL_ERR_UNSUPPORTED, "dril_agent_spaces: the handle was not created with dril_create_with_env_module");
    h->env.agent_obs_space(obs_low, obs_high);
    if (!h->env.desc.discrete) h->env.agent_action_space(action_low, action_high);
    if (scaling) *scaling = h->env.scaling ? 1 : 0;
    return DRIL_OK;
}

namespace {
#define CCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::string m = std::string(#expr) + ": " + hipGetErrorString(_e); dril_destroy(h); return fail(nullptr, DRIL_ERR_HIP, m); } } while (0)
int create_impl(const dril_config* cfg, const char* module_path, dril_handle** out) {
    if (!cfg || !out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "null cfg/out");
    if (cfg->abi_version != DRIL_ABI_VERSION) return fail(nullptr, DRIL_ERR_INVALID_ARG, "abi_version mismatch");
    if (cfg->env_kind < DRIL_ENV_CARTPOLE || cfg->env_kind > DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "unknown env_kind");
    const bool is_module = cfg->env_kind == DRIL_ENV_MODULE;
    if (is_module && (cfg->norm_obs || cfg->norm_reward)) return fail(nullptr, DRIL_ERR_UNSUPPORTED, "DRIL_ENV_MODULE: NormalizeWrapperEnv through cfg.norm_obs / cfg.norm_reward is for the built-in envs (8 observation dims); wrap a device env plug-in with dril_normalize_enable on the created handle");
    if (is_module && cfg->episode_len < 0) return fail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_MODULE: episode_len must be > 0, or 0 for the plug-in's own time limit");
    const bool ext = cfg->env_kind == DRIL_ENV_EXTERNAL;
    if (ext && (cfg->ext_obs_dim < 1 || cfg->ext_obs_dim > 1024 || cfg->ext_action_dim < 1 || cfg->ext_action_dim > 64)) return fail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_EXTERNAL: ext_obs_dim must be 1..1024 and ext_action_dim 1..64");
    // hidden_dims / activation: n_hidden == 0 is the two-layer form (hidden1, hidden2); otherwise hidden[0 .. n_hidden-1]
    if (cfg->n_hidden < 0 || cfg->n_hidden > kMaxHidden) return fail(nullptr, DRIL_ERR_INVALID_ARG, "n_hidden must be 0 (hidden1 / hidden2) or 1..4");
    if (cfg->activation < 0 || cfg->activation > 7) return fail(nullptr, DRIL_ERR_UNSUPPORTED, "activation must be 0 (tanh), 1 (relu), 2 (sigmoid), 3 (elu), 4 (leakyrelu), 5 (softplus), 6 (gelu) or 7 (swish)");
    int nh = cfg->n_hidden ? cfg->n_hidden : 2, hd[kMaxHidden] = {cfg->hidden1, cfg->hidden2, 0, 0};
    if (cfg->n_hidden) for (int l = 0; l < nh; ++l) hd[l] = cfg->hidden[l];
    for (int l = 0; l < nh; ++l) if (hd[l] < 1 || hd[l] > 1024) return fail(nullptr, DRIL_ERR_INVALID_ARG, "hidden widths must be 1..1024");
    if (ext && (cfg->norm_obs || cfg->norm_reward || cfg->monitor_window)) return fail(nullptr, DRIL_ERR_UNSUPPORTED, "DRIL_ENV_EXTERNAL: NormalizeWrapperEnv / MonitorWrapperEnv wrap the host env on the host");
    if (cfg->n_envs < 1 || cfg->n_steps < 1 || cfg->epochs < 0 || cfg->batch_size < 1) return fail(nullptr, DRIL_ERR_INVALID_ARG, "n_envs/n_steps/batch_size must be positive");
    const bool fused_shape = nh == 2 && cfg->activation == 0 && hd[0] == hd[1] && (hd[0] == 32 || hd[0] == 64 || hd[0] == 128 || hd[0] == 256);   // 32: the reference's benchmark-suite shape (f32-MFMA kernels only)   // everything else: the generic kernels (any depth <= 4, any width <= 1024, tanh / relu)
    if (cfg->monitor_window < 0) return fail(nullptr, DRIL_ERR_INVALID_ARG, "monitor_window must be >= 0");
    if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return fail(nullptr, DRIL_ERR_INVALID_ARG, "bad rank/world_size");
    if (cfg->batch_size % cfg->world_size != 0) return fail(nullptr, DRIL_ERR_INVALID_ARG, "batch_size must be divisible by world_size");
    // Multi-process RCCL on this platform needs dmabuf IPC: with the legacy IPC mode (the ROCr default) `hipIpcGetMemHandle` fails with "invalid argument" on a
    // host driver that only supports dmabuf, and ncclCommInitRank / the first collective across processes dies with it.  The ROCr runtime reads the variable
    // when it initialises, i.e. at this process's first HIP call — which for a DRiL user is normally the plug-in load or the hipSetDevice below.  It is only set if the
    // caller left it unset (bench.py and the tests export it themselves; a process that already touched HIP before dril_create must export it on its own: README "Multi-GPU").
    if (cfg->world_size > 1) setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", /*overwrite=*/0);
    dril_handle* h = nullptr;
    try { h = new dril_handle(); } catch (...) { return fail(nullptr, DRIL_ERR_INVALID_ARG, "out of host memory"); }
    h->cfg = *cfg;
    {   // a plug-in's descriptor gives the spaces: it is loaded here, before anything is sized
        std::string msg; const int rcm = h->env.open(cfg->env_kind, cfg->n_envs, cfg->episode_len, cfg->fixed_length_episodes, cfg->action_start, module_path, cfg->device, msg);
        if (rcm) { delete h; return fail(nullptr, rcm, "dril_create_with_env_module: " + msg); }
        h->cfg.episode_len = h->env.episode_len;
    }
    const DrilEnvPluginDesc& desc = h->env.desc;
    h->cfg.hidden1 = hd[0]; h->cfg.hidden2 = nh > 1 ? hd[1] : hd[0];   // the fused kernels read hidden1 (only reached with two equal layers)
    const EnvKindInfo* kinfo = env_kind_info(cfg->env_kind);
    if (kinfo) { h->discrete = kinfo->discrete; h->D = kinfo->D; h->A = kinfo->A; h->S = kinfo->S; }                             // a built-in kind: fused kernels at the fused shapes
    else if (is_module) { h->discrete = desc.discrete != 0; h->D = desc.D; h->A = desc.A; h->S = desc.S; h->generic = true; }   // no fused kernels for a plug-in env
    else { h->discrete = cfg->ext_discrete != 0; h->D = cfg->ext_obs_dim; h->A = cfg->ext_action_dim; h->S = 0; h->external = true; h->generic = true; }   // DRIL_ENV_EXTERNAL
    h->gd = GenericDims{h->D, h->A, nh, {hd[0], hd[1], hd[2], hd[3]}, h->discrete ? 1 : 0, cfg->activation};
    if (nh == 2) { h->actor = net_off(0, h->D, hd[0], hd[1], h->A); h->critic = net_off(h->actor.end, h->D, hd[0], hd[1], 1); }
    else {                                                                            // other depths exist on the generic path only, which reads just the first offset and the end of a net
        std::memset(&h->actor, 0, sizeof(h->actor)); std::memset(&h->critic, 0, sizeof(h->critic));
        h->actor.w1 = 0; h->actor.end = generic_net_size(h->gd, h->A);
        h->critic.w1 = h->actor.end; h->critic.end = h->actor.end + generic_net_size(h->gd, 1);
    }
    h->Pa = h->actor.end; h->Pc = h->critic.end - h->actor.end; h->log_std_off = h->critic.end;
    h->P = h->critic.end + (h->discrete ? 0 : h->A);
    h->N = (int64_t)cfg->n_envs * cfg->n_steps; h->lr = cfg->learning_rate;
    if (!fused_shape || std::getenv("DRIL_FORCE_GENERIC")) h->generic = true;            // DRIL_FORCE_GENERIC: run a fused-shape handle on the generic kernels (A/B and parity tests)
    if (const char* e = std::getenv("DRIL_FORCE_ALLREDUCE")) h->force_allreduce = std::atoi(e) != 0;
    if (const char* e = std::getenv("DRIL_FORCE_STEPWISE")) h->force_stepwise = std::atoi(e) != 0;
    if (const char* e = std::getenv("DRIL_GRAD_ACTOR_PERMILLE")) { h->grad_actor_pct = std::atoi(e); if (h->grad_actor_pct < 100 || h->grad_actor_pct > 900) h->grad_actor_pct = 0; }
    if (const char* e = std::getenv("DRIL_GRAD_VARIANT")) { h->grad_variant = std::atoi(e); if (h->grad_variant < -1 || h->grad_variant > 2) h->grad_variant = -1; if (h->grad_variant == 2) h->grad_variant = 1; }
    h->no_persistent = std::getenv("DRIL_NO_PERSISTENT_UPDATE") != nullptr; { const char* e = std::getenv("DRIL_NO_EPOCH_INDEX"); h->no_epoch_index = e && std::atoi(e) != 0; }
    if (const char* e = debug_env("DRIL_SMALL_CHUNK")) { const long c = std::atol(e); if (c > 0) { h->small_chunk = c; h->update_fused_chunk = c; } }   // optimiser steps per launch of ppo_update_small_kernel and of ppo_update_generic_small_kernel (tests: launch boundaries)
    h->no_small_path = debug_env("DRIL_NO_SMALL_PATH") != nullptr;
    h->no_f32_retry = std::getenv("DRIL_NO_F32_RETRY") != nullptr;
    CCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop; CCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { std::string m = std::string("libdril_hip targets gfx950 (MI355X) only; device is ") + prop.gcnArchName; dril_destroy(h); return fail(nullptr, DRIL_ERR_UNSUPPORTED, m); }
    h->num_cus = prop.multiProcessorCount;
    {
        char bus[64] = "?"; int ndev = -1; (void)hipDeviceGetPCIBusId(bus, (int)sizeof(bus), cfg->device); (void)hipGetDeviceCount(&ndev);
        const char* hv = std::getenv("HIP_VISIBLE_DEVICES"); const char* rv = std::getenv("ROCR_VISIBLE_DEVICES");
        h->device_info = "device " + std::to_string(cfg->device) + " of " + std::to_string(ndev) + " visible: " + prop.name + " " + prop.gcnArchName + ", " + std::to_string(prop.multiProcessorCount) + " CUs, PCI " + bus +
                         ", HIP_VISIBLE_DEVICES=" + (hv ? hv : "(unset)") + " ROCR_VISIBLE_DEVICES=" + (rv ? rv : "(unset)");
    }
    CCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t E = cfg->n_envs, N = (size_t)h->N, P = h->P;
    CCHK(h->params.alloc(P)); CCHK(h->adam_m.alloc(P)); CCHK(h->adam_v.alloc(P)); CCHK(h->bt.alloc(4));
    CCHK(h->flat.alloc(P + 8)); CCHK(h->norm_out.alloc(1)); CCHK(h->w2max_dev.alloc(1));
    { const size_t words = (size_t)gae_chunks(cfg->n_steps) * cfg->n_envs; CCHK(h->gae_carry.alloc(words)); CCHK(hipMemsetAsync(h->gae_carry, 0, words * 8, h->stream));
      CCHK(h->gae_err.alloc(1)); CCHK(hipMemsetAsync(h->gae_err, 0, 4, h->stream)); }
    h->n_norm_partials = (int)((P + 31) / 32); CCHK(h->norm_partials.alloc(h->n_norm_partials));
    if (h->generic) { h->slab_a = generic_slab_size(h->gd, true); h->slab_c = generic_slab_size(h->gd, false); }
    else { h->slab_a = slab_size_actor(*kinfo, hd[0]); h->slab_c = slab_size_critic(*kinfo, hd[0]); }
    h->wide = !h->generic && hd[0] > 64;
    h->Gmax = (h->wide && hd[0] > 128) ? (h->num_cus / 2 > 0 ? h->num_cus / 2 : 1) : (!h->wide && h->grad_variant != 0) ? 3 * h->num_cus : h->num_cus;   // H = 128: 4 waves and 77 KB LDS per workgroup, two workgroups per CU   // [64,64]: 2 workgroups per CU (actor + critic), 4 waves each; wide: 1 workgroup of H/32 waves per CU
    if (h->generic) h->Gmax = 64;                                                                                                                                                                                             // generic path: one slab per row chunk of the minibatch
    if (const char* e = debug_env("DRIL_GRAD_GMAX")) { const int g = std::atoi(e); if (g > 0 && g < h->Gmax) h->Gmax = g; }   // diagnostic: fewer workgroups per net
    if (h->wide) { const size_t pb = (size_t)hd[0] * hd[0] * 6;    // three bf16 pieces per element
        CCHK(h->w2p_actor.alloc(pb)); CCHK(h->w2tp_actor.alloc(pb)); CCHK(h->w2p_critic.alloc(pb)); CCHK(h->w2tp_critic.alloc(pb));
        CCHK(h->w2pf_actor.alloc(pb)); CCHK(h->w2pf_critic.alloc(pb)); }
    if (h->wide) { const size_t hh = (size_t)hd[0] * hd[0]; CCHK(h->w2a_actor.alloc(hh)); CCHK(h->w2ta_actor.alloc(hh)); CCHK(h->w2a_critic.alloc(hh)); CCHK(h->w2ta_critic.alloc(hh)); }
    CCHK(h->slabs_a.alloc((size_t)h->Gmax * h->slab_a)); CCHK(h->slabs_c.alloc((size_t)h->Gmax * h->slab_c));
    CCHK(h->env.alloc(h->S));
    CCHK(h->obs.alloc(N * h->D)); CCHK(h->act.alloc(N * act_bytes_per(h))); CCHK(h->rew.alloc(N)); CCHK(h->adv.alloc(N));
    CCHK(h->ret.alloc(N)); CCHK(h->logp.alloc(N)); CCHK(h->val.alloc(N)); CCHK(h->boot.alloc(N)); CCHK(h->flags.alloc(N));
    CCHK(h->last_values.alloc(E));
    if (!h->generic) CCHK(h->rec.alloc((size_t)(h->D <= 4 ? 2 : 3) * N));   // packed minibatch records: 2 (D <= 4) or 3 (D <= 8) float4 per sample
    if (h->generic) CCHK(h->gen_tmp.alloc(E));
    if (ext) { CCHK(h->ext_stage_rew.alloc(N)); CCHK(h->ext_stage_flags.alloc(N)); }
    if (ext) {
        CCHK(hipEventCreateWithFlags(&h->ext_ev_in, hipEventDisableTiming)); CCHK(hipEventCreateWithFlags(&h->ext_ev_out, hipEventDisableTiming));
        CCHK(h->ext_err.alloc(1)); CCHK(hipMemsetAsync(h->ext_err, 0, 4, h->stream)); CCHK(h->ext_err_host.alloc(1)); *h->ext_err_host = 0;
    }
    if (cfg->monitor_window > 0) {
        const size_t W = cfg->monitor_window;
        CCHK(h->mon_cur_ret.alloc(E)); CCHK(h->mon_cur_len.alloc(E)); CCHK(h->ep_ret.alloc(N)); CCHK(h->ep_len.alloc(N));
        CCHK(h->mon_ring_ret.alloc(W)); CCHK(h->mon_ring_len.alloc(W)); CCHK(h->e_ep_ret.alloc(E)); CCHK(h->e_ep_len.alloc(E));
        CCHK(h->mon_cnt.alloc((size_t)cfg->n_steps)); CCHK(h->mon_meta.alloc(2)); CCHK(h->e_flags.alloc(E));
        CCHK(hipMemset(h->mon_cur_ret, 0, E * 4)); CCHK(hipMemset(h->mon_cur_len, 0, E * 4)); CCHK(hipMemset(h->mon_meta, 0, 8));
    }
    h->adv_blocks = 1024; CCHK(h->adv_partials.alloc(2 * (size_t)h->adv_blocks)); CCHK(h->adv_stats.alloc(4));
    h->ev_blocks = 1024; CCHK(h->ev_partials.alloc(4 * (size_t)h->ev_blocks));
    CCHK(h->stop_flag.alloc(1)); CCHK(h->nan_flag.alloc(1));
#ifdef DRIL_STAMPS
    CCHK(h->dbg.alloc((size_t)2 * h->Gmax * 4 * 12)); CCHK(hipMemset(h->dbg, 0, (size_t)2 * h->Gmax * 4 * 12 * 8));
#endif
    CCHK(h->e_obs.alloc(E * h->D)); CCHK(h->e_rew.alloc(E)); CCHK(h->e_tobs.alloc(E * h->D)); CCHK(h->e_term.alloc(E));
    CCHK(h->e_trunc.alloc(E)); CCHK(h->e_act.alloc(E * act_bytes_per(h)));
    CCHK(h->e_obs_raw.alloc(E * h->D)); CCHK(h->e_rew_n.alloc(E)); CCHK(h->obs_rms.alloc(2)); CCHK(h->ret_rms.alloc(2)); CCHK(h->rms_partials.alloc((size_t)h->rms_blocks * 16)); CCHK(h->rms_red.alloc(16));
    { RmsState init[2]; for (auto& r : init) { for (int d = 0; d < 8; ++d) { r.mean[d] = 0.f; r.var[d] = 1.f; } r.count = 0; }   // RunningMeanStd{T}(shape): zeros, ones, 0 (normalizeWrapperEnv.jl:14-16)
      CCHK(hipMemcpy(h->obs_rms, init, sizeof(init), hipMemcpyHostToDevice)); CCHK(hipMemcpy(h->ret_rms, init, sizeof(init), hipMemcpyHostToDevice)); }
    CCHK(hipMemsetAsync(h->params, 0, P * 4, h->stream)); CCHK(hipMemsetAsync(h->boot, 0, N * 4, h->stream));
    CCHK(hipMemsetAsync(h->flags, 0, N, h->stream)); CCHK(hipMemsetAsync(h->last_values, 0, E * 4, h->stream));
    CCHK(hipMemsetAsync(h->stop_flag, 0, 4, h->stream)); CCHK(hipMemsetAsync(h->nan_flag, 0, 4, h->stream));
    CCHK(hipMemsetAsync(h->e_tobs, 0, E * h->D * 4, h->stream));
    if (!h->discrete) { std::vector<float> ls(h->A, cfg->log_std_init); CCHK(hipMemcpyAsync(h->params + h->log_std_off, ls.data(), 4 * h->A, hipMemcpyHostToDevice, h->stream)); CCHK(hipStreamSynchronize(h->stream)); }
    int rc = reset_optimizer(h);
    if (rc) { std::string m = h->err; dril_destroy(h); return fail(nullptr, rc, m); }
    *out = h;
    return DRIL_OK;
}
#undef CCHK
}  // namespace
DRIL_EXPORT int32_t dril_create(const dril_config* cfg, dril_handle** out) {
    if (cfg && cfg->abi_version == DRIL_ABI_VERSION && cfg->env_kind == DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "DRIL_ENV_MODULE needs a code object: use dril_create_with_env_module(cfg, code_object_path, out)");
    return create_impl(cfg, nullptr, out);
}
DRIL_EXPORT int32_t dril_create_with_env_module(const dril_config* cfg, const char* code_object_path, dril_handle** out) {
    if (!cfg || !out) return fail(nullptr, DRIL_ERR_INVALID_ARG, "null cfg/out");
    if (cfg->abi_version != DRIL_ABI_VERSION) return fail(nullptr, DRIL_ERR_INVALID_ARG, "abi_version mismatch");
    if (cfg->env_kind != DRIL_ENV_MODULE) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_create_with_env_module: cfg->env_kind must be DRIL_ENV_MODULE");
    std::string msg; const int rc = check_code_object_path(code_object_path, msg);
    if (rc) return fail(nullptr, rc, "dril_create_with_env_module: " + msg);
    return create_impl(cfg, code_object_path, out);
}

DRIL_EXPORT int32_t dril_destroy(dril_handle* h) {
    if (h) (void)hipSetDevice(h->cfg.device);
    if (!h) return DRIL_OK;
    if (h->pop) { h->err = "dril_destroy: the handle is a member of a population: dril_population_destroy first (the members stay alive and usable)"; return DRIL_ERR_INVALID_ARG; }
    if (h->stream) hipStreamSynchronize(h->stream);
    comm_release(h);
    h->env.release();
    if (h->ext_ev_in) (void)hipEventDestroy(h->ext_ev_in); if (h->ext_ev_out) (void)hipEventDestroy(h->ext_ev_out);
    for (auto& p : h->prof_pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto& p : h->prof_pool) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return DRIL_OK;
}
DRIL_EXPORT const char* dril_last_error(const dril_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }
DRIL_EXPORT int32_t dril_synchronize(dril_handle* h) { NEED(h); return sync(h); }
DRIL_EXPORT int32_t dril_obs_dim(const dril_handle* h) { return h ? h->D : -1; }
DRIL_EXPORT int32_t dril_action_dim(const dril_handle* h) { return h ? h->A : -1; }
DRIL_EXPORT int32_t dril_is_discrete(const dril_handle* h) { return h ? (h->discrete ? 1 : 0) : -1; }
DRIL_EXPORT int64_t dril_param_count(const dril_handle* h) { return h ? h->P : -1; }

DRIL_EXPORT int32_t dril_set_params(dril_handle* h, const float* flat, size_t n) {
    NEED(h); if (!flat || n != (size_t)h->P) return fail(h, DRIL_ERR_INVALID_ARG, "dril_set_params: n != dril_param_count");
    HIPCHK(h, hipMemcpyAsync(h->params, flat, n * 4, hipMemcpyHostToDevice, h->stream)); h->wimg_dirty = true;
    if (!h->generic) {                                                                // max |W2| of the new parameters decides the forward's arithmetic (fwd_exact)
        const size_t HH = (size_t)h->cfg.hidden1 * h->cfg.hidden1; float m = 0.f;
        for (const float* w : {flat + h->actor.w2, flat + h->critic.w2}) for (size_t i = 0; i < HH; ++i) { const float x = std::fabs(w[i]); m = (x > m || x != x) ? (x != x ? INFINITY : x) : m; }
        h->w2max = m;
    }
    return sync(h);
}
DRIL_EXPORT int32_t dril_get_params(dril_handle* h, float* flat, size_t n) {
    NEED(h); if (!flat || n != (size_t)h->P) return fail(h, DRIL_ERR_INVALID_ARG, "dril_get_params: n != dril_param_count");
    HIPCHK(h, hipMemcpyAsync(flat, h->params, n * 4, hipMemcpyDeviceToHost, h->stream)); return sync(h);
}
DRIL_EXPORT int32_t dril_reset_optimizer(dril_handle* h) { NEED(h); return reset_optimizer(h); }
DRIL_EXPORT int32_t dril_set_learning_rate(dril_handle* h, float lr) { NEED(h); h->lr = lr; return DRIL_OK; }
DRIL_EXPORT int32_t dril_get_optimizer_state(dril_handle* h, float* m, float* v, size_t n, float* beta_powers, int64_t* steps) {
    NEED(h);
    if (!m || !v || !beta_powers || n != (size_t)h->P) return fail(h, DRIL_ERR_INVALID_ARG, "dril_get_optimizer_state: n != dril_param_count or null pointer");
    float bt[4];
    HIPCHK(h, hipMemcpyAsync(m, h->adam_m, n * 4, hipMemcpyDeviceToHost, h->stream)); HIPCHK(h, hipMemcpyAsync(v, h->adam_v, n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bt, h->bt, sizeof(bt), hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    const int slot = 2 * (int)(h->adam_steps & 1);                                     // the slot the NEXT step reads (ping-pong)
    beta_powers[0] = bt[slot]; beta_powers[1] = bt[slot + 1];
    if (steps) *steps = h->adam_steps;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_set_optimizer_state(dril_handle* h, const float* m, const float* v, size_t n, const float* beta_powers, int64_t steps) {
    NEED(h);
    if (!m || !v || !beta_powers || n != (size_t)h->P || steps < 0) return fail(h, DRIL_ERR_INVALID_ARG, "dril_set_optimizer_state: n != dril_param_count, null pointer or negative step count");
    const float bt[4] = {beta_powers[0], beta_powers[1], beta_powers[0], beta_powers[1]};
    HIPCHK(h, hipMemcpyAsync(h->adam_m, m, n * 4, hipMemcpyHostToDevice, h->stream)); HIPCHK(h, hipMemcpyAsync(h->adam_v, v, n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->bt, bt, sizeof(bt), hipMemcpyHostToDevice, h->stream));
    h->adam_steps = steps;
    return sync(h);
}

// ---- env verbs -----------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_env_reset(dril_handle* h, uint64_t seed) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_reset");
    h->env.seed0 = seed + (uint64_t)h->cfg.rank * (uint64_t)h->cfg.n_envs;
    HIPCHK(h, h->env.reset(h->stream));
    if (h->mon_cur_ret) { HIPCHK(h, hipMemsetAsync(h->mon_cur_ret, 0, (size_t)h->cfg.n_envs * 4, h->stream)); HIPCHK(h, hipMemsetAsync(h->mon_cur_len, 0, (size_t)h->cfg.n_envs * 4, h->stream)); }   // MonitorWrapperEnv.reset! :38-44
    if (h->pn.on) {                                                                  // NormalizeWrapperEnv.reset! :110-121: old_obs = the raw observation, returns = 0, the statistics stay
        HIPCHK(h, hipMemsetAsync(h->env.disc_returns, 0, (size_t)h->cfg.n_envs * 4, h->stream)); HIPCHK(h, h->env.observe(h->e_obs_raw, h->stream));
    }
    h->env.ready = true;
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_observe(dril_handle* h, float* host_obs, int32_t update_stats) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_observe");
    if (!h->env.ready) return fail(h, DRIL_ERR_NOT_INITIALISED, "dril_env_observe before dril_env_reset");
    if (!host_obs) return fail(h, DRIL_ERR_INVALID_ARG, "null host_obs");
    if (normalizing(h) || h->pn.on) { int rc = observe_dev(h, update_stats != 0); if (rc) return rc; }
    else HIPCHK(h, h->env.observe(h->e_obs, h->stream));
    HIPCHK(h, hipMemcpyAsync(host_obs, h->e_obs, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_step(dril_handle* h, const void* actions, float* rewards, uint8_t* terminated, uint8_t* truncated, float* terminal_obs) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_step");
    if (!h->env.ready) return fail(h, DRIL_ERR_NOT_INITIALISED, "dril_env_step before dril_env_reset");
    if (!actions) return fail(h, DRIL_ERR_INVALID_ARG, "null actions");
    const size_t E = h->cfg.n_envs;
    HIPCHK(h, hipMemcpyAsync(h->e_act, actions, E * act_bytes_per(h), hipMemcpyHostToDevice, h->stream));
    float* rew_dev = h->e_rew;
    if (normalizing(h) || h->pn.on) { rew_dev = h->e_rew_n; int rc = step_dev(h, h->e_act, rew_dev, nullptr); if (rc) return rc; }
    else { int rc = env_step_arrays(h, h->e_act); if (rc) return rc; }
    if (rewards) HIPCHK(h, hipMemcpyAsync(rewards, rew_dev, E * 4, hipMemcpyDeviceToHost, h->stream));
    if (terminated) HIPCHK(h, hipMemcpyAsync(terminated, h->e_term, E, hipMemcpyDeviceToHost, h->stream));
    if (truncated) HIPCHK(h, hipMemcpyAsync(truncated, h->e_trunc, E, hipMemcpyDeviceToHost, h->stream));
    if (terminal_obs) HIPCHK(h, hipMemcpyAsync(terminal_obs, h->e_tobs, E * h->D * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_get_state(dril_handle* h, float* state, int32_t* step_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_get_state"); if (!state) return fail(h, DRIL_ERR_INVALID_ARG, "null state");
    // a world handle moves its W = n_envs / N states (S floats each, world w at float offset w S); the counters are per row for every handle
    HIPCHK(h, hipMemcpyAsync(state, h->env.state, (size_t)h->env.n_worlds() * h->S * 4, hipMemcpyDeviceToHost, h->stream));
    if (step_count) HIPCHK(h, hipMemcpyAsync(step_count, h->env.step_count, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_env_set_state(dril_handle* h, const float* state, const int32_t* step_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_env_set_state"); if (!state) return fail(h, DRIL_ERR_INVALID_ARG, "null state");
    if (step_count && h->env.is_world()) {                                             // the N rows of a world count the same steps: unequal values are refused, nothing is written
        const int N = h->env.agents();
        for (int e = 0; e < h->cfg.n_envs; ++e) if (step_count[e] != step_count[e - e % N])
            return fail(h, DRIL_ERR_INVALID_ARG, "dril_env_set_state: rows " + std::to_string(e - e % N) + " and " + std::to_string(e) + " belong to one world of " + std::to_string(N) + " agents but are given step counts " + std::to_string(step_count[e - e % N]) + " and " + std::to_string(step_count[e]) + ": the rows of a world share the world's step count");
    }
    HIPCHK(h, hipMemcpyAsync(h->env.state, state, (size_t)h->env.n_worlds() * h->S * 4, hipMemcpyHostToDevice, h->stream));
    if (step_count) HIPCHK(h, hipMemcpyAsync(h->env.step_count, step_count, (size_t)h->cfg.n_envs * 4, hipMemcpyHostToDevice, h->stream));
    return sync(h);
}
DRIL_EXPORT int32_t dril_norm_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_norm_get_stats");
    if (h->env.module && h->pn.on) return dril_normalize_get_stats(h, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);   // the wrapper of dril_normalize_enable
    NOT_MODULE(h, "dril_norm_get_stats");
    RmsState o, r;
    HIPCHK(h, hipMemcpyAsync(&o, h->obs_rms + h->obs_par, sizeof(o), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&r, h->ret_rms + h->ret_par, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    if (obs_mean) std::memcpy(obs_mean, o.mean, 4 * h->D); if (obs_var) std::memcpy(obs_var, o.var, 4 * h->D); if (obs_count) *obs_count = o.count;
    if (ret_mean) *ret_mean = r.mean[0]; if (ret_var) *ret_var = r.var[0]; if (ret_count) *ret_count = r.count;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_norm_set_stats(dril_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    NEED(h); NOT_EXTERNAL(h, "dril_norm_set_stats");
    if (h->env.module && h->pn.on) return dril_normalize_set_stats(h, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
    NOT_MODULE(h, "dril_norm_set_stats");
    if (!obs_mean || !obs_var) return fail(h, DRIL_ERR_INVALID_ARG, "null statistics");
    RmsState o{}, r{};
    for (int d = 0; d < 8; ++d) { o.mean[d] = d < h->D ? obs_mean[d] : 0.f; o.var[d] = d < h->D ? obs_var[d] : 1.f; r.mean[d] = 0.f; r.var[d] = 1.f; }
    o.count = obs_count; r.mean[0] = ret_mean; r.var[0] = ret_var; r.count = ret_count;
    HIPCHK(h, hipMemcpyAsync(h->obs_rms + h->obs_par, &o, sizeof(o), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->ret_rms + h->ret_par, &r, sizeof(r), hipMemcpyHostToDevice, h->stream));
    return sync(h);
}

DRIL_EXPORT int32_t dril_norm_get_original(dril_handle* h, float* obs, float* rewards) {
    NEED(h); NOT_EXTERNAL(h, "dril_norm_get_original");
    if (h->env.module && h->pn.on) return dril_normalize_get_original(h, obs, rewards);
    NOT_MODULE(h, "dril_norm_get_original");
    if (!normalizing(h)) return fail(h, DRIL_ERR_NOT_INITIALISED, "NormalizeWrapperEnv is off (cfg.norm_obs == cfg.norm_reward == 0)");
    if (obs) HIPCHK(h, hipMemcpyAsync(obs, h->e_obs_raw, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost, h->stream));
    if (rewards) HIPCHK(h, hipMemcpyAsync(rewards, h->e_rew, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}


// ---- policy on host batches ----------------------------------------------------------------------
namespace {
int policy_host(dril_handle* h, const float* obs, int64_t B, const void* noise, void* actions, bool actions_in, float* values, float* logp,
                float* entropy, int mode, int deterministic = 0) {
    if (!obs || B < 1) return fail(h, DRIL_ERR_INVALID_ARG, "policy: null obs or batch < 1");
    DevBuf<float> d_obs, d_val, d_lp, d_ent; DevBuf<char> d_noise, d_act;                       // freed on every return
    const size_t ab = (size_t)B * act_bytes_per(h), nb = (size_t)B * (h->discrete ? 8 : 4 * (size_t)h->A);
    HIPCHK(h, d_obs.alloc((size_t)B * h->D)); HIPCHK(h, d_val.alloc((size_t)B)); HIPCHK(h, d_lp.alloc((size_t)B)); HIPCHK(h, d_ent.alloc((size_t)B));
    HIPCHK(h, d_act.alloc(ab));
    HIPCHK(h, hipMemcpyAsync(d_obs, obs, (size_t)B * h->D * 4, hipMemcpyHostToDevice, h->stream));
    if (noise) { HIPCHK(h, d_noise.alloc(nb)); HIPCHK(h, hipMemcpyAsync(d_noise, noise, nb, hipMemcpyHostToDevice, h->stream)); }
    if (actions_in) HIPCHK(h, hipMemcpyAsync(d_act, actions, ab, hipMemcpyHostToDevice, h->stream));
    { int rcw = ensure_wimg(h); if (rcw) return rcw; }
    PolicyArgs a = policy_args(h, d_obs, B, d_noise, d_act, d_val, d_lp, d_ent, mode);
    a.deterministic = deterministic;
    HIPCHK(h, run_policy(h, a));
    h->policy_calls += 1;
    if (values) HIPCHK(h, hipMemcpyAsync(values, d_val, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (logp && mode != 2) HIPCHK(h, hipMemcpyAsync(logp, d_lp, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (entropy && mode == 1) HIPCHK(h, hipMemcpyAsync(entropy, d_ent, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    if (actions && mode == 0) HIPCHK(h, hipMemcpyAsync(actions, d_act, ab, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
}  // namespace
DRIL_EXPORT int32_t dril_policy_forward(dril_handle* h, const float* obs, int64_t batch, const void* noise, void* actions, float* values, float* logprobs) {
    NEED(h); return policy_host(h, obs, batch, noise, actions, false, values, logprobs, nullptr, 0);
}
DRIL_EXPORT int32_t dril_evaluate_actions(dril_handle* h, const float* obs, const void* actions, int64_t batch, float* values, float* logprobs, float* entropy) {
    NEED(h); if (!actions) return fail(h, DRIL_ERR_INVALID_ARG, "null actions");
    return policy_host(h, obs, batch, nullptr, const_cast<void*>(actions), true, values, logprobs, entropy, 1);
}
DRIL_EXPORT int32_t dril_predict_actions(dril_handle* h, const float* obs, int64_t batch, int32_t deterministic, const void* noise, void* actions) {
    NEED(h); if (!actions) return fail(h, DRIL_ERR_INVALID_ARG, "null actions");
    return policy_host(h, obs, batch, deterministic ? nullptr : noise, actions, false, nullptr, nullptr, nullptr, 0, deterministic ? 1 : 0);
}
DRIL_EXPORT int32_t dril_predict_values(dril_handle* h, const float* obs, int64_t batch, float* values) {
    NEED(h); return policy_host(h, obs, batch, nullptr, nullptr, false, values, nullptr, nullptr, 2);
}

// extract_policy(agent) / extract_policy(agent, norm_env) (deployment_policy.jl:15-22, :52-58) on the device: the actor, log_std, the adapter's bounds and — with_norm —
// the observation statistics in force are copied device-to-device into a policy object of its own (include/dril_policy.h).  Reads the handle, changes nothing in it.
DRIL_EXPORT int32_t dril_policy_from_handle(dril_handle* h, int32_t with_norm, dril_policy** out) {
    if (!h) { policy_set_create_error("dril_policy_from_handle: null handle"); return DRIL_ERR_NOT_INITIALISED; }
    NEED(h);
    auto refuse = [&](int code, const std::string& m) { policy_set_create_error(m); return fail(h, code, m); };
    if (!out) return refuse(DRIL_ERR_INVALID_ARG, "dril_policy_from_handle: null out pointer");
    *out = nullptr;
    PolicyDeviceSource s{}; dril_policy_desc& d = s.desc;
    d.abi_version = DRIL_POLICY_ABI_VERSION; d.kind = h->discrete ? DRIL_POLICY_CATEGORICAL : DRIL_POLICY_DIAG_GAUSSIAN;
    d.obs_dim = h->D; d.action_dim = h->A; d.action_start = h->discrete ? h->cfg.action_start : 0;
    d.n_hidden = h->gd.nh; for (int l = 0; l < h->gd.nh; ++l) d.hidden[l] = h->gd.H[l];
    d.activation = h->cfg.activation; d.device = h->cfg.device;
    if (!h->discrete) for (int a = 0; a < h->A; ++a) {                                 // the Box the ClampAdapter clamps to (default_adapters.jl:4-11)
        if (h->env.module) { d.action_low[a] = h->env.desc.action_low[a]; d.action_high[a] = h->env.desc.action_high[a]; }
        else if (h->external && h->ext_bounds_set) { d.action_low[a] = h->ext_bounds.lo[a]; d.action_high[a] = h->ext_bounds.hi[a]; }   // dril_ext_set_action_bounds
        else if (h->external) { d.action_low[a] = h->cfg.ext_action_low; d.action_high[a] = h->cfg.ext_action_high; }   // low >= high: per-dimension bounds the host env clamps to itself
        else { const EnvKindInfo* k = env_kind_info(h->env.kind); d.action_low[a] = k->act_lo; d.action_high[a] = k->act_hi; }   // a built-in Box: Pendulum's torque [-2, 2], every other [-1, 1]
    }
    if (with_norm) {
        if (h->env.module && h->pn.on) {                                                   // the wrapper of dril_normalize_enable
            d.has_norm = 1; d.clip_obs = h->pn.cfg.clip_obs; d.epsilon = h->pn.cfg.epsilon;
            s.obs_mean = h->pn.half(h->pn.cur); s.obs_var = s.obs_mean + h->D;
        } else if (!h->env.module && !h->external && normalizing(h)) {                     // cfg.norm_obs / cfg.norm_reward: the built-in envs' wrapper
            d.has_norm = 1; d.clip_obs = h->cfg.clip_obs; d.epsilon = h->cfg.norm_epsilon;
            const RmsState* st = h->obs_rms + h->obs_par;
            s.obs_mean = st->mean; s.obs_var = st->var;
        } else return refuse(DRIL_ERR_NOT_INITIALISED, "dril_policy_from_handle: with_norm = 1, but the handle has no NormalizeWrapperEnv (cfg.norm_obs / cfg.norm_reward, or dril_normalize_enable on a plug-in handle)");
    }
    s.actor = h->params + h->actor.w1; s.n = (size_t)h->Pa; s.log_std = h->discrete ? nullptr : h->params + h->log_std_off; s.stream = h->stream;
    std::string msg;
    const int rc = policy_from_device(s, out, &msg);
    return rc ? fail(h, rc, "dril_policy_from_handle: " + msg) : DRIL_OK;
}

// ---- train! ------------------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_train(dril_handle* h, int64_t max_steps, dril_ppo_stats* stats, double* fps, int32_t* iterations_done) {
    NEED(h); NOT_EXTERNAL(h, "dril_train");
    const int64_t per_iter = (int64_t)h->cfg.n_steps * h->cfg.n_envs * h->cfg.world_size;
    const int64_t iterations = max_steps / per_iter;                                   // ppo.jl:117
    int32_t done = 0;
    for (int64_t i = 0; i < iterations; ++i) {
        h->lr = h->cfg.learning_rate;                                                  // ppo.jl:155-156
        double f = 0; int rc = collect_rollout(h, &f, false);                          // ppo.jl:167
        if (rc) { if (iterations_done) *iterations_done = done; return rc; }
        if (fps) fps[i] = f;
        rc = ppo_update(h, stats ? &stats[i] : nullptr);                               // ppo.jl:188-264
        if (rc) { if (iterations_done) *iterations_done = done; return rc; }
        ++done;
    }
    if (iterations_done) *iterations_done = done;
    return DRIL_OK;
}

DRIL_EXPORT int64_t dril_debug_device_bytes_live(void) { return g_devmem_live_bytes.load(); }
DRIL_EXPORT const char* dril_device_info(const dril_handle* h) { return h ? h->device_info.c_str() : ""; }

// ---- measurement ----------------------------------------------------------------------------------------
DRIL_EXPORT int32_t dril_profile_get(dril_handle* h, int32_t kid, double* total_ms, int64_t* launches) {
    NEED(h); if (kid < 0 || kid >= DRIL_K_COUNT) return fail(h, DRIL_ERR_INVALID_ARG, "bad kernel id");
    int rc = sync(h); if (rc) return rc;
    if (total_ms) *total_ms = h->prof_ms[kid]; if (launches) *launches = h->prof_n[kid];
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_profile_launches(dril_handle* h, int32_t kid, int64_t* all_launches) {
    NEED(h); if (kid < 0 || kid >= DRIL_K_COUNT || !all_launches) return fail(h, DRIL_ERR_INVALID_ARG, "bad kernel id");
    *all_launches = h->prof_all[kid];
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_profile_reset(dril_handle* h) {
    NEED(h); int rc = sync(h); if (rc) return rc;
    for (int i = 0; i < DRIL_K_COUNT; ++i) { h->prof_ms[i] = 0; h->prof_n[i] = 0; h->prof_all[i] = 0; }
    return DRIL_OK;
}
DRIL_EXPORT const char* dril_kernel_name(int32_t kid) {
    static const char* names[] = {"rollout_kernel", "gae_kernel", "adv_moments_kernel", "ppo_grad_kernel", "grad_reduce_kernel", "adam_kernel", "ncclAllReduce", "pack_records_kernel", "explained_var_kernel"};
    static_assert(sizeof(names) / sizeof(names[0]) == DRIL_K_COUNT, "one name per kernel class");
    return (kid >= 0 && kid < DRIL_K_COUNT) ? names[kid] : "?";
}
DRIL_EXPORT int32_t dril_kernel_count(void) { return DRIL_K_COUNT; }
static const char* grad_kernel_base(int variant) {
    switch (variant) {
        case 0: return "ppo_grad_kernel: f32 (v_mfma_f32_32x32x2_f32)";
        case 2: return "ppo_grad_wide_kernel: f32 (v_mfma_f32_32x32x2_f32)";
        case 6: return "ppo_update_small_kernel: f32 (f16x2 split, f32 accumulate; v_mfma_f32_32x32x16_f16 x 3 per k16 step on two-piece f16 operands = 2^-24 relative, input layer on v_mfma_f32_32x32x2_f32; two persistent workgroups (actor | critic), all optimiser steps of the iteration in one launch)";
        case 5: return "ppo_grad_pair_kernel: f32 (f16x2 split, f32 accumulate; v_mfma_f32_32x32x16_f16 x 3 per k16 step on two-piece f16 operands = 2^-24 relative, input layer on v_mfma_f32_32x32x2_f32)";
        case 4: return "ppo_grad_wide_split_kernel: f32 (f16x2 split, f32 accumulate; v_mfma_f32_32x32x16_f16 x 3 per k16 step on two-piece f16 operands = 2^-24 relative, input layer on f32 MFMAs, dW1 / dW3 in f32 on the vector ALU)";
        case 7: return "ppo_update_generic_small_kernel: f32 (v_fma_f32 on the vector ALU, f32 accumulate; one workgroup, parameters and gradients in LDS, all optimiser steps of the update in one launch)";
        case 3: return "generic path: f32 contractions (sac_gemm_*; large ones bf16x3 split, f32 accumulate)";
        default: return "none yet";
    }
}
DRIL_EXPORT const char* dril_grad_kernel_info(const dril_handle* h) {
    if (!h) return "?";
    const char* base = grad_kernel_base(h->last_variant);
    if (h->last_variant < 0 || h->last_variant == 6 || h->last_variant == 7) return base;              // no step yet; the persistent update kernels have no slab grid
    std::snprintf(h->grad_info, sizeof(h->grad_info), "%s; grid G=%d Gc=%d", base, h->last_G, h->last_Gc);   // what ppo_step launched: slabs (ppo_grad_pair_kernel: pairs) of the actor, of the critic
    return h->grad_info;
}
DRIL_EXPORT const char* dril_version(void) { return "dril_hip 0.2 (gfx950, abi 2)"; }
