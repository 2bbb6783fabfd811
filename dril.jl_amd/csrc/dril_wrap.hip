// dril_wrap.hip — NormalizeWrapperEnv around a device env plug-in (dril_normalize_*) and around the envs of a DRIL_ENV_EXTERNAL handle (dril_ext_normalize_*), and
// MonitorWrapperEnv's statistics (dril_monitor_get_stats, dril_ext_monitor_*; include/dril_hip.h).  Both normalisers sit in this one unit: they share
// norm_moments_kernel<64>, and no kernel may be instantiated in two objects
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dril_handle.h"
#include "dril_ppo_norm.h"   // the plug-in handle's kernels: ppo_norm_fold_kernel, ppo_norm_apply_kernel; the table shape (pn_rows, pn_tiles)
#include "dril_ext_norm.h"   // the external handle's kernels: ext_norm_observe_kernel, ext_norm_record_kernel

using namespace dril;
using namespace dril::ppo;

namespace {
// ---- the wrapper's state and the two launches both handles' forms share ----
void pn_free(dril_handle* h) { h->pn.release(); h->pn_red.release(); }
// the apply grid of the three kernels (ppo_norm_apply_kernel, ext_norm_observe_kernel, ext_norm_record_kernel): env ranges x column tiles
dim3 pn_grid(int E, int D, int* epb) {
    const int W = D > kPnTile ? kPnTile : D;
    *epb = std::max(std::max(1, 4096 / W), (E + 255) / 256);
    return dim3((E + *epb - 1) / *epb, pn_tiles(D));
}
// norm_moments_kernel over n_envs rows of observations (raw) and / or the `returns` recursion over n_envs rewards (rew) — e_obs_raw / e_rew on a plug-in handle, the
// caller's arrays on an external one; *rows: the rows of the table it writes
int pn_moments(dril_handle* h, const float* raw, const float* rew, int* rows) {
    const int E = h->cfg.n_envs, D = h->D;
    *rows = pn_rows(E, D, h->pn_rows_cap);
    const int R = (E + *rows - 1) / *rows;
    *rows = (E + R - 1) / R;
    const NormMomArgs m{E, D, R, raw, rew, h->env.disc_returns, h->pn.cfg.gamma, h->pn.partials};
    hipLaunchKernelGGL(norm_moments_kernel<kPnTile>, dim3(*rows, raw ? pn_tiles(D) : 1), dim3(256), 0, h->stream, m);
    HIPCHK(h, hipGetLastError());
    return DRIL_OK;
}
// ppo_norm_apply_kernel.  Data-parallel jobs: the batch moments cover every env of the job (global_partials does the same for the built-in envs' 16 columns) — this
// rank's table folded to one row of 2 D + 2 doubles, ONE all-reduce of that row, and every rank applies the identical merge with n = world * E, so the statistics
// stay bit-identical across ranks
int pn_apply(dril_handle* h, PnApplyArgs p, int rows, bool upd_obs, bool upd_ret) {
    NormWrapArgs& a = p.w;
    const int E = h->cfg.n_envs, D = h->D, C = 2 * D + 2;
    const int world = comm_ready(h) ? h->cfg.world_size : 1;
    h->pn.fill(a, upd_obs, upd_ret, E);
    a.E = E; a.rows = rows;
    if ((upd_obs || upd_ret) && (world > 1 || (comm_ready(h) && h->force_allreduce))) {
        hipLaunchKernelGGL(ppo_norm_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, h->stream, h->pn.partials, rows, C, h->pn_red);
        HIPCHK(h, hipGetLastError());
        int rc = rccl_allreduce(h, h->pn_red, (size_t)C, kNcclFloat64); if (rc) return rc;
        a.partials = h->pn_red; a.rows = 1; a.n = (long long)E * world;
    }
    const dim3 grid = pn_grid(E, D, &a.epb);
    hipLaunchKernelGGL(ppo_norm_apply_kernel, grid, dim3(256), 0, h->stream, p);
    HIPCHK(h, hipGetLastError());
    h->pn.commit(a);
    return DRIL_OK;
}
}  // namespace
namespace dril::ppo {
// observe(env) of the wrapper (:123-137): the plug-in's observe kernel into e_obs_raw, then moments + apply into e_obs
int pn_observe(dril_handle* h, bool update_stats) {
    HIPCHK(h, h->env.observe(h->e_obs_raw, h->stream));
    const bool upd = update_stats && h->pn.cfg.training && h->pn.cfg.norm_obs;
    int rows = 0;
    if (upd) { int rc = pn_moments(h, h->e_obs_raw, nullptr, &rows); if (rc) return rc; }
    PnApplyArgs a{}; a.w.raw = h->e_obs_raw; a.w.obs_out = h->e_obs;
    return pn_apply(h, a, rows, upd, false);
}
// act!(env, actions) of the wrapper (:139-165) through the E-sized per-step arrays: raw rewards stay in e_rew, the delivered ones go to rew_out
int pn_step(dril_handle* h, const void* actions, float* rew_out) {
    { int rcs = env_step_arrays(h, actions); if (rcs) return rcs; }                // (MonitorWrapperEnv sits inside: raw rewards)
    const bool upd = h->pn.cfg.training && h->pn.cfg.norm_reward;
    int rows = 0;
    if (upd) { int rc = pn_moments(h, nullptr, h->e_rew, &rows); if (rc) return rc; }
    PnApplyArgs a{}; a.w.rew = h->e_rew; a.rew_out = rew_out; a.w.returns = h->env.disc_returns; a.w.term = h->e_term; a.w.trunc = h->e_trunc; a.tobs = h->e_tobs;
    return pn_apply(h, a, rows, false, upd);
}

// the loop of collect_rollout_module (dril_rollout.hip) under dril_normalize_enable: the plug-in's step kernel writes raw reward, terminal observation and raw next observation into the per-step arrays, then
// norm_moments_kernel (dril_norm_wrap.h) + ppo_norm_apply_kernel (dril_ppo_norm.h) put the normalised reward into row t and the normalised next observation where the policy reads it:
// two launches more per env step than collect_rollout_module, and two for the opening observe.  V(terminal_observation) is V of the normalised terminal observation
int collect_rollout_module_norm(dril_handle* h) {
    const int E = h->cfg.n_envs, T = h->cfg.n_steps, D = h->D, A = h->A;
    const size_t ab = act_bytes_per(h);
    const bool upd_obs = h->pn.cfg.training && h->pn.cfg.norm_obs, upd_ret = h->pn.cfg.training && h->pn.cfg.norm_reward;
    int rc = pn_observe(h, true); if (rc) return rc;                                       // new_obs = observe(env), trajectory.jl:32
    h->rollout_launches += 3 + (int64_t)T * (2 + ((upd_obs || upd_ret) ? 1 : 0));          // observe + its wrapper; per step: the step kernel, the apply kernel, the moments
    for (int t = 0; t < T; ++t) {
        const size_t k = (size_t)t * E;
        const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * (size_t)A)) : nullptr;
        PolicyArgs p = policy_args(h, h->e_obs, E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);
        p.gstep = h->env.gstep; p.env_seed0 = h->env.seed0; p.obs_out = h->obs + k * D;
        if (t > 0) { p.boot_obs = h->e_tobs; p.boot_where = h->e_trunc; p.boot_out = h->boot + (k - E); }   // :57-61 for step t-1
        HIPCHK(h, run_policy(h, p));                                                       // get_action_and_values, :41
        HIPCHK(h, h->env.step((const char*)h->act + k * ab, EnvStepOut{h->e_rew, h->e_term, h->e_trunc, h->e_tobs, h->e_obs_raw}, monitor_rollout_args(h, k), h->stream));   // to_env + the env's own act! + raw observe
        int rows = 0;
        if (upd_obs || upd_ret) { rc = pn_moments(h, upd_obs ? h->e_obs_raw : nullptr, upd_ret ? h->e_rew : nullptr, &rows); if (rc) return rc; }
        PnApplyArgs a{}; a.w.raw = h->e_obs_raw; a.w.obs_out = h->e_obs;
        a.w.rew = h->e_rew; a.rew_out = h->rew + k; a.w.returns = h->env.disc_returns; a.w.term = h->e_term; a.w.trunc = h->e_trunc; a.tobs = h->e_tobs;
        rc = pn_apply(h, a, rows, upd_obs, upd_ret); if (rc) return rc;                    // the wrapper's act! :139-165 and observe :123-137
    }
    PolicyArgs l = policy_args(h, h->e_obs, E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);
    l.boot_obs = h->e_tobs; l.boot_where = h->e_trunc; l.boot_out = h->boot + (size_t)(T - 1) * E;
    HIPCHK(h, run_policy(h, l));                                                           // V(new_obs) for rollout-limited tails, :65-70
    return monitor_collect_rollout(h);
}
}  // namespace dril::ppo

// ---- NormalizeWrapperEnv around a device env plug-in (rules and state: dril_norm_wrap.h) ------------------------------------------------------------------------------------
namespace {
int pn_kind_check(dril_handle* h, const char* what) {
    if (h->external) return fail(h, DRIL_ERR_UNSUPPORTED, std::string(what) + ": the envs of DRIL_ENV_EXTERNAL live on the host: NormalizeWrapperEnv wraps them there (envs whose arrays live on the device: dril_ext_normalize_enable, honoured by the dril_ext_*_device verbs)");
    if (!h->env.module) return fail(h, DRIL_ERR_UNSUPPORTED, std::string(what) + ": this verb family wraps a device env plug-in (DRIL_ENV_MODULE); a built-in env is wrapped at create with cfg.norm_obs / cfg.norm_reward (dril_norm_get_stats / dril_norm_set_stats / dril_norm_get_original)");
    return DRIL_OK;
}
#define PN_ON(h, what) do { int _rc = pn_kind_check(h, what); if (_rc) return _rc; \
    if (!(h)->pn.on) return fail(h, DRIL_ERR_NOT_INITIALISED, what ": NormalizeWrapperEnv is off (dril_normalize_enable has not been called with a configuration)"); } while (0)
// the bodies of the verbs that read or write a wrapper that is on: one definition for dril_normalize_* (plug-in handles) and dril_ext_normalize_* (external handles)
int pn_get_config(dril_handle* h, const char* verb, dril_normalize_config* cfg) {
    if (!cfg) return fail(h, DRIL_ERR_INVALID_ARG, std::string(verb) + ": null out pointer");
    *cfg = h->pn.cfg;
    return DRIL_OK;
}
int pn_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    std::vector<float> st(h->pn.stats_floats());
    HIPCHK(h, hipMemcpyAsync(st.data(), h->pn.half(h->pn.cur), st.size() * 4, hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    h->pn.unpack(st, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
    return DRIL_OK;
}
int pn_set_stats(dril_handle* h, const char* verb, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    if (const NormErr err = norm_set_stats_check(obs_mean, obs_var, obs_count, ret_count)) return fail(h, err.code, std::string(verb) + ": " + err.msg);
    const std::vector<float> st = h->pn.pack(obs_mean, obs_var, ret_mean, ret_var);
    HIPCHK(h, hipMemcpyAsync(h->pn.half(h->pn.cur), st.data(), st.size() * 4, hipMemcpyHostToDevice, h->stream));
    int rc = sync(h); if (rc) return rc;
    h->pn.obs_count = obs_count; h->pn.ret_count = ret_count;
    return DRIL_OK;
}
int pn_get_original(dril_handle* h, const char* verb, float* obs, float* rewards) {
    if (!obs && !rewards) return fail(h, DRIL_ERR_INVALID_ARG, std::string(verb) + ": both out pointers are null");
    if (obs) HIPCHK(h, hipMemcpyAsync(obs, h->e_obs_raw, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost, h->stream));
    if (rewards) HIPCHK(h, hipMemcpyAsync(rewards, h->e_rew, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
int pn_get_returns(dril_handle* h, const char* verb, float* returns) {
    if (!returns) return fail(h, DRIL_ERR_INVALID_ARG, std::string(verb) + ": null out pointer");
    HIPCHK(h, hipMemcpyAsync(returns, h->env.disc_returns, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost, h->stream));
    return sync(h);
}
}  // namespace
DRIL_EXPORT int32_t dril_normalize_config_default(dril_normalize_config* c) {
    if (!c) return fail(nullptr, DRIL_ERR_INVALID_ARG, "dril_normalize_config_default: null configuration");
    norm_config_default(c);
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_normalize_enable(dril_handle* h, const dril_normalize_config* cfg) {
    NEED(h);
    { int rc = pn_kind_check(h, "dril_normalize_enable"); if (rc) return rc; }
    if (!cfg) {                                                                        // the wrapper off: the handle enqueues the launches of a handle that never had it
        if (!h->pn.on) return DRIL_OK;
        int rc = sync(h); if (rc) return rc;
        pn_free(h);
        return DRIL_OK;
    }
    if (h->fused_rollout) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_normalize_enable: the fused rollout is on, and a workgroup per tile of envs cannot keep statistics that couple all envs at every step: switch it off with dril_rollout_fused_enable(h, 0) first");
    if (const NormErr err = norm_config_check(*cfg, h->D)) return fail(h, err.code, "dril_normalize_enable: " + err.msg);
    const dril_normalize_config c = norm_config_canonical(*cfg);
    if (h->pn.keeps(c)) return DRIL_OK;                                                // the same wrapper again (training apart): its statistics and returns stay
    { int rc = sync(h); if (rc) return rc; }
    pn_free(h);
    const size_t E = (size_t)h->cfg.n_envs, D = (size_t)h->D, Cn = 2 * D + 2;
    h->pn_rows_cap = 0;
    if (const char* e = debug_env("DRIL_NORM_ROWS")) { const int r = std::atoi(e); if (r > 0) h->pn_rows_cap = r; }   // measurements: fewer rows in the partial table
    hipError_t e = h->pn.alloc((int)D, (size_t)pn_rows((int)E, (int)D, h->pn_rows_cap));
    if (e == hipSuccess) e = h->pn_red.alloc(Cn);
    if (e == hipSuccess) e = hipMemset(h->pn_red, 0, Cn * 8);
    if (e == hipSuccess) e = hipMemset(h->env.disc_returns, 0, E * 4);                     // returns, and the cached originals, start at 0
    if (e == hipSuccess) e = hipMemset(h->e_obs_raw, 0, E * D * 4);
    if (e == hipSuccess) e = hipMemset(h->e_rew, 0, E * 4);
    if (e != hipSuccess) { pn_free(h); return fail(h, DRIL_ERR_HIP, std::string("dril_normalize_enable: ") + hipGetErrorString(e)); }
    h->pn.cfg = c; h->pn.on = true;
    if (h->env.ready) HIPCHK(h, h->env.observe(h->e_obs_raw, h->stream));                    // old_obs of the envs' present state, as reset! would have stored it
    return sync(h);
}
DRIL_EXPORT int32_t dril_normalize_set_training(dril_handle* h, int32_t training) {
    NEED(h); PN_ON(h, "dril_normalize_set_training");
    h->pn.cfg.training = training != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_normalize_get_config(dril_handle* h, dril_normalize_config* cfg) {
    NEED(h); PN_ON(h, "dril_normalize_get_config");
    return pn_get_config(h, "dril_normalize_get_config", cfg);
}
DRIL_EXPORT int32_t dril_normalize_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    NEED(h); PN_ON(h, "dril_normalize_get_stats");
    return pn_get_stats(h, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_normalize_set_stats(dril_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    NEED(h); PN_ON(h, "dril_normalize_set_stats");
    return pn_set_stats(h, "dril_normalize_set_stats", obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_normalize_get_original(dril_handle* h, float* obs, float* rewards) {
    NEED(h); PN_ON(h, "dril_normalize_get_original");
    return pn_get_original(h, "dril_normalize_get_original", obs, rewards);
}
DRIL_EXPORT int32_t dril_normalize_get_returns(dril_handle* h, float* returns) {
    NEED(h); PN_ON(h, "dril_normalize_get_returns");
    return pn_get_returns(h, "dril_normalize_get_returns", returns);
}

namespace {
int monitor_window_stats(dril_handle* h, int W, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes) {
    std::vector<float> r(W); std::vector<int32_t> l(W); int meta[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(r.data(), h->mon_ring_ret, (size_t)W * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(l.data(), h->mon_ring_len, (size_t)W * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(meta, h->mon_meta, 8, hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    double sr = 0, sl = 0;
    for (int i = 0; i < meta[0]; ++i) { sr += r[i]; sl += l[i]; }
    if (n_episodes) *n_episodes = meta[0];
    if (ep_rew_mean) *ep_rew_mean = meta[0] ? (float)(sr / meta[0]) : 0.f;      // log_stats: mean over the CircularBuffer, monitorWrapperEnv.jl:64-70
    if (ep_len_mean) *ep_len_mean = meta[0] ? (float)(sl / meta[0]) : 0.f;
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_monitor_get_stats(dril_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes) {
    NEED(h);
    if (!h->mon_cur_ret || h->external) return fail(h, DRIL_ERR_NOT_INITIALISED, "MonitorWrapperEnv is off (cfg.monitor_window == 0)");   // (an external handle's monitor: dril_ext_monitor_get_stats)
    return monitor_window_stats(h, h->cfg.monitor_window, ep_rew_mean, ep_len_mean, n_episodes);
}

// ---- NormalizeWrapperEnv / MonitorWrapperEnv around the envs of an external handle (dril_ext_normalize_enable / dril_ext_monitor_enable) ----
namespace dril::ppo {
// observe (:123-137) of B rows of the caller's array into obs_out.  rollout: a verb of the collection (B == n_envs) — statistics updated where training && norm_obs,
// old_obs cached; else the read-only pass of dril_predict_actions_device.  *added: the launches enqueued
int xn_observe(dril_handle* h, const float* raw, int64_t B, float* obs_out, bool rollout, int64_t* added) {
    const bool upd = rollout && h->pn.cfg.training && h->pn.cfg.norm_obs;
    int rows = 0;
    if (upd) { int rc = pn_moments(h, raw, nullptr, &rows); if (rc) return rc; *added += 1; }
    XnObserveArgs p{}; NormWrapArgs& a = p.w;
    h->pn.fill(a, upd, false, (long long)B);
    a.E = (int)B; a.rows = rows; a.raw = raw; a.obs_out = obs_out; p.old_obs = rollout ? h->e_obs_raw : nullptr;
    const dim3 grid = pn_grid(a.E, h->D, &a.epb);
    hipLaunchKernelGGL(ext_norm_observe_kernel, grid, dim3(256), 0, h->stream, p);
    HIPCHK(h, hipGetLastError());
    h->pn.commit(a); *added += 1;
    return DRIL_OK;
}
// act! (:139-165) with the record's own work and the monitor's sums, row k / E of the buffer.  tobs_norm: where the critic must read the terminal observations
// (the scratch, or the caller's array with norm_obs == 0; null without terminal_obs)
int xn_record(dril_handle* h, size_t k, const float* d_rewards, const uint8_t* d_terminated, const uint8_t* d_truncated, const float* d_terminal_obs, const float** tobs_norm, int64_t* launches) {
    const int E = h->cfg.n_envs;
    const bool upd = h->pn.on && h->pn.cfg.training && h->pn.cfg.norm_reward;
    int rows = 0;
    if (upd) { int rc = pn_moments(h, nullptr, d_rewards, &rows); if (rc) return rc; *launches += 1; }
    XnRecordArgs p{}; NormWrapArgs& a = p.w;
    if (h->pn.on) h->pn.fill(a, false, upd, E);
    a.D = h->D; a.E = E; a.rows = rows; a.rew = d_rewards; a.term = d_terminated; a.trunc = d_truncated; a.returns = h->env.disc_returns;
    p.has_norm = h->pn.on ? 1 : 0;
    p.tobs = d_terminal_obs; p.tobs_out = (d_terminal_obs && h->pn.on && h->pn.cfg.norm_obs) ? h->e_tobs : nullptr;
    *tobs_norm = p.tobs_out ? p.tobs_out : d_terminal_obs;
    p.old_rew = h->e_rew; p.rew_out = h->rew + k; p.flags = h->flags + k; p.boot = h->boot + k; p.err = h->ext_err;
    if (h->ext_mon_window > 0) { p.mon_cur_ret = h->mon_cur_ret; p.mon_cur_len = h->mon_cur_len; p.ep_ret = h->ep_ret + k; p.ep_len = h->ep_len + k; }
    dim3 grid = pn_grid(E, h->D, &a.epb);
    if (!p.tobs_out && !a.st_out) grid.y = 1;                                            // no column work and no statistics to carry: the per-env pass alone
    hipLaunchKernelGGL(ext_norm_record_kernel, grid, dim3(256), 0, h->stream, p);
    HIPCHK(h, hipGetLastError());
    if (h->pn.on) h->pn.commit(a);
    *launches += 1;
    return DRIL_OK;
}
}  // namespace dril::ppo
namespace {
// the monitor's arrays of an external handle (those of cfg.monitor_window on a device env, sized by ext_mon_window)
void xm_free(dril_handle* h) {
    h->mon_cur_ret.release(); h->mon_cur_len.release(); h->ep_ret.release(); h->ep_len.release();
    h->mon_ring_ret.release(); h->mon_ring_len.release(); h->mon_cnt.release(); h->mon_meta.release();
    h->ext_mon_window = 0;
}
int xw_kind_check(dril_handle* h, const char* what) {
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, std::string(what) + ": the handle was not created with DRIL_ENV_EXTERNAL; a built-in env is wrapped at create (cfg.norm_obs / cfg.norm_reward / cfg.monitor_window), a device env plug-in with dril_normalize_enable");
    return DRIL_OK;
}
int xw_between_rollouts(dril_handle* h, const char* what) {
    if (h->ext_t != 0 || h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, std::string(what) + ": a rollout is under way (dril_ext_steps != 0, or an act without its record): switch the wrapper between rollouts, after dril_ext_finish_device");
    return DRIL_OK;
}
#define XN_ON(h, what) do { int _rc = xw_kind_check(h, what); if (_rc) return _rc; \
    if (!(h)->pn.on) return fail(h, DRIL_ERR_NOT_INITIALISED, what ": NormalizeWrapperEnv is off (dril_ext_normalize_enable has not been called with a configuration)"); } while (0)
}  // namespace
// ---- NormalizeWrapperEnv / MonitorWrapperEnv on an external handle (rules and state: dril_norm_wrap.h; kernels: dril_ext_norm.h) ----
DRIL_EXPORT int32_t dril_ext_normalize_enable(dril_handle* h, const dril_normalize_config* cfg) {
    NEED(h);
    { int rc = xw_kind_check(h, "dril_ext_normalize_enable"); if (rc) return rc; }
    if (h->cfg.world_size > 1) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_normalize_enable: world_size > 1: the batch moments of a data-parallel job need an all-reduce per env step, which is not free of host waits here; run a single rank, or normalise in the env's own arrays");
    { int rc = xw_between_rollouts(h, "dril_ext_normalize_enable"); if (rc) return rc; }
    if (!cfg) {                                                                        // the wrapper off: the handle enqueues the launches of a handle that never had it
        if (!h->pn.on) return DRIL_OK;
        int rc = sync(h); if (rc) return rc;
        pn_free(h);
        return DRIL_OK;
    }
    if (const NormErr err = norm_config_check(*cfg, h->D)) return fail(h, err.code, "dril_ext_normalize_enable: " + err.msg);
    const dril_normalize_config c = norm_config_canonical(*cfg);
    if (h->pn.keeps(c)) return DRIL_OK;                                                // the same wrapper again (training apart): its statistics and returns stay
    { int rc = sync(h); if (rc) return rc; }
    pn_free(h);
    const size_t E = (size_t)h->cfg.n_envs, D = (size_t)h->D;
    h->pn_rows_cap = 0;
    hipError_t e = h->pn.alloc((int)D, (size_t)pn_rows((int)E, (int)D, h->pn_rows_cap));   // every array of the wrapper that create did not size: statistics and the partial table
    if (e == hipSuccess) e = hipMemset(h->env.disc_returns, 0, E * 4);                     // returns, and the cached originals, start at 0
    if (e == hipSuccess) e = hipMemset(h->e_obs_raw, 0, E * D * 4);
    if (e == hipSuccess) e = hipMemset(h->e_rew, 0, E * 4);
    if (e != hipSuccess) { pn_free(h); return fail(h, DRIL_ERR_HIP, std::string("dril_ext_normalize_enable: ") + hipGetErrorString(e)); }
    h->pn.cfg = c; h->pn.on = true; h->xw_allocs = 0;
    return sync(h);
}
DRIL_EXPORT int32_t dril_ext_normalize_set_training(dril_handle* h, int32_t training) {
    NEED(h); XN_ON(h, "dril_ext_normalize_set_training");
    h->pn.cfg.training = training != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_normalize_get_config(dril_handle* h, dril_normalize_config* cfg) {
    NEED(h); XN_ON(h, "dril_ext_normalize_get_config");
    return pn_get_config(h, "dril_ext_normalize_get_config", cfg);
}
DRIL_EXPORT int32_t dril_ext_normalize_get_stats(dril_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    NEED(h); XN_ON(h, "dril_ext_normalize_get_stats");
    return pn_get_stats(h, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_ext_normalize_set_stats(dril_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    NEED(h); XN_ON(h, "dril_ext_normalize_set_stats");
    return pn_set_stats(h, "dril_ext_normalize_set_stats", obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_ext_normalize_get_original(dril_handle* h, float* obs, float* rewards) {
    NEED(h); XN_ON(h, "dril_ext_normalize_get_original");
    return pn_get_original(h, "dril_ext_normalize_get_original", obs, rewards);
}
DRIL_EXPORT int32_t dril_ext_normalize_get_returns(dril_handle* h, float* returns) {
    NEED(h); XN_ON(h, "dril_ext_normalize_get_returns");
    return pn_get_returns(h, "dril_ext_normalize_get_returns", returns);
}
DRIL_EXPORT int32_t dril_ext_normalize_reset(dril_handle* h, void* caller_stream) {
    NEED(h); XN_ON(h, "dril_ext_normalize_reset");
    int rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->env.disc_returns, 0, (size_t)h->cfg.n_envs * 4, h->stream));   // reset! :118; old_obs follows with the next observe
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_monitor_enable(dril_handle* h, int32_t stats_window) {
    NEED(h);
    { int rc = xw_kind_check(h, "dril_ext_monitor_enable"); if (rc) return rc; }
    if (stats_window < 0) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_monitor_enable: stats_window must be >= 0 (0: off)");
    { int rc = xw_between_rollouts(h, "dril_ext_monitor_enable"); if (rc) return rc; }
    if (stats_window == h->ext_mon_window) return DRIL_OK;                             // the window in force (or off while off): nothing changes
    { int rc = sync(h); if (rc) return rc; }
    xm_free(h);
    if (stats_window == 0) return DRIL_OK;
    const size_t E = (size_t)h->cfg.n_envs, N = (size_t)h->N, W = (size_t)stats_window;
    hipError_t e = h->mon_cur_ret.alloc(E);
    if (e == hipSuccess) e = h->mon_cur_len.alloc(E);
    if (e == hipSuccess) e = h->ep_ret.alloc(N);
    if (e == hipSuccess) e = h->ep_len.alloc(N);
    if (e == hipSuccess) e = h->mon_ring_ret.alloc(W);
    if (e == hipSuccess) e = h->mon_ring_len.alloc(W);
    if (e == hipSuccess) e = h->mon_cnt.alloc((size_t)h->cfg.n_steps);
    if (e == hipSuccess) e = h->mon_meta.alloc(2);
    if (e == hipSuccess) e = hipMemset(h->mon_cur_ret, 0, E * 4);                      // fresh sums, an empty window
    if (e == hipSuccess) e = hipMemset(h->mon_cur_len, 0, E * 4);
    if (e == hipSuccess) e = hipMemset(h->mon_meta, 0, 8);
    if (e != hipSuccess) { xm_free(h); return fail(h, DRIL_ERR_HIP, std::string("dril_ext_monitor_enable: ") + hipGetErrorString(e)); }
    h->ext_mon_window = stats_window;
    if (!h->pn.on) h->xw_allocs = 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_monitor_get_stats(dril_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes) {
    NEED(h);
    { int rc = xw_kind_check(h, "dril_ext_monitor_get_stats"); if (rc) return rc; }
    if (h->ext_mon_window < 1) return fail(h, DRIL_ERR_NOT_INITIALISED, "dril_ext_monitor_get_stats: MonitorWrapperEnv is off (dril_ext_monitor_enable has not been called with a window)");
    return monitor_window_stats(h, h->ext_mon_window, ep_rew_mean, ep_len_mean, n_episodes);
}
DRIL_EXPORT int32_t dril_ext_wrap_info(const dril_handle* h, struct dril_ext_wrap_info* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return DRIL_ERR_INVALID_ARG;
    if (!h->external) return DRIL_ERR_UNSUPPORTED;
    std::memset(out, 0, sizeof(*out));
    out->normalize_on = h->pn.on ? 1 : 0; out->monitor_on = h->ext_mon_window > 0 ? 1 : 0; out->monitor_window = h->ext_mon_window;
    out->launches_act = h->xw_added[0]; out->launches_record = h->xw_added[1]; out->launches_finish = h->xw_added[2]; out->allocations = h->xw_allocs;
    return DRIL_OK;
}
