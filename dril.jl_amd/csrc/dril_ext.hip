// dril_ext.hip — the verbs of a DRIL_ENV_EXTERNAL handle (dril_handle.h): act / record / finish on host arrays and on device arrays, dril_predict_actions_device, the
// ClampAdapter's bounds and the counters.  Their kernels: dril_ext_device.hip; the wrappers they honour: dril_wrap.hip.
#include <cstring>
#include <string>
#include <vector>

#include "dril_handle.h"

#include "dril_ext_stream.h"  // the pointer rule and the stream hand-over of the device-array verbs, shared with the SAC handle

using namespace dril;
using namespace dril::ppo;

namespace {
// dril_ext_device_info counts per rollout: the first act of a rollout starts the counters again
void ext_count_begin(dril_handle* h) { if (h->ext_t == 0) { h->ext_steps_dev = h->ext_steps_host = h->ext_syncs = 0; h->ext_launches = 0; h->xw_added[0] = h->xw_added[1] = h->xw_added[2] = 0; } }
// the one drain of a rollout over external envs; the sticky error word of dril_ext_record_device comes back with it (a rollout may mix host and device verbs)
int ext_finish_drain(dril_handle* h, const char* verb) {
    HIPCHK(h, hipMemcpyAsync(h->ext_err_host, h->ext_err, 4, hipMemcpyDeviceToHost, h->stream));
    int rc = sync(h); if (rc) return rc;
    if (*h->ext_err_host) {
        *h->ext_err_host = 0;
        HIPCHK(h, hipMemsetAsync(h->ext_err, 0, 4, h->stream));
        return fail(h, DRIL_ERR_INVALID_ARG, std::string(verb) + ": dril_ext_record_device: truncated envs need terminal_obs (infos[i][\"terminal_observation\"], multithreadedParallelEnv.jl:64-66); the rollout is discarded");
    }
    return DRIL_OK;
}
// an argument of a device verb must be memory the handle's device can address, long enough for the array: a host pointer handed to a kernel is a GPU fault
int ext_check_ptr(dril_handle* h, const char* verb, const char* name, const void* p, size_t bytes) {
    const std::string msg = ext_ptr_problem(h->cfg.device, verb, name, p, bytes);         // dril_ext_stream.h: the rule the SAC handle's device verbs share
    return msg.empty() ? DRIL_OK : fail(h, DRIL_ERR_INVALID_ARG, msg);
}
}  // namespace
namespace dril::ppo {
// the handle's stream takes over from the caller's stream / hands back to it: two events per handle, no host wait
int ext_stream_enter(dril_handle* h, void* caller_stream) { HIPCHK(h, ext_stream_take(h->stream, h->ext_ev_in, caller_stream)); return DRIL_OK; }
int ext_stream_leave(dril_handle* h, void* caller_stream) { HIPCHK(h, ext_stream_give(h->stream, h->ext_ev_out, caller_stream)); return DRIL_OK; }
}  // namespace dril::ppo
namespace {
// the adapter's table of a Box handle as the actions-out kernel takes it (null: Discrete, or nothing to clamp)
const ExtBounds* ext_bounds_for(dril_handle* h, ExtBounds& scalar) {
    if (h->discrete) return nullptr;
    if (h->ext_bounds_set) return &h->ext_bounds;
    if (!(h->cfg.ext_action_low < h->cfg.ext_action_high)) return nullptr;
    for (int a = 0; a < h->A; ++a) { scalar.lo[a] = h->cfg.ext_action_low; scalar.hi[a] = h->cfg.ext_action_high; }
    return &scalar;
}

// a wrapper of dril_ext_normalize_enable / dril_ext_monitor_enable is on (dril_wrap.hip): the device verbs honour it, the host verbs refuse
bool xw_on(const dril_handle* h) { return h->pn.on || h->ext_mon_window > 0; }
#define XW_HOST_REFUSED(h, what) do { if (xw_on(h)) return fail(h, DRIL_ERR_UNSUPPORTED, what ": wrapper on: use the device verbs, or wrap the host env on the host (dril_ext_normalize_enable / dril_ext_monitor_enable are honoured by dril_ext_act_device / _record_device / _finish_device only)"); } while (0)
}  // namespace
// ---- collect_trajectories over HOST envs (DRIL_ENV_EXTERNAL), trajectory.jl:22-78: the caller steps its envs, the device does the rest ----
DRIL_EXPORT int32_t dril_ext_act(dril_handle* h, const float* obs, void* raw_actions, void* env_actions) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_act: the handle was not created with DRIL_ENV_EXTERNAL");
    XW_HOST_REFUSED(h, "dril_ext_act");
    if (!obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act: null obs");
    if (h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act: the previous step has no dril_ext_record yet");
    if (h->ext_t >= h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act: n_steps env steps are recorded; call dril_ext_finish");
    const size_t E = h->cfg.n_envs, D = h->D, A = h->A, ab = act_bytes_per(h), k = (size_t)h->ext_t * E;
    ext_count_begin(h); const int64_t l0 = h->gws.launches;
    HIPCHK(h, hipMemcpyAsync(h->obs + k * D, obs, E * D * 4, hipMemcpyHostToDevice, h->stream));                          // observation -> buffer, :46-47
    const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * A)) : nullptr;
    PolicyArgs p = policy_args(h, h->obs + k * D, (int64_t)E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);     // get_action_and_values :41; raw action stored :48
    HIPCHK(h, run_policy(h, p));
    h->policy_calls += 1;
    void* first = raw_actions ? raw_actions : env_actions;                             // one device-to-host copy; the second output is a host copy of it
    if (first) HIPCHK(h, hipMemcpyAsync(first, (char*)h->act + k * ab, E * ab, hipMemcpyDeviceToHost, h->stream));
    h->ext_launches += h->gws.launches - l0;
    int rc = sync(h); if (rc) return rc;
    h->ext_syncs += 1;
    if (raw_actions && env_actions) std::memcpy(env_actions, raw_actions, E * ab);
    if (env_actions && !h->discrete && h->ext_bounds_set) {                                                               // the per-dimension table of dril_ext_set_action_bounds
        float* a = (float*)env_actions;
        for (size_t i = 0; i < E * A; ++i) { const float lo = h->ext_bounds.lo[i % A], hi = h->ext_bounds.hi[i % A]; if (lo < hi) a[i] = a[i] < lo ? lo : (a[i] > hi ? hi : a[i]); }
    } else
    if (env_actions && !h->discrete && h->cfg.ext_action_low < h->cfg.ext_action_high) {                                  // to_env(ClampAdapter) :42, default_adapters.jl:4-11; E * A floats, on the host
        float* a = (float*)env_actions; const float lo = h->cfg.ext_action_low, hi = h->cfg.ext_action_high;
        for (size_t i = 0; i < E * A; ++i) a[i] = a[i] < lo ? lo : (a[i] > hi ? hi : a[i]);
    }
    h->ext_acted = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_record(dril_handle* h, const float* rewards, const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_record: the handle was not created with DRIL_ENV_EXTERNAL");
    XW_HOST_REFUSED(h, "dril_ext_record");
    if (!rewards || !terminated || !truncated) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record: null rewards / terminated / truncated");
    if (!h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record without a preceding dril_ext_act");
    const size_t E = h->cfg.n_envs, D = h->D, k = (size_t)h->ext_t * E;
    float* srew = h->ext_stage_rew + k; uint8_t* fl = h->ext_stage_flags + k;     // this step's slot of the pinned staging area: not reused before the next rollout
    std::vector<int> tr;
    for (size_t e = 0; e < E; ++e) { fl[e] = (uint8_t)((terminated[e] ? 1 : 0) | (truncated[e] ? 2 : 0)); if (truncated[e]) tr.push_back((int)e); }
    if (!tr.empty() && !terminal_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record: truncated envs need terminal_obs (infos[i][\"terminal_observation\"], multithreadedParallelEnv.jl:64-66)");
    std::memcpy(srew, rewards, E * 4);
    HIPCHK(h, hipMemcpyAsync(h->rew + k, srew, E * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->flags + k, fl, E, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->boot + k, 0, E * 4, h->stream));
    if (!tr.empty()) {                                                                // V(terminal_observation) of the truncated envs only, trajectory.jl:57-61
        const size_t n = tr.size();
        std::vector<float> tobs(n * D), bv(n), row(E, 0.f);
        for (size_t j = 0; j < n; ++j) std::memcpy(&tobs[j * D], terminal_obs + (size_t)tr[j] * D, D * 4);
        HIPCHK(h, hipMemcpyAsync(h->e_tobs, tobs.data(), n * D * 4, hipMemcpyHostToDevice, h->stream));
        PolicyArgs p = policy_args(h, h->e_tobs, (int64_t)n, nullptr, nullptr, h->e_rew, nullptr, nullptr, 2);
        const int64_t l0 = h->gws.launches;
        HIPCHK(h, run_policy(h, p));
        h->ext_launches += h->gws.launches - l0;
        HIPCHK(h, hipMemcpyAsync(bv.data(), h->e_rew, n * 4, hipMemcpyDeviceToHost, h->stream));
        int rc = sync(h); if (rc) return rc;                                          // host temporaries: drain before they go out of scope
        for (size_t j = 0; j < n; ++j) row[tr[j]] = bv[j];
        HIPCHK(h, hipMemcpyAsync(h->boot + k, row.data(), E * 4, hipMemcpyHostToDevice, h->stream));
        rc = sync(h); if (rc) return rc;
        h->ext_syncs += 2;
    }
    // no truncation: nothing to wait for — the copies read the pinned slot and complete behind the next dril_ext_act
    h->ext_t += 1; h->ext_acted = false; h->ext_steps_host += 1;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_finish(dril_handle* h, const float* last_obs) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_finish: the handle was not created with DRIL_ENV_EXTERNAL");
    XW_HOST_REFUSED(h, "dril_ext_finish");
    if (!last_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish: null last_obs");
    if (h->ext_acted || h->ext_t != h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish: the rollout needs exactly n_steps act/record pairs");
    const size_t E = h->cfg.n_envs, D = h->D;
    HIPCHK(h, hipMemcpyAsync(h->e_obs, last_obs, E * D * 4, hipMemcpyHostToDevice, h->stream));
    PolicyArgs p = policy_args(h, h->e_obs, (int64_t)E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);          // V(new_obs) where the last step left the trajectory open, :65-70
    const int64_t l0 = h->gws.launches;
    HIPCHK(h, run_policy(h, p));
    h->ext_launches += h->gws.launches - l0 + 1;
    h->ext_t = 0; h->noise_set = false;
    int rc = compute_gae(h); if (rc) return rc;                                       // compute_advantages! + returns, rollout_buffer.jl:83-87
    return ext_finish_drain(h, "dril_ext_finish");
}
DRIL_EXPORT int32_t dril_ext_steps(const dril_handle* h) { return h ? h->ext_t : -1; }

// ---- the same three verbs on DEVICE arrays: no copy across PCIe, no drain before dril_ext_finish_device (include/dril_hip.h) ----
DRIL_EXPORT int32_t dril_ext_act_device(dril_handle* h, const float* d_obs, void* d_raw_actions, void* d_env_actions, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_act_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act_device: null obs");
    if (h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act_device: the previous step has no dril_ext_record yet");
    if (h->ext_t >= h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_act_device: n_steps env steps are recorded; call dril_ext_finish");
    const size_t E = h->cfg.n_envs, D = h->D, A = h->A, ab = act_bytes_per(h), k = (size_t)h->ext_t * E;
    int rc = ext_check_ptr(h, "dril_ext_act_device", "d_obs", d_obs, E * D * 4); if (rc) return rc;
    if (d_raw_actions) { rc = ext_check_ptr(h, "dril_ext_act_device", "d_raw_actions", d_raw_actions, E * ab); if (rc) return rc; }
    if (d_env_actions) { rc = ext_check_ptr(h, "dril_ext_act_device", "d_env_actions", d_env_actions, E * ab); if (rc) return rc; }
    ext_count_begin(h); const int64_t l0 = h->gws.launches;
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (h->pn.on) {                                                                   // the wrapper's observe: raw -> old_obs and the normalised row in one pass (no copy)
        int64_t added = 0;
        rc = xn_observe(h, d_obs, (int64_t)E, h->obs + k * D, true, &added); if (rc) return rc;
        h->ext_launches += added; h->xw_added[0] += added;
    } else
    HIPCHK(h, hipMemcpyAsync(h->obs + k * D, d_obs, E * D * 4, hipMemcpyDefault, h->stream));                               // observation -> buffer, :46-47
    const void* nz = h->noise_set ? (const void*)((const char*)h->noise_dev + k * (h->discrete ? 8 : 4 * A)) : nullptr;
    PolicyArgs p = policy_args(h, h->obs + k * D, (int64_t)E, nz, (char*)h->act + k * ab, h->val + k, h->logp + k, nullptr, 0);     // the host verb's forward: the same bits
    HIPCHK(h, run_policy(h, p));
    h->policy_calls += 1;
    h->ext_launches += h->gws.launches - l0;
    if (d_raw_actions || d_env_actions) {                                                                                   // to_env(ClampAdapter) :42 on the device
        ExtBounds scalar; const ExtBounds* b = ext_bounds_for(h, scalar);
        HIPCHK(h, launch_ext_actions_out((char*)h->act + k * ab, d_raw_actions, d_env_actions, (int64_t)E, (int)A, h->discrete ? 1 : 0, b, h->stream));
        h->ext_launches += 1;
    }
    rc = ext_stream_leave(h, caller_stream); if (rc) return rc;
    h->ext_acted = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_record_device(dril_handle* h, const float* d_rewards, const uint8_t* d_terminated, const uint8_t* d_truncated, const float* d_terminal_obs, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_record_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_rewards || !d_terminated || !d_truncated) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record_device: null rewards / terminated / truncated");
    if (!h->ext_acted) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_record_device without a preceding dril_ext_act");
    const size_t E = h->cfg.n_envs, D = h->D, k = (size_t)h->ext_t * E;
    int rc = ext_check_ptr(h, "dril_ext_record_device", "d_rewards", d_rewards, E * 4); if (rc) return rc;
    rc = ext_check_ptr(h, "dril_ext_record_device", "d_terminated", d_terminated, E); if (rc) return rc;
    rc = ext_check_ptr(h, "dril_ext_record_device", "d_truncated", d_truncated, E); if (rc) return rc;
    if (d_terminal_obs) { rc = ext_check_ptr(h, "dril_ext_record_device", "d_terminal_obs", d_terminal_obs, E * D * 4); if (rc) return rc; }
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (xw_on(h)) {                                                                   // a wrapper on: act! of the wrapper and the record in one kernel, then V(normalised terminal_observation) selected into boot[t]
        const float* tobs_norm = nullptr; int64_t own = 0;
        rc = xn_record(h, k, d_rewards, d_terminated, d_truncated, d_terminal_obs, &tobs_norm, &own); if (rc) return rc;
        const int64_t l0 = h->gws.launches;
        if (tobs_norm) {
            PolicyArgs p = policy_args(h, tobs_norm, (int64_t)E, nullptr, nullptr, h->gen_tmp, nullptr, nullptr, 2);
            HIPCHK(h, run_policy(h, p));
            HIPCHK(h, generic_select((int64_t)E, d_truncated, h->gen_tmp, h->boot + k, h->stream));
            own += 1;
        }
        h->ext_launches += h->gws.launches - l0 + own; h->xw_added[1] += own - 1;      // (the unwrapped verb's one launch of its own is ext_record_kernel)
        rc = ext_stream_leave(h, caller_stream); if (rc) return rc;
        h->ext_t += 1; h->ext_acted = false; h->ext_steps_dev += 1;
        return DRIL_OK;
    }
    if (d_terminal_obs) {                                                             // V(terminal_observation), trajectory.jl:57-61: the critic over all E columns, kept where truncated
        const int64_t l0 = h->gws.launches;
        PolicyArgs p = policy_args(h, d_terminal_obs, (int64_t)E, nullptr, nullptr, h->gen_tmp, nullptr, nullptr, 2);
        HIPCHK(h, run_policy(h, p));
        h->ext_launches += h->gws.launches - l0;
    }
    HIPCHK(h, launch_ext_record((int)E, d_rewards, d_terminated, d_truncated, d_terminal_obs ? h->gen_tmp : nullptr, h->rew + k, h->flags + k, h->boot + k, h->ext_err, h->stream));
    h->ext_launches += 1;
    rc = ext_stream_leave(h, caller_stream); if (rc) return rc;
    h->ext_t += 1; h->ext_acted = false; h->ext_steps_dev += 1;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_finish_device(dril_handle* h, const float* d_last_obs, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_finish_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_last_obs) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish_device: null last_obs");
    if (h->ext_acted || h->ext_t != h->cfg.n_steps) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_finish_device: the rollout needs exactly n_steps act/record pairs");
    const size_t E = h->cfg.n_envs, D = h->D;
    int rc = ext_check_ptr(h, "dril_ext_finish_device", "d_last_obs", d_last_obs, E * D * 4); if (rc) return rc;
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (h->pn.on) {                                                                   // one more observe of the wrapper
        int64_t added = 0;
        rc = xn_observe(h, d_last_obs, (int64_t)E, h->e_obs, true, &added); if (rc) return rc;
        h->ext_launches += added; h->xw_added[2] += added;
    } else
    HIPCHK(h, hipMemcpyAsync(h->e_obs, d_last_obs, E * D * 4, hipMemcpyDefault, h->stream));
    PolicyArgs p = policy_args(h, h->e_obs, (int64_t)E, nullptr, nullptr, h->last_values, nullptr, nullptr, 2);          // V(new_obs) where the last step left the trajectory open, :65-70
    const int64_t l0 = h->gws.launches;
    HIPCHK(h, run_policy(h, p));
    h->ext_launches += h->gws.launches - l0 + 1;
    h->ext_t = 0; h->noise_set = false;
    rc = compute_gae(h); if (rc) return rc;                                           // compute_advantages! + returns, rollout_buffer.jl:83-87
    if (h->ext_mon_window > 0) {                                                      // MonitorWrapperEnv: this rollout's finished episodes enter the window in (step, env) order
        HIPCHK(h, launch_monitor_collect(h->flags, h->ep_ret, h->ep_len, h->cfg.n_envs, h->cfg.n_steps, h->ext_mon_window, h->mon_cnt, h->mon_ring_ret, h->mon_ring_len, h->mon_meta, h->stream));
        h->ext_launches += 2; h->xw_added[2] += 2;                                    // (its count and its collect kernel)
    }
    return ext_finish_drain(h, "dril_ext_finish_device");                             // the drain covers the read of d_last_obs: nothing for caller_stream to wait for
}
DRIL_EXPORT int32_t dril_predict_actions_device(dril_handle* h, const float* d_obs, int64_t batch, int32_t deterministic, void* d_raw_actions, void* d_env_actions, void* caller_stream) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_predict_actions_device: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!d_obs || batch < 1) return fail(h, DRIL_ERR_INVALID_ARG, "dril_predict_actions_device: null obs or batch < 1");
    if (!d_raw_actions && !d_env_actions) return fail(h, DRIL_ERR_INVALID_ARG, "dril_predict_actions_device: null actions");
    const size_t B = (size_t)batch, ab = act_bytes_per(h);
    int rc = ext_check_ptr(h, "dril_predict_actions_device", "d_obs", d_obs, B * h->D * 4); if (rc) return rc;
    if (d_raw_actions) { rc = ext_check_ptr(h, "dril_predict_actions_device", "d_raw_actions", d_raw_actions, B * ab); if (rc) return rc; }
    if (d_env_actions) { rc = ext_check_ptr(h, "dril_predict_actions_device", "d_env_actions", d_env_actions, B * ab); if (rc) return rc; }
    HIPCHK(h, h->ext_pred_act.grow(B * ab)); HIPCHK(h, h->ext_pred_lp.grow(B));           // grow-only scratch: the head kernel's actions and log-probabilities (a free waits for the device)
    const bool nz_eval = h->pn.on && h->pn.cfg.norm_obs;                               // evaluation under the wrapper: the statistics in force, never updated
    if (nz_eval && batch > h->cfg.n_envs) {                                            // (up to n_envs rows fit e_obs; more: grow-only scratch, counted by dril_ext_wrap_info)
        bool grew; HIPCHK(h, h->ext_pred_obs.grow(B * h->D, &grew));
        if (grew) h->xw_allocs += 1;
    }
    rc = ext_stream_enter(h, caller_stream); if (rc) return rc;
    if (nz_eval) {
        float* scratch = batch > h->cfg.n_envs ? h->ext_pred_obs : h->e_obs; int64_t added = 0;
        rc = xn_observe(h, d_obs, batch, scratch, false, &added); if (rc) return rc;
        d_obs = scratch;
    }
    PolicyArgs a = policy_args(h, d_obs, batch, nullptr, h->ext_pred_act, nullptr, h->ext_pred_lp, nullptr, 0);
    a.deterministic = deterministic ? 1 : 0;
    HIPCHK(h, run_policy(h, a));
    h->policy_calls += 1;
    ExtBounds scalar; const ExtBounds* b = ext_bounds_for(h, scalar);
    HIPCHK(h, launch_ext_actions_out(h->ext_pred_act, d_raw_actions, d_env_actions, batch, h->A, h->discrete ? 1 : 0, b, h->stream));
    return ext_stream_leave(h, caller_stream);
}
DRIL_EXPORT int32_t dril_ext_set_action_bounds(dril_handle* h, const float* low, const float* high) {
    NEED(h);
    if (!h->external) return fail(h, DRIL_ERR_UNSUPPORTED, "dril_ext_set_action_bounds: the handle was not created with DRIL_ENV_EXTERNAL");
    if (h->discrete) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_set_action_bounds: a Discrete action space has no bounds to clamp to");
    if (!low && !high) { h->ext_bounds_set = false; return DRIL_OK; }
    if (!low || !high) return fail(h, DRIL_ERR_INVALID_ARG, "dril_ext_set_action_bounds: null low / high");
    for (int a = 0; a < h->A; ++a) { h->ext_bounds.lo[a] = low[a]; h->ext_bounds.hi[a] = high[a]; }
    h->ext_bounds_set = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_ext_device_info(const dril_handle* h, struct dril_ext_device_info* out) {
    if (!h) return fail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    if (!out) return DRIL_ERR_INVALID_ARG;
    if (!h->external) return DRIL_ERR_UNSUPPORTED;
    std::memset(out, 0, sizeof(*out));
    out->steps_device = h->ext_steps_dev; out->steps_host = h->ext_steps_host; out->host_syncs = h->ext_syncs; out->per_dim_bounds = h->ext_bounds_set ? 1 : 0;
    out->launches = h->ext_launches;
    return DRIL_OK;
}
