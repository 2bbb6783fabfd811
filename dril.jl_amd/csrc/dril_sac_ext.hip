// dril_sac_ext.hip — the verbs of a DRIL_ENV_EXTERNAL SAC handle (include/dril_sac.h): dril_sac_ext_push on host arrays; the sync-free loop on device arrays
// (dril_sac_ext_act_device, dril_sac_predict_actions_device, dril_sac_ext_push_device, dril_sac_update_enqueue, dril_sac_flush) with its kernels; NormalizeWrapperEnv
// and MonitorWrapperEnv around such a handle's envs (dril_sac_ext_normalize_*, dril_sac_ext_monitor_*, dril_sac_ext_collection_begin, dril_sac_ext_wrap_info).
// The units: dril_sac_handle.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "dril_sac_handle.h"
#include "dril_ext_stream.h"     // the pointer rule and the stream hand-over of the device-array verbs, shared with the PPO handle
#include "dril_sac_ext_norm.h"   // NormalizeWrapperEnv / MonitorWrapperEnv on such a handle: the act and push apply kernels

using namespace dril;
using namespace dril::sac;

// one env step of the caller's host envs into the ring: the same push kernel as the device collection (truncated envs store their terminal observation)
DRIL_EXPORT int32_t dril_sac_ext_push(dril_sac_handle* h, const float* obs, const float* stored_actions, const float* rewards, const uint8_t* terminated,
                                      const uint8_t* truncated, const float* next_obs, const float* terminal_obs) {
    SNEED(h);
    if (h->env.module) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_ext_push: the env of a device env plug-in (DRIL_ENV_MODULE) is on the device, not on the host: dril_sac_collect_rollout steps it");
    if (!h->external) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_ext_push: the handle was not created with DRIL_ENV_EXTERNAL");
    if (!obs || !stored_actions || !rewards || !terminated || !truncated || !next_obs) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_push: null pointer");
    if (h->ext_acted) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_push: a dril_sac_ext_act_device step is pending; dril_sac_ext_push_device completes it");
    if (h->nz.on || h->mon_window) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_ext_push: wrapper on: use the device verbs, or wrap the host env on the host (dril_sac_ext_normalize_enable / dril_sac_ext_monitor_enable are honoured by dril_sac_ext_act_device / _push_device only)");
    const size_t E = h->cfg.n_envs, D = h->D, A = h->A;
    bool any_trunc = false; for (size_t e = 0; e < E; ++e) any_trunc = any_trunc || truncated[e] != 0;
    if (any_trunc && !terminal_obs) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_push: truncated envs need terminal_obs");
    SHIP(h, hipMemcpyAsync(h->obs_cur, obs, E * D * 4, hipMemcpyHostToDevice, h->stream));
    SHIP(h, hipMemcpyAsync(h->obs_nxt, next_obs, E * D * 4, hipMemcpyHostToDevice, h->stream));
    SHIP(h, hipMemcpyAsync(h->e_raw, stored_actions, E * A * 4, hipMemcpyHostToDevice, h->stream));
    SHIP(h, hipMemcpyAsync(h->e_rew, rewards, E * 4, hipMemcpyHostToDevice, h->stream));
    SHIP(h, hipMemcpyAsync(h->e_term, terminated, E, hipMemcpyHostToDevice, h->stream));
    SHIP(h, hipMemcpyAsync(h->e_trunc, truncated, E, hipMemcpyHostToDevice, h->stream));
    if (any_trunc) SHIP(h, hipMemcpyAsync(h->e_tobs, terminal_obs, E * D * 4, hipMemcpyHostToDevice, h->stream));
    const long long tail = (h->head + h->size) % h->cap;
    PushArgs pa{(int)E, (int)D, (int)A, h->cap, tail, h->obs_cur, h->e_raw, h->e_rew, h->e_tobs, h->obs_nxt, h->e_term, h->e_trunc,
                h->rb_obs, h->rb_next, h->rb_act, h->rb_rew, h->rb_term, h->rb_trunc};
    launch_push(h, pa);
    SHIP(h, hipGetLastError());
    const long long over = h->size + (long long)E - h->cap;                                       // CircularBuffer: overwrite the oldest
    if (over > 0) { h->head = (h->head + over) % h->cap; h->size = h->cap; } else h->size += (long long)E;
    h->ext_steps_host += 1;
    return ssync(h);                                                                              // the caller's arrays are pageable host memory: drain before returning
}

// ---- the same loop on DEVICE arrays: nothing below waits on the host except dril_sac_flush (include/dril_sac.h) --------------------------------------------
#define S_EXTERNAL_ONLY(h, verb) do { if (!(h)->external) return sfail(h, DRIL_ERR_UNSUPPORTED, verb ": the handle was not created with DRIL_ENV_EXTERNAL"); } while (0)
namespace {
// ---- the device-array verbs of a DRIL_ENV_EXTERNAL handle (dril_sac_ext_act_device / dril_sac_predict_actions_device / dril_sac_ext_push_device) ------------
// Head of the device act, one launch behind the actor forward: the noise draw (the words sac_noise_fill_kernel would have written to a buffer, computed in the
// thread that uses them), the squashed sample (squashed_sample_logp: sac_squash_eval_kernel's own expression, so its bits), TanhScaleAdapter — or, mode 2, the
// uniform branch rand(action_space) — and the writes into the caller's arrays and the handle's pending-action rows.  One thread per row: A <= kMaxA floats per
// thread, n x A <= a few hundred KB in all; the launch is latency-bound, the point is that it is ONE launch and no copy.
// rand(rng, Box) of one dimension as __fadd_rn(low, __fmul_rn(u, __fsub_rn(high, low))): three float32 operations, each rounded on its own, which NumPy float32
// restates to the bit.  Spelled with plain operators under contract(off): this toolchain's __fmul_rn / __fadd_rn ARE plain operators compiled with contraction
// allowed, and the pair became one v_fmac_f32 (a single rounding) when the intrinsics were used
__device__ __forceinline__ float ext_rand_box_rn(float u, float lo, float hi) {
#pragma clang fp contract(off)
    const float w = hi - lo;
    const float p = u * w;
    return lo + p;
}
struct ExtHeadArgs {
    int n, A, mode;                                   // mode 0: sample, 1: deterministic (tanh(mean)), 2: rand(action_space)
    const float* mu; const float* log_std; const float* noise;   // noise null: the handle's stream (rng)
    SacRng rng; const float* low; const float* high;
    float* stored; float* envact; float* keep;        // the caller's arrays (either may be null) and the handle's e_raw (null: predict only)
};
__global__ __launch_bounds__(256) void sac_ext_head_kernel(ExtHeadArgs g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    const int A = g.A;
    float nz[kMaxA], a_[kMaxA], ev[kMaxA];
    if (g.mode == 2) {
        for (int a = 0; a < A; ++a) {
            float u;
            if (g.noise) u = g.noise[(size_t)i * A + a];
            else {                                                                                // the uniform of the word pair sac_noise(rng, 8, i, a) turns into a normal
                uint32_t o[4];
                philox4x32_10((uint32_t)g.rng.key, (uint32_t)(g.rng.key >> 32), (uint32_t)g.rng.u, (uint32_t)(g.rng.u >> 32), 8u, (uint32_t)(i * 4 + a / 2), o);
                u = u01_f32((a & 1) ? o[2] : o[0]);
            }
            const float lo = g.low[a], hi = g.high[a];
            a_[a] = ext_rand_box_rn(u, lo, hi);
            ev[a] = a_[a];
        }
    } else {
        float ls[kMaxA], gg[kMaxA];
        for (int a = 0; a < A; ++a) { ls[a] = g.log_std[a]; nz[a] = g.mode == 1 ? 0.f : (g.noise ? g.noise[(size_t)i * A + a] : sac_noise(g.rng, 8, i, a)); }
        (void)squashed_sample_logp(g.mu + (size_t)i * A, ls, nz, A, a_, gg);
        for (int a = 0; a < A; ++a) ev[a] = sac_to_env(a_[a], g.low[a], g.high[a]);
    }
    for (int a = 0; a < A; ++a) {
        const size_t k = (size_t)i * A + a;
        if (g.keep) g.keep[k] = a_[a];
        if (g.stored) g.stored[k] = a_[a];
        if (g.envact) g.envact[k] = ev[a];
    }
}
// push! of the pending step from the caller's arrays: sac_push_block's flat (env, dim) walk over kPushEnvsPerBlock envs per workgroup.  A null tobs states "no env
// was truncated": the block then reads nobs in its place, and a truncated flag set all the same raises the sticky error word (a plain vector store of an int, as
// ext_record_kernel's; dril_sac_flush reads it after its drain)
__global__ __launch_bounds__(256) void sac_ext_push_kernel(PushArgs g, int* err) {
    const int e0 = blockIdx.x * kPushEnvsPerBlock, n = min(kPushEnvsPerBlock, g.E - e0);            // grid = ceil(E / kPushEnvsPerBlock): n >= 1
    if (!g.tobs) {
        if ((int)threadIdx.x < n && g.trunc[e0 + threadIdx.x]) *err = 1;
        g.tobs = g.nobs;
    }
    sac_push_block(g, e0, n);
}

constexpr int kPendingCap = DRIL_SAC_PENDING_CAPACITY;
// a wait inside the scope of one of these is counted (ssync): dril_sac_ext_device_info.host_syncs
struct DeviceVerbScope { dril_sac_handle* h; explicit DeviceVerbScope(dril_sac_handle* h_) : h(h_) { h->in_device_verb = true; } ~DeviceVerbScope() { h->in_device_verb = false; } };
// once the handle's stream has taken over from the caller's, EVERY way out of the verb hands it back: a step that fails half-way still leaves the caller's stream
// ordered behind what was already enqueued.  give() is the successful path (its status is the verb's); the destructor covers the early returns
struct StreamHandOver {
    dril_sac_handle* h; void* caller; bool given = false;
    StreamHandOver(dril_sac_handle* h_, void* caller_) : h(h_), caller(caller_) {}
    hipError_t give() { given = true; return ext_stream_give(h->stream, h->ext_ev_out, caller); }
    ~StreamHandOver() { if (!given && ext_stream_give(h->stream, h->ext_ev_out, caller) != hipSuccess) (void)hipGetLastError(); }
};
// cfg.profile_events: a pair of events of the handle's pool around what one act or push enqueues.  The scope takes the pair when the pool (created with the handle)
// has one left — a call made while it is full is not timed, nothing is ever created here — and a verb that fails between its two marks gives the pair back, so the
// pool always holds whole pairs
struct XpScope {
    dril_sac_handle* h; size_t n0; bool on, ok = false;
    explicit XpScope(dril_sac_handle* h_) : h(h_), n0(h_->xp_n), on(h_->xp_n + 2 <= h_->xp_events.size()) {}
    hipError_t mark() { if (!on) return hipSuccess; const hipError_t e = hipEventRecord(h->xp_events[h->xp_n], h->stream); if (e == hipSuccess) h->xp_n += 1; return e; }
    ~XpScope() { if (!ok) h->xp_n = n0; }
};
int sac_check_ptr(dril_sac_handle* h, const char* verb, const char* name, const void* p, size_t bytes) {
    const std::string msg = ext_ptr_problem(h->cfg.device, verb, name, p, bytes);
    return msg.empty() ? DRIL_OK : sfail(h, DRIL_ERR_INVALID_ARG, msg);
}
// actor means of n rows already in `x` (device), then the head: net_forward is the call dril_sac_predict_actions makes (actor_chunk), so the means are its bits
int actor_device_rows(dril_sac_handle* h, const float* x, int n, int mode, const float* d_noise, float* stored, float* envact, float* keep) {
    if (mode != 2) { const int64_t l0 = h->fwd_launches; SDO(net_forward(h, h->params, h->actor, 0, h->D, h->A, x, h->D, 0, n, actor_bufs(h), 1)); h->ext_launches += h->fwd_launches - l0; }
    SacRng rng{0, 0};
    if (mode != 1 && !d_noise) rng = SacRng{h->cfg.seed ^ 0x0b5e55edull, h->aux_counter++};       // the handle's stream: one counter per chunk, as actor_chunk (taken once the forward is enqueued: a failed call leaves the stream's position alone)
    ExtHeadArgs g{n, h->A, mode, h->mu, h->params + h->log_std_off, d_noise, rng, h->act_bounds, h->act_bounds + kMaxA, stored, envact, keep};
    hipLaunchKernelGGL(sac_ext_head_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, g);
    SHIP(h, hipGetLastError());
    h->ext_launches += 1;
    return DRIL_OK;
}
// ---- the wrappers of an external handle inside the device verbs (kernels: dril_sac_ext_norm.h) ----
int xs_epb(int n, int D) { return std::max(std::min(64, std::max(1, 2048 / D)), (n + 127) / 128); }   // (nz_apply's split: a block's share of the rows)
// observe (:123-137) of n rows of the caller's array into `out`, in the place of the unwrapped verb's device-to-device copy.  opening: a collection's first act — the
// one observe that updates the statistics (one more launch: the moments); cache: the wrapper's old_obs takes the rows (not for predict)
int xw_observe(dril_sac_handle* h, const float* raw, int n, float* out, bool opening, bool cache) {
    const bool upd = opening && h->nz.cfg.training && h->nz.cfg.norm_obs;
    int rows = 0;
    if (upd) { SDO(nz_moments_over(h, raw, nullptr, &rows)); h->ext_launches += 1; h->xw_launches_act += 1; }
    XsActArgs p{}; NormWrapArgs& a = p.w;
    h->nz.fill(a, upd, false, h->cfg.n_envs);
    a.E = n; a.rows = rows; a.epb = xs_epb(n, h->D); a.raw = raw; a.obs_out = out; p.old_obs = cache ? h->nz_old_obs : nullptr;
    hipLaunchKernelGGL(sac_ext_norm_act_kernel, dim3((n + a.epb - 1) / a.epb), dim3(256), nz_apply_lds(h->D), h->stream, p);
    SHIP(h, hipGetLastError());
    h->nz.commit(a); h->ext_launches += 1;
    return DRIL_OK;
}
// act! + observe + push! of the pending step under a wrapper, in the place of sac_ext_push_kernel: the moments over the caller's next observations and rewards (ONE
// launch, only where statistics are updated), then the apply-and-push kernel.  The monitor's block of buffered steps is collected first when it is full
int xw_push(dril_sac_handle* h, const PushArgs& pa, const float* d_terminal_obs) {
    const bool nzon = h->nz.on, upd_obs = nzon && h->nz.cfg.training && h->nz.cfg.norm_obs, upd_ret = nzon && h->nz.cfg.training && h->nz.cfg.norm_reward;
    const int E = h->cfg.n_envs, D = h->D;
    int rows = 0;
    if (upd_obs || upd_ret) { SDO(nz_moments_over(h, upd_obs ? pa.nobs : nullptr, upd_ret ? pa.rew : nullptr, &rows)); h->ext_launches += 1; h->xw_launches_push += 1; }
    if (h->mon_window && h->mon_row >= h->mon_rows_cap) { SDO(monitor_end(h)); h->ext_launches += 1; h->xw_launches_push += 1; }
    XsPushArgs p{}; NormWrapArgs& a = p.w;
    if (nzon) h->nz.fill(a, upd_obs, upd_ret, E); else a.D = D;
    a.E = E; a.rows = rows; a.epb = xs_epb(E, D); a.raw = pa.nobs; a.rew = pa.rew; a.term = pa.term; a.trunc = pa.trunc; a.returns = h->nz_returns;
    p.has_norm = nzon ? 1 : 0; p.tobs = d_terminal_obs; p.old_obs = h->nz_old_obs; p.old_rew = h->nz_old_rew; p.push = pa; p.err = h->ext_err;
    const MonitorArgs m = monitor_row(h);
    p.mon_cur_ret = m.cur_ret; p.mon_cur_len = m.cur_len; p.ep_ret = m.ep_ret; p.ep_len = m.ep_len; p.ep_flags = m.flags_out;
    hipLaunchKernelGGL(sac_ext_norm_push_kernel, dim3((E + a.epb - 1) / a.epb), dim3(256), nzon ? xs_push_lds(D) : 0, h->stream, p);
    SHIP(h, hipGetLastError());
    if (nzon) h->nz.commit(a);
    if (h->mon_window) h->mon_row += 1;
    h->ext_launches += 1;
    return DRIL_OK;
}
}  // namespace
DRIL_EXPORT int32_t dril_sac_ext_act_device(dril_sac_handle* h, const float* d_obs, int32_t use_random_actions, const float* d_noise, float* d_stored_actions,
                                            float* d_env_actions, void* caller_stream) {
    SNEED(h); S_EXTERNAL_ONLY(h, "dril_sac_ext_act_device");
    if (!d_obs) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_act_device: null obs");
    if (h->ext_acted) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_act_device: the previous step has no dril_sac_ext_push_device yet");
    const size_t E = h->cfg.n_envs, D = h->D, A = h->A;
    SDO(sac_check_ptr(h, "dril_sac_ext_act_device", "d_obs", d_obs, E * D * 4));
    if (d_noise) SDO(sac_check_ptr(h, "dril_sac_ext_act_device", "d_noise", d_noise, E * A * 4));
    if (d_stored_actions) SDO(sac_check_ptr(h, "dril_sac_ext_act_device", "d_stored_actions", d_stored_actions, E * A * 4));
    if (d_env_actions) SDO(sac_check_ptr(h, "dril_sac_ext_act_device", "d_env_actions", d_env_actions, E * A * 4));
    if (h->nz.on && !h->xw_begin && !h->xw_live)
        return sfail(h, DRIL_ERR_NOT_INITIALISED, "dril_sac_ext_act_device: no collection is in progress under NormalizeWrapperEnv (wrapper switched, statistics set or wrapper reset since the last step): dril_sac_ext_collection_begin marks the act that opens one");
    DeviceVerbScope scope(h);
    SHIP(h, ext_stream_take(h->stream, h->ext_ev_in, caller_stream));
    StreamHandOver back(h, caller_stream);
    XpScope xp(h); SHIP(h, xp.mark());
    if (h->nz.on) {                                                                                // observe through the wrapper: normalised into obs_cur, raw into old_obs, from one read
        SDO(xw_observe(h, d_obs, (int)E, h->obs_cur, h->xw_begin, true));
        h->xw_begin = false; h->xw_live = true;
    } else {
        SHIP(h, hipMemcpyAsync(h->obs_cur, d_obs, E * D * 4, hipMemcpyDeviceToDevice, h->stream)); // the pending step's observation; the forward reads it from here
        h->ext_launches += 1;
    }
    SDO(actor_device_rows(h, h->obs_cur, (int)E, use_random_actions ? 2 : 0, d_noise, d_stored_actions, d_env_actions, h->e_raw));
    SHIP(h, xp.mark()); xp.ok = true;
    SHIP(h, back.give());
    h->ext_acted = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_predict_actions_device(dril_sac_handle* h, const float* d_obs, int64_t batch, int32_t deterministic, const float* d_noise,
                                                    float* d_raw_actions, float* d_env_actions, void* caller_stream) {
    SNEED(h); S_EXTERNAL_ONLY(h, "dril_sac_predict_actions_device");
    if (!d_obs || batch < 1) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_predict_actions_device: null obs or batch < 1");
    if (!d_raw_actions && !d_env_actions) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_predict_actions_device: null actions");
    const size_t B = (size_t)batch, D = h->D, A = h->A;
    SDO(sac_check_ptr(h, "dril_sac_predict_actions_device", "d_obs", d_obs, B * D * 4));
    if (d_noise) SDO(sac_check_ptr(h, "dril_sac_predict_actions_device", "d_noise", d_noise, B * A * 4));
    if (d_raw_actions) SDO(sac_check_ptr(h, "dril_sac_predict_actions_device", "d_raw_actions", d_raw_actions, B * A * 4));
    if (d_env_actions) SDO(sac_check_ptr(h, "dril_sac_predict_actions_device", "d_env_actions", d_env_actions, B * A * 4));
    DeviceVerbScope scope(h);
    SHIP(h, ext_stream_take(h->stream, h->ext_ev_in, caller_stream));
    StreamHandOver back(h, caller_stream);
    for (int64_t o = 0; o < batch; o += h->nmax) {                                                 // chunks of nmax rows, as the host verb: stream order keeps the scratch rows apart
        const int n = (int)std::min<int64_t>(h->nmax, batch - o);
        if (h->nz.on && h->nz.cfg.norm_obs) SDO(xw_observe(h, d_obs + o * D, n, h->xa, false, false));   // the statistics in force; nothing of the wrapper is written
        else { SHIP(h, hipMemcpyAsync(h->xa, d_obs + o * D, (size_t)n * D * 4, hipMemcpyDeviceToDevice, h->stream)); h->ext_launches += 1; }
        SDO(actor_device_rows(h, h->xa, n, deterministic ? 1 : 0, deterministic || !d_noise ? nullptr : d_noise + o * A,
                              d_raw_actions ? d_raw_actions + o * A : nullptr, d_env_actions ? d_env_actions + o * A : nullptr, nullptr));
    }
    SHIP(h, back.give());
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_push_device(dril_sac_handle* h, const float* d_rewards, const uint8_t* d_terminated, const uint8_t* d_truncated,
                                             const float* d_next_obs, const float* d_terminal_obs, void* caller_stream) {
    SNEED(h); S_EXTERNAL_ONLY(h, "dril_sac_ext_push_device");
    if (!d_rewards || !d_terminated || !d_truncated || !d_next_obs) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_push_device: null rewards / terminated / truncated / next_obs");
    if (!h->ext_acted) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_push_device without a preceding dril_sac_ext_act_device");
    const size_t E = h->cfg.n_envs, D = h->D;
    SDO(sac_check_ptr(h, "dril_sac_ext_push_device", "d_rewards", d_rewards, E * 4));
    SDO(sac_check_ptr(h, "dril_sac_ext_push_device", "d_terminated", d_terminated, E));
    SDO(sac_check_ptr(h, "dril_sac_ext_push_device", "d_truncated", d_truncated, E));
    SDO(sac_check_ptr(h, "dril_sac_ext_push_device", "d_next_obs", d_next_obs, E * D * 4));
    if (d_terminal_obs) SDO(sac_check_ptr(h, "dril_sac_ext_push_device", "d_terminal_obs", d_terminal_obs, E * D * 4));
    DeviceVerbScope scope(h);
    SHIP(h, ext_stream_take(h->stream, h->ext_ev_in, caller_stream));
    StreamHandOver back(h, caller_stream);
    XpScope xp(h); SHIP(h, xp.mark());
    const long long tail = (h->head + h->size) % h->cap;
    PushArgs pa{(int)E, (int)D, h->A, h->cap, tail, h->obs_cur, h->e_raw, d_rewards, d_terminal_obs, d_next_obs, d_terminated, d_truncated,
                h->rb_obs, h->rb_next, h->rb_act, h->rb_rew, h->rb_term, h->rb_trunc, nullptr};
    if (h->nz.on || h->mon_window) SDO(xw_push(h, pa, d_terminal_obs));
    else {
        hipLaunchKernelGGL(sac_ext_push_kernel, dim3((unsigned)((E + kPushEnvsPerBlock - 1) / kPushEnvsPerBlock)), dim3(256), 0, h->stream, pa, h->ext_err);
        SHIP(h, hipGetLastError());
        h->ext_launches += 1;
    }
    ring_advance(h);                                                                              // head / size are host counters: nothing to wait for
    SHIP(h, xp.mark()); xp.ok = true;
    SHIP(h, back.give());
    h->ext_acted = false; h->ext_steps_dev += 1;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_update_enqueue(dril_sac_handle* h, int32_t n_updates) {
    SNEED(h); S_EXTERNAL_ONLY(h, "dril_sac_update_enqueue");
    if (n_updates <= 0) return sfail(h, DRIL_ERR_INVALID_ARG, "n_updates must be positive");
    if (h->inj_updates && h->inj_updates != n_updates) return sfail(h, DRIL_ERR_INVALID_ARG, "injected batches were set for a different n_updates");
    if ((int64_t)h->pend_n + n_updates > kPendingCap)
        return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_update_enqueue: " + std::to_string(h->pend_n) + " pending + " + std::to_string(n_updates) + " new statistics rows exceed the pending table of " + std::to_string(kPendingCap) + ": flush first (dril_sac_flush)");
    if (h->size <= 0) return sfail(h, DRIL_ERR_NOT_INITIALISED, "the replay buffer is empty");
    const int nb = h->adam_blocks_c + h->end_blocks;
    DeviceVerbScope scope(h);
    const bool injected = h->inj_updates != 0;
    int rc = DRIL_OK;
    for (int k = 0; k < n_updates && rc == DRIL_OK; ++k) {
        const size_t row = (size_t)h->pend_n;
        rc = sac_one_update(h, injected ? k : -1, h->pend_stats + row * 8, nullptr, h->pend_ssq + row * nb);
        if (rc == DRIL_OK) h->pend_n += 1;
    }
    // the injected batches are read by launches still in flight: freeing them would wait for the device, so they go with the next flush
    if (h->inj_idx || h->inj_ne || h->inj_nn || h->inj_np) h->pend_free.push_back(dril_sac_handle::InjectedBatches{std::move(h->inj_idx), std::move(h->inj_ne), std::move(h->inj_nn), std::move(h->inj_np)});
    h->inj_updates = 0;
    return rc;
}
DRIL_EXPORT int32_t dril_sac_flush(dril_sac_handle* h, dril_sac_stats* stats, int64_t stats_capacity, int64_t* n_stats) {
    SNEED(h); S_EXTERNAL_ONLY(h, "dril_sac_flush");
    SDO(monitor_end(h));                                                                           // MonitorWrapperEnv (dril_sac_ext_monitor_enable): the episodes of the steps since the last collection into the window
    SHIP(h, hipMemcpyAsync(h->ext_err_host, h->ext_err, 4, hipMemcpyDeviceToHost, h->stream));
    SDO(ssync(h));
    h->ext_flushes += 1;
    for (size_t i = 0; i + 1 < h->xp_n; i += 2) { float ms = 0; if (hipEventElapsedTime(&ms, h->xp_events[i], h->xp_events[i + 1]) == hipSuccess) h->collect_ms += ms; }   // cfg.profile_events: an act and a push per env step
    h->collect_steps += (int64_t)(h->xp_n / 4); h->xp_n = 0;                                       // (a step = an act and a push: four events)
    h->pend_free.clear();
    const int n = h->pend_n;
    if (n_stats) *n_stats = n;
    if (n > 0 && stats && stats_capacity > 0) {
        std::vector<dril_sac_stats> tmp((size_t)n);
        SDO(fetch_stats(h, n, tmp.data(), h->pend_stats, h->pend_ssq));
        for (int64_t k = 0; k < std::min<int64_t>(stats_capacity, n); ++k) stats[k] = tmp[(size_t)k];
    }
    h->pend_n = 0;
    if (*h->ext_err_host) {
        *h->ext_err_host = 0;
        SHIP(h, hipMemsetAsync(h->ext_err, 0, 4, h->stream));
        return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_flush: a dril_sac_ext_push_device call had truncated envs and terminal_obs == NULL (infos[i][\"terminal_observation\"], off_policy_collection.jl:75-79); the rows of that push stay in the ring with next_obs in its place");
    }
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_set_action_bounds(dril_sac_handle* h, const float* low, const float* high) {
    SNEED(h); S_EXTERNAL_ONLY(h, "dril_sac_ext_set_action_bounds");
    if (!low || !high) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_set_action_bounds: null low / high");
    float tb[2 * kMaxA];
    for (int a = 0; a < kMaxA; ++a) { tb[a] = h->act_lo; tb[kMaxA + a] = h->act_hi; }
    for (int a = 0; a < h->A; ++a) {
        if (!std::isfinite(low[a]) || !std::isfinite(high[a]) || !(low[a] < high[a]))
            return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_set_action_bounds: dimension " + std::to_string(a) + " needs finite bounds with low < high (TanhScaleAdapter, default_adapters.jl:13-21)");
        tb[a] = low[a]; tb[kMaxA + a] = high[a];
    }
    SDO(ssync(h));                                                                                 // launches in flight read the table
    SHIP(h, hipMemcpy(h->act_bounds, tb, sizeof(tb), hipMemcpyHostToDevice));
    h->ext_bounds_set = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_device_info(const dril_sac_handle* h, struct dril_sac_ext_device_info* out) {
    if (!h) return sfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    dril_sac_handle* hm = const_cast<dril_sac_handle*>(h);                                         // (the message slot only)
    if (!out) return sfail(hm, DRIL_ERR_INVALID_ARG, "dril_sac_ext_device_info: null out pointer");
    if (!h->external) return sfail(hm, DRIL_ERR_UNSUPPORTED, "dril_sac_ext_device_info: the handle was not created with DRIL_ENV_EXTERNAL");
    std::memset(out, 0, sizeof(*out));
    out->steps_device = h->ext_steps_dev; out->steps_host = h->ext_steps_host; out->host_syncs = h->ext_syncs; out->flushes = h->ext_flushes; out->launches = h->ext_launches;
    out->pending_updates = h->pend_n; out->pending_capacity = kPendingCap; out->per_dim_bounds = h->ext_bounds_set ? 1 : 0;
    return DRIL_OK;
}

// the same for the device-resident envs of an external handle (dril_sac_ext_monitor_enable): the episodes of the steps pushed since the last collection enter the window first
DRIL_EXPORT int32_t dril_sac_ext_monitor_get_stats(dril_sac_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes) {
    SNEED(h);
    if (!h->external) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_ext_monitor_get_stats: the handle was not created with DRIL_ENV_EXTERNAL: the wrapper around device envs is dril_sac_monitor_enable / dril_sac_monitor_get_stats");
    if (!h->mon_window) return sfail(h, DRIL_ERR_NOT_INITIALISED, "dril_sac_ext_monitor_get_stats: MonitorWrapperEnv is off (dril_sac_ext_monitor_enable has not been called with a window >= 1)");
    SDO(monitor_end(h));
    return monitor_read(h, ep_rew_mean, ep_len_mean, n_episodes);
}
DRIL_EXPORT int32_t dril_sac_ext_wrap_info(const dril_sac_handle* h, struct dril_sac_ext_wrap_info* out) {
    if (!h) return sfail(nullptr, DRIL_ERR_NOT_INITIALISED, "null handle");
    dril_sac_handle* hm = const_cast<dril_sac_handle*>(h);                            // (the message slot only)
    if (!out) return sfail(hm, DRIL_ERR_INVALID_ARG, "dril_sac_ext_wrap_info: null out pointer");
    if (!h->external) return sfail(hm, DRIL_ERR_UNSUPPORTED, "dril_sac_ext_wrap_info: the handle was not created with DRIL_ENV_EXTERNAL");
    std::memset(out, 0, sizeof(*out));
    out->normalize_on = h->nz.on ? 1 : 0; out->monitor_on = h->mon_window > 0 ? 1 : 0; out->monitor_window = h->mon_window;
    out->launches_act = h->xw_launches_act; out->launches_push = h->xw_launches_push; out->allocations = 0;   // (structural: see the header)
    return DRIL_OK;
}

// ---- NormalizeWrapperEnv / MonitorWrapperEnv around the device-resident envs of an external handle (include/dril_sac.h; the device verbs honour them: xw_observe / xw_push) ----
#define XW_KIND(h, verb, twin) do { if (!(h)->external) return sfail(h, DRIL_ERR_UNSUPPORTED, verb ": the handle was not created with DRIL_ENV_EXTERNAL: the wrapper around device envs is " twin); } while (0)
#define XN_ON(h, verb) do { XW_KIND(h, verb, "dril_sac_normalize_enable"); \
    if (!(h)->nz.on) return sfail(h, DRIL_ERR_NOT_INITIALISED, verb ": NormalizeWrapperEnv is off (dril_sac_ext_normalize_enable has not been called with a configuration)"); } while (0)
#define XW_NO_PENDING_ACT(h, verb) do { if ((h)->ext_acted) return sfail(h, DRIL_ERR_INVALID_ARG, verb ": a dril_sac_ext_act_device step is pending: switch wrappers between env steps (after dril_sac_ext_push_device)"); } while (0)
DRIL_EXPORT int32_t dril_sac_ext_normalize_enable(dril_sac_handle* h, const dril_sac_normalize_config* cfg) {
    SNEED(h); XW_KIND(h, "dril_sac_ext_normalize_enable", "dril_sac_normalize_enable");
    dril_normalize_config c{};
    if (cfg) {
        memcpy(&c, cfg, sizeof(c));
        if (const NormErr err = norm_config_check(c, h->D)) return sfail(h, err.code, "dril_sac_ext_normalize_enable: " + err.msg);
        c = norm_config_canonical(c);
    }
    XW_NO_PENDING_ACT(h, "dril_sac_ext_normalize_enable");
    if (!cfg) {
        if (!h->nz.on) return DRIL_OK;
        SDO(ssync(h)); normalize_free(h); h->xw_begin = h->xw_live = false;
        return DRIL_OK;
    }
    if (h->nz.keeps(c)) return DRIL_OK;                                                // the same wrapper again (training apart, which is set): its statistics, returns and collection stay
    SDO(ssync(h));
    normalize_free(h);
    const hipError_t e = normalize_alloc(h, kNzMaxRows);
    if (e != hipSuccess) { normalize_free(h); return sfail(h, DRIL_ERR_HIP, std::string("dril_sac_ext_normalize_enable: ") + hipGetErrorString(e)); }
    h->nz.cfg = c; h->nz.on = true; h->xw_begin = h->xw_live = false;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_normalize_set_training(dril_sac_handle* h, int32_t training) {
    SNEED(h); XN_ON(h, "dril_sac_ext_normalize_set_training");
    h->nz.cfg.training = training != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_normalize_get_config(dril_sac_handle* h, dril_sac_normalize_config* cfg) {
    SNEED(h); XN_ON(h, "dril_sac_ext_normalize_get_config");
    return nzv_get_config(h, "dril_sac_ext_normalize_get_config", cfg);
}
DRIL_EXPORT int32_t dril_sac_ext_normalize_get_stats(dril_sac_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    SNEED(h); XN_ON(h, "dril_sac_ext_normalize_get_stats");
    return nzv_get_stats(h, "dril_sac_ext_normalize_get_stats", obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_sac_ext_normalize_set_stats(dril_sac_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    SNEED(h); XN_ON(h, "dril_sac_ext_normalize_set_stats");
    XW_NO_PENDING_ACT(h, "dril_sac_ext_normalize_set_stats");                          // (the pending observation was normalised under the statistics in force)
    return nzv_set_stats(h, "dril_sac_ext_normalize_set_stats", obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_sac_ext_normalize_get_original(dril_sac_handle* h, float* obs, float* rewards) {
    SNEED(h); XN_ON(h, "dril_sac_ext_normalize_get_original");
    if (!obs && !rewards) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_normalize_get_original: both out pointers are null");
    SDO(ssync(h));
    if (obs) SHIP(h, hipMemcpy(obs, h->nz_old_obs, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost));
    if (rewards) SHIP(h, hipMemcpy(rewards, h->nz_old_rew, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_normalize_get_returns(dril_sac_handle* h, float* returns) {
    SNEED(h); XN_ON(h, "dril_sac_ext_normalize_get_returns");
    return nzv_get_returns(h, "dril_sac_ext_normalize_get_returns", returns);
}
DRIL_EXPORT int32_t dril_sac_ext_normalize_reset(dril_sac_handle* h, void* caller_stream) {
    SNEED(h); XN_ON(h, "dril_sac_ext_normalize_reset");
    XW_NO_PENDING_ACT(h, "dril_sac_ext_normalize_reset");
    DeviceVerbScope scope(h);
    SHIP(h, ext_stream_take(h->stream, h->ext_ev_in, caller_stream));
    StreamHandOver back(h, caller_stream);
    SHIP(h, hipMemsetAsync(h->nz_returns, 0, (size_t)h->cfg.n_envs * 4, h->stream));   // reset! :110-121: returns <- 0; the env's own reset gives the next observation
    SHIP(h, back.give());
    h->xw_begin = h->xw_live = false;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_collection_begin(dril_sac_handle* h) {
    SNEED(h); XW_KIND(h, "dril_sac_ext_collection_begin", "driven by dril_sac_collect_rollout");
    if (h->nz.on) h->xw_begin = true;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_ext_monitor_enable(dril_sac_handle* h, int32_t window) {
    SNEED(h); XW_KIND(h, "dril_sac_ext_monitor_enable", "dril_sac_monitor_enable");
    if (window < 0) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_ext_monitor_enable: window must be >= 1 (MonitorWrapperEnv's stats_window), or 0 to switch the monitor off");
    XW_NO_PENDING_ACT(h, "dril_sac_ext_monitor_enable");
    if (window == h->mon_window) return DRIL_OK;                                      // the same wrapper again: its window and running sums stay
    SDO(ssync(h));
    monitor_free(h);
    if (window == 0) return DRIL_OK;
    // the block of buffered steps: a row per push until dril_sac_flush / dril_sac_ext_monitor_get_stats (or a full block) collects it; about a million entries, 4 .. 256 rows
    const size_t E = (size_t)h->cfg.n_envs, rows = std::max<size_t>(4, std::min<size_t>(256, ((size_t)1 << 20) / E));
    const hipError_t e = monitor_alloc(h, window, rows);
    if (e != hipSuccess) { monitor_free(h); return sfail(h, DRIL_ERR_HIP, std::string("dril_sac_ext_monitor_enable: ") + hipGetErrorString(e)); }
    h->mon_window = window; h->mon_rows_cap = (int)rows;
    return DRIL_OK;
}
