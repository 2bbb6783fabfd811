// dril_sac_wrap.hip — MonitorWrapperEnv (monitorWrapperEnv.jl) and NormalizeWrapperEnv (normalizeWrapperEnv.jl; rules and state: dril_norm_wrap.h) around the SAC
// handle's device envs, the counterpart of dril_wrap.hip: their arrays, the window launch after a collection, the moments and apply launches of a collected step,
// and the verbs dril_sac_monitor_* and dril_sac_normalize_*.  The steps that go through the wrappers are dril_sac_collect.hip; the wrappers of an external handle
// (dril_sac_ext.hip) use the same arrays and the nzv_* bodies.  The units: dril_sac_handle.h.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "dril_sac_handle.h"

using namespace dril;
using namespace dril::sac;

namespace {

// ---- NormalizeWrapperEnv in a collection: apply + push (argument blocks and the table shape: dril_sac_norm.h) -------------------------------------------------
// Block b owns the envs [b epb, b epb + epb) and keeps the statistics of all D columns in (dynamic) LDS.  Head (dril_norm_wrap.h): the column sums of the table, 256
// columns at a time, the merge, the new statistics in LDS; block 0 stores them to st_out.  Body: flat (env, dim) loops, so a wave's loads and its stores into obs_out
// and the ring are contiguous runs for any D.
__global__ __launch_bounds__(256) void sac_norm_apply_kernel(NzApplyArgs p) {
    extern __shared__ double nz_sh[];
    const NormWrapArgs& a = p.w;
    const int t = threadIdx.x, D = a.D, C = 2 * D + 2;
    double* s_part = nz_sh; double* s_col = nz_sh + 256;
    float* s_mean = reinterpret_cast<float*>(s_col + C); float* s_var = s_mean + D; float* s_rvar = s_var + D;
    const bool upd_obs = a.partials && a.upd_obs, upd_ret = a.partials && a.upd_ret && a.rew;
    if (upd_obs || upd_ret)
        for (int c0 = 0; c0 < C; c0 += 256) nz_fold(a.partials, a.rows, C, min(256, C - c0), [=](int j) { return c0 + j; }, s_part, s_col + c0);
    nz_statistics(a, upd_obs, upd_ret, 0, D, true, 0, blockIdx.x == 0, s_col, s_mean, s_var, s_rvar);
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    const bool push = p.push.E > 0;
    for (int i = t; i < n * D; i += 256) {
        const int e = e0 + i / D, d = i % D; const size_t j = (size_t)e * D + d;
        float v = a.raw[j];
        if (a.norm_obs) v = nz_obs(v, s_mean[d], s_var[d], a.eps, a.clip_obs);           // observe :123-137: the NEW statistics
        a.obs_out[j] = v;
        if (push) {
            const long long slot = (p.push.tail + e) % p.push.cap;
            p.push.rb_obs[slot * D + d] = p.push.obs[j];
            if (a.trunc[e]) {                                                            // terminal_observation, :157-163: the statistics as they are before this observe
                v = p.tobs[j];
                if (a.norm_obs) v = nz_obs(v, a.st_in[d], a.st_in[D + d], a.eps, a.clip_obs);
            }
            p.push.rb_next[slot * D + d] = v;                                            // truncated_observation | next observation
        }
    }
    if (a.rew) {
        const float rvar = *s_rvar;
        for (int i = t; i < n; i += 256) {
            const int e = e0 + i;
            const float r = a.rew[e];
            p.old_rew[e] = r;
            float rn = r;
            if (a.norm_reward) rn = nz_reward(r, rvar, a.eps, a.clip_reward);
            const bool term = a.term[e] != 0, trunc = a.trunc[e] != 0;
            if (term || trunc) a.returns[e] = 0.f;                                       // :152-155
            if (push) { const long long slot = (p.push.tail + e) % p.push.cap; p.push.rb_rew[slot] = rn; p.push.rb_term[slot] = term; p.push.rb_trunc[slot] = trunc; }
        }
    }
    if (push) {
        const int A = p.push.A;
        for (int i = t; i < n * A; i += 256) {
            const int e = e0 + i / A, k = i % A;
            p.push.rb_act[((p.push.tail + e) % p.push.cap) * A + k] = p.push.raw[(size_t)e * A + k];   // unprocessed action, off_policy_collection.jl:72
        }
    }
    phase_stamp(p.push.stamp);
}

// ---- MonitorWrapperEnv's window (monitorWrapperEnv.jl:1-7,53-58) after a collection, in ONE launch ---------------------------------------------------
// flags / ep_ret / ep_len: the collection's [T][E] block (a row per env step; ep_* valid where the flag is set), whose flat order IS the (step, env) order in which
// the reference pushes finished episodes.  One workgroup: count the events, then an ordered scan that writes the last min(total, W) of them behind the ring's head.
// The two-kernel form of dril_kernels.hip (monitor_count_kernel + monitor_collect_kernel) spreads the count over T workgroups, which pays for a PPO rollout of
// hundreds of steps; a SAC collection is train_freq steps, usually ONE, and a second dependent launch would add a launch gap to every env step — so the count is
// the first pass of the same workgroup here, and a collection in which no episode ended (nearly all of them) leaves after it.
constexpr int kMonBlock = 1024;
__global__ __launch_bounds__(kMonBlock) void sac_monitor_window_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ ep_ret, const int32_t* __restrict__ ep_len,
                                                                       int n, int W, float* ring_ret, int32_t* ring_len, int* meta) {
    __shared__ int wsum[kMonBlock / 64], s_total, s_base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += kMonBlock) c += flags[i] != 0;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) wsum[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < kMonBlock / 64; ++w) t += wsum[w]; s_total = t; s_base = 0; }
    __syncthreads();
    const int total = s_total;
    if (total == 0) return;
    const int skip = total > W ? total - W : 0, head0 = meta[1];
    for (int i0 = 0; i0 < n; i0 += kMonBlock) {
        const int i = i0 + threadIdx.x;
        const int f = (i < n && flags[i] != 0) ? 1 : 0;
        int incl = f;                                                                // inclusive scan within the wave, then across the waves
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d); if (lane >= d) incl += v; }
        __syncthreads();                                                             // (wsum of the previous pass has been read by everyone)
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int off = 0, chunk = 0;
        for (int w = 0; w < kMonBlock / 64; ++w) { if (w < wv) off += wsum[w]; chunk += wsum[w]; }
        const int gi = s_base + off + incl - f;                                      // this event's index among the collection's events
        if (f && gi >= skip) { const int pos = (head0 + gi - skip) % W; ring_ret[pos] = ep_ret[i]; ring_len[pos] = ep_len[i]; }
        __syncthreads();
        if (threadIdx.x == 0) s_base += chunk;
    }
    if (threadIdx.x == 0) {
        const int pushed = total - skip;
        meta[1] = (head0 + pushed) % W;
        const int cnt = meta[0] + pushed; meta[0] = cnt > W ? W : cnt;
    }
}

}  // namespace

namespace dril::sac {
// ---- MonitorWrapperEnv around the handle's device envs (monitorWrapperEnv.jl) ----------------------------------------------------------------------------
void monitor_free(dril_sac_handle* h) {
    h->mon_cur_ret.release(); h->mon_cur_len.release(); h->mon_ring_ret.release(); h->mon_ring_len.release();
    h->mon_meta.release(); h->mon_ep_ret.release(); h->mon_ep_len.release(); h->mon_flags.release();
    h->mon_window = 0; h->mon_rows_cap = 0; h->mon_row = 0;
}
// the arrays of a monitor with this window and a block of `rows` buffered steps, zeroed: fresh sums, an empty window
hipError_t monitor_alloc(dril_sac_handle* h, int32_t window, size_t rows) {
    const size_t E = (size_t)h->cfg.n_envs;
    hipError_t e = h->mon_cur_ret.alloc_zero(E);
    if (e == hipSuccess) e = h->mon_cur_len.alloc_zero(E);
    if (e == hipSuccess) e = h->mon_ring_ret.alloc_zero((size_t)window);
    if (e == hipSuccess) e = h->mon_ring_len.alloc_zero((size_t)window);
    if (e == hipSuccess) e = h->mon_meta.alloc_zero(2);
    if (e == hipSuccess) e = h->mon_ep_ret.alloc_zero(rows * E);
    if (e == hipSuccess) e = h->mon_ep_len.alloc_zero(rows * E);
    if (e == hipSuccess) e = h->mon_flags.alloc_zero(rows * E);
    return e;
}
// MonitorWrapperEnv in a collection: the running sums and row h->mon_row of the collection's finished-episode block for the step being enqueued (all null: off)
MonitorArgs monitor_row(dril_sac_handle* h) {
    MonitorArgs m{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!h->mon_window) return m;
    const size_t o = (size_t)h->mon_row * h->cfg.n_envs;
    m.cur_ret = h->mon_cur_ret; m.cur_len = h->mon_cur_len; m.ep_ret = h->mon_ep_ret + o; m.ep_len = h->mon_ep_len + o; m.flags_out = h->mon_flags + o;
    return m;
}
// before a collection of n_steps: its block has n_steps rows (grown on demand: the start phase is the one long collection of a run)
int monitor_begin(dril_sac_handle* h, int n_steps) {
    if (!h->mon_window) return DRIL_OK;
    h->mon_row = 0;
    if (n_steps <= h->mon_rows_cap) return DRIL_OK;
    SDO(ssync(h));                                                                                 // (the previous collection's window launch reads the old rows)
    h->mon_rows_cap = 0;
    const size_t n = (size_t)n_steps * h->cfg.n_envs;
    SHIP(h, h->mon_ep_ret.alloc_zero(n)); SHIP(h, h->mon_ep_len.alloc_zero(n)); SHIP(h, h->mon_flags.alloc_zero(n)); h->mon_rows_cap = n_steps;
    return DRIL_OK;
}
// after its last step: the finished episodes of the whole collection into the window, one launch (sac_monitor_window_kernel)
int monitor_end(dril_sac_handle* h) {
    if (!h->mon_window || h->mon_row == 0) return DRIL_OK;
    hipLaunchKernelGGL(sac_monitor_window_kernel, dim3(1), dim3(kMonBlock), 0, h->stream, h->mon_flags, h->mon_ep_ret, h->mon_ep_len, h->mon_row * h->cfg.n_envs, h->mon_window,
                       h->mon_ring_ret, h->mon_ring_len, h->mon_meta);
    SHIP(h, hipGetLastError());
    h->mon_row = 0;
    return DRIL_OK;
}
// log_stats over the window as it stands on the device, after a drain: one body for dril_sac_monitor_get_stats and dril_sac_ext_monitor_get_stats
int monitor_read(dril_sac_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes) {
    const int W = h->mon_window;
    std::vector<float> r(W); std::vector<int32_t> l(W); int meta[2] = {0, 0};
    SHIP(h, hipMemcpyAsync(r.data(), h->mon_ring_ret, (size_t)W * 4, hipMemcpyDeviceToHost, h->stream));
    SHIP(h, hipMemcpyAsync(l.data(), h->mon_ring_len, (size_t)W * 4, hipMemcpyDeviceToHost, h->stream));
    SHIP(h, hipMemcpyAsync(meta, h->mon_meta, 8, hipMemcpyDeviceToHost, h->stream));
    SDO(ssync(h));
    double sr = 0, sl = 0;
    for (int i = 0; i < meta[0]; ++i) { sr += r[i]; sl += l[i]; }
    if (n_episodes) *n_episodes = meta[0];
    if (meta[0] > 0) {                                                                // log_stats: mean over the CircularBuffer, monitorWrapperEnv.jl:64-70; nothing to log for an empty one
        if (ep_rew_mean) *ep_rew_mean = (float)(sr / meta[0]);
        if (ep_len_mean) *ep_len_mean = (float)(sl / meta[0]);
    }
    return DRIL_OK;
}

// ---- NormalizeWrapperEnv in a collection (kernels: dril_sac_norm.h) -----------------------------------------------------------------------------------------
void normalize_free(dril_sac_handle* h) {
    h->nz.release();
    h->nz_returns.release(); h->nz_old_obs.release(); h->nz_old_rew.release(); h->nz_raw_valid = false;
}
// a fresh wrapper with a table of `rows` rows, and the handle's arrays next to it, zeroed: returns and the cached originals start at 0
hipError_t normalize_alloc(dril_sac_handle* h, size_t rows) {
    const size_t E = (size_t)h->cfg.n_envs, D = (size_t)h->D;
    hipError_t e = h->nz.alloc((int)D, rows);
    if (e == hipSuccess) e = h->nz_returns.alloc_zero(E);
    if (e == hipSuccess) e = h->nz_old_obs.alloc_zero(E * D);
    if (e == hipSuccess) e = h->nz_old_rew.alloc_zero(E);
    return e;
}
// the raw observation of the envs' present state in nz_old_obs (reset! :110-121 stores it; so does every observe)
int nz_ensure_raw(dril_sac_handle* h) {
    if (!h->env.ready) return sfail(h, DRIL_ERR_NOT_INITIALISED, "dril_sac_env_reset has not been called");
    if (h->nz_raw_valid) return DRIL_OK;
    SHIP(h, h->env.observe(h->nz_old_obs, h->stream));
    h->nz_raw_valid = true;
    return DRIL_OK;
}
// norm_moments_kernel over nz_old_obs (obs) and / or the `returns` recursion over e_rew (ret); *rows: the rows of the table it writes
// (raw / rew: the arrays — the handle's own, or the caller's const ones on an external handle; null: that half is not summed)
int nz_moments_over(dril_sac_handle* h, const float* raw, const float* rew, int* rows) {
    const int E = h->cfg.n_envs, D = h->D, R = std::max(kEnvsPerBlock, (E + kNzMaxRows - 1) / kNzMaxRows);
    *rows = (E + R - 1) / R;
    const NormMomArgs m{E, D, R, raw, rew, h->nz_returns, h->nz.cfg.gamma, h->nz.partials};
    hipLaunchKernelGGL(norm_moments_kernel<kNzTile>, dim3(*rows, raw && D > 64 ? (D + kNzTile - 1) / kNzTile : 1), dim3(256), 0, h->stream, m);
    SHIP(h, hipGetLastError());
    return DRIL_OK;
}
int nz_moments(dril_sac_handle* h, bool obs, bool ret, int* rows) { return nz_moments_over(h, obs ? h->nz_old_obs : nullptr, ret ? h->e_rew : nullptr, rows); }
// sac_norm_apply_kernel over the table of `rows` rows the moments launch wrote
int nz_apply(dril_sac_handle* h, NzApplyArgs p, int rows, bool upd_obs, bool upd_ret) {
    NormWrapArgs& a = p.w;
    const int E = h->cfg.n_envs, D = h->D;
    h->nz.fill(a, upd_obs, upd_ret, E);
    a.E = E; a.rows = rows; a.epb = std::max(std::min(64, std::max(1, 2048 / D)), (E + 127) / 128);
    hipLaunchKernelGGL(sac_norm_apply_kernel, dim3((E + a.epb - 1) / a.epb), dim3(256), nz_apply_lds(D), h->stream, p);
    SHIP(h, hipGetLastError());
    h->nz.commit(a);
    return DRIL_OK;
}
// observe(env) of the wrapper (:123-137) over the envs' present state into `out`; update = false: a read-only peek
int nz_observe(dril_sac_handle* h, bool update, float* out) {
    SDO(nz_ensure_raw(h));
    const bool upd = update && h->nz.cfg.training && h->nz.cfg.norm_obs;
    int rows = 0;
    if (upd) SDO(nz_moments(h, true, false, &rows));
    NzApplyArgs a{}; a.w.raw = h->nz_old_obs; a.w.obs_out = out;
    return nz_apply(h, a, rows, upd, false);
}
// collect_trajectories begins with observe(env) (off_policy_collection.jl:42): one statistics update over the current raw observations, re-normalised
int nz_collect_begin(dril_sac_handle* h) { SDO(nz_observe(h, true, h->obs_cur)); h->obs_valid = true; return DRIL_OK; }

// the bodies of the verbs that read or write a wrapper that is on: one definition for dril_sac_normalize_* (device envs) and dril_sac_ext_normalize_* (external handles)
int nzv_get_config(dril_sac_handle* h, const std::string& verb, dril_sac_normalize_config* cfg) {
    if (!cfg) return sfail(h, DRIL_ERR_INVALID_ARG, verb + ": null out pointer");
    memcpy(cfg, &h->nz.cfg, sizeof(*cfg));
    return DRIL_OK;
}
int nzv_get_stats(dril_sac_handle* h, const std::string& verb, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    if (!obs_mean || !obs_var || !obs_count || !ret_mean || !ret_var || !ret_count) return sfail(h, DRIL_ERR_INVALID_ARG, verb + ": null out pointer");
    SDO(ssync(h));
    std::vector<float> st(h->nz.stats_floats());
    SHIP(h, hipMemcpy(st.data(), h->nz.half(h->nz.cur), st.size() * 4, hipMemcpyDeviceToHost));
    h->nz.unpack(st, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
    return DRIL_OK;
}
int nzv_set_stats(dril_sac_handle* h, const std::string& verb, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    if (const NormErr err = norm_set_stats_check(obs_mean, obs_var, obs_count, ret_count)) return sfail(h, err.code, verb + ": " + err.msg);
    SDO(ssync(h));
    const std::vector<float> st = h->nz.pack(obs_mean, obs_var, ret_mean, ret_var);
    SHIP(h, hipMemcpy(h->nz.half(h->nz.cur), st.data(), st.size() * 4, hipMemcpyHostToDevice));
    h->nz.obs_count = obs_count; h->nz.ret_count = ret_count;
    h->obs_valid = false; h->xw_begin = h->xw_live = false;                           // (the current normalised observation was made with other statistics)
    return DRIL_OK;
}
int nzv_get_returns(dril_sac_handle* h, const std::string& verb, float* returns) {
    if (!returns) return sfail(h, DRIL_ERR_INVALID_ARG, verb + ": null out pointer");
    SDO(ssync(h));
    SHIP(h, hipMemcpy(returns, h->nz_returns, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
}  // namespace dril::sac

DRIL_EXPORT int32_t dril_sac_monitor_enable(dril_sac_handle* h, int32_t window) {
    SNEED(h);
    if (h->external) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_monitor_enable: the envs of DRIL_ENV_EXTERNAL live on the host: MonitorWrapperEnv wraps them there");
    if (window < 0) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_monitor_enable: window must be >= 1 (MonitorWrapperEnv's stats_window), or 0 to switch the monitor off");
    if (window == h->mon_window) return DRIL_OK;                                      // the same wrapper again: its window and running sums stay
    SDO(ssync(h));
    monitor_free(h);
    if (window == 0) return DRIL_OK;
    const size_t E = (size_t)h->cfg.n_envs, rows = (size_t)std::max(1, h->cfg.train_freq);
    const hipError_t e = monitor_alloc(h, window, rows);
    if (e != hipSuccess) { monitor_free(h); return sfail(h, DRIL_ERR_HIP, std::string("dril_sac_monitor_enable: ") + hipGetErrorString(e)); }
    h->mon_window = window; h->mon_rows_cap = (int)rows;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_monitor_get_stats(dril_sac_handle* h, float* ep_rew_mean, float* ep_len_mean, int32_t* n_episodes) {
    SNEED(h);
    if (h->external) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_monitor_get_stats: the envs of DRIL_ENV_EXTERNAL live on the host: MonitorWrapperEnv wraps them there");
    if (!h->mon_window) return sfail(h, DRIL_ERR_NOT_INITIALISED, "MonitorWrapperEnv is off (dril_sac_monitor_enable has not been called with a window >= 1)");
    return monitor_read(h, ep_rew_mean, ep_len_mean, n_episodes);
}
// ---- NormalizeWrapperEnv around the handle's device envs (normalizeWrapperEnv.jl; rules and state: dril_norm_wrap.h) ------------------------------------------------------
#define S_NORMALIZE_ON(h, what) do { if ((h)->external) return sfail(h, DRIL_ERR_UNSUPPORTED, what ": the envs of DRIL_ENV_EXTERNAL live on the host: NormalizeWrapperEnv wraps them there"); \
    if (!(h)->nz.on) return sfail(h, DRIL_ERR_NOT_INITIALISED, what ": NormalizeWrapperEnv is off (dril_sac_normalize_enable has not been called with a configuration)"); } while (0)
// the two public configuration structs are one layout; inside the library it is dril_normalize_config
static_assert(sizeof(dril_sac_normalize_config) == sizeof(dril_normalize_config) && offsetof(dril_sac_normalize_config, training) == offsetof(dril_normalize_config, training) &&
              offsetof(dril_sac_normalize_config, norm_obs) == offsetof(dril_normalize_config, norm_obs) && offsetof(dril_sac_normalize_config, norm_reward) == offsetof(dril_normalize_config, norm_reward) &&
              offsetof(dril_sac_normalize_config, clip_obs) == offsetof(dril_normalize_config, clip_obs) && offsetof(dril_sac_normalize_config, clip_reward) == offsetof(dril_normalize_config, clip_reward) &&
              offsetof(dril_sac_normalize_config, gamma) == offsetof(dril_normalize_config, gamma) && offsetof(dril_sac_normalize_config, epsilon) == offsetof(dril_normalize_config, epsilon) &&
              offsetof(dril_sac_normalize_config, reserved) == offsetof(dril_normalize_config, reserved), "dril_sac_normalize_config and dril_normalize_config");
DRIL_EXPORT int32_t dril_sac_normalize_config_default(dril_sac_normalize_config* c) {
    if (!c) return sfail(nullptr, DRIL_ERR_INVALID_ARG, "dril_sac_normalize_config_default: null configuration");
    dril_normalize_config d; norm_config_default(&d); memcpy(c, &d, sizeof(d));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_normalize_enable(dril_sac_handle* h, const dril_sac_normalize_config* cfg) {
    SNEED(h);
    if (h->external) return sfail(h, DRIL_ERR_UNSUPPORTED, "dril_sac_normalize_enable: the envs of DRIL_ENV_EXTERNAL live on the host: NormalizeWrapperEnv wraps them there");
    if (!cfg) {                                                                        // the wrapper off: the next collection observes the env itself again
        if (!h->nz.on) return DRIL_OK;
        SDO(ssync(h)); normalize_free(h); h->obs_valid = false;
        return DRIL_OK;
    }
    dril_normalize_config c; memcpy(&c, cfg, sizeof(c));
    if (const NormErr err = norm_config_check(c, h->D)) return sfail(h, err.code, "dril_sac_normalize_enable: " + err.msg);
    c = norm_config_canonical(c);
    if (h->nz.keeps(c)) return DRIL_OK;                                                // the same wrapper again (training apart: that is set_training's to change): its statistics and returns stay
    SDO(ssync(h));
    normalize_free(h);
    const size_t E = (size_t)h->cfg.n_envs;
    const hipError_t e = normalize_alloc(h, std::max<size_t>(kNzMaxRows, h->env.module ? 0 : (E + kEnvsPerBlock - 1) / kEnvsPerBlock));
    if (e != hipSuccess) { normalize_free(h); return sfail(h, DRIL_ERR_HIP, std::string("dril_sac_normalize_enable: ") + hipGetErrorString(e)); }
    h->nz.cfg = c; h->nz.on = true; h->obs_valid = false;                              // the next collection observes through the wrapper
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_normalize_set_training(dril_sac_handle* h, int32_t training) {
    SNEED(h); S_NORMALIZE_ON(h, "dril_sac_normalize_set_training");
    h->nz.cfg.training = training != 0;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_normalize_get_config(dril_sac_handle* h, dril_sac_normalize_config* cfg) {
    SNEED(h); S_NORMALIZE_ON(h, "dril_sac_normalize_get_config");
    return nzv_get_config(h, "dril_sac_normalize_get_config", cfg);
}
DRIL_EXPORT int32_t dril_sac_normalize_get_stats(dril_sac_handle* h, float* obs_mean, float* obs_var, int64_t* obs_count, float* ret_mean, float* ret_var, int64_t* ret_count) {
    SNEED(h); S_NORMALIZE_ON(h, "dril_sac_normalize_get_stats");
    return nzv_get_stats(h, "dril_sac_normalize_get_stats", obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_sac_normalize_set_stats(dril_sac_handle* h, const float* obs_mean, const float* obs_var, int64_t obs_count, float ret_mean, float ret_var, int64_t ret_count) {
    SNEED(h); S_NORMALIZE_ON(h, "dril_sac_normalize_set_stats");
    return nzv_set_stats(h, "dril_sac_normalize_set_stats", obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count);
}
DRIL_EXPORT int32_t dril_sac_normalize_get_original(dril_sac_handle* h, float* obs, float* rewards) {
    SNEED(h); S_NORMALIZE_ON(h, "dril_sac_normalize_get_original");
    if (!obs && !rewards) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_normalize_get_original: both out pointers are null");
    SDO(nz_ensure_raw(h)); SDO(ssync(h));
    if (obs) SHIP(h, hipMemcpy(obs, h->nz_old_obs, (size_t)h->cfg.n_envs * h->D * 4, hipMemcpyDeviceToHost));
    if (rewards) SHIP(h, hipMemcpy(rewards, h->nz_old_rew, (size_t)h->cfg.n_envs * 4, hipMemcpyDeviceToHost));
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_normalize_get_returns(dril_sac_handle* h, float* returns) {
    SNEED(h); S_NORMALIZE_ON(h, "dril_sac_normalize_get_returns");
    return nzv_get_returns(h, "dril_sac_normalize_get_returns", returns);
}
