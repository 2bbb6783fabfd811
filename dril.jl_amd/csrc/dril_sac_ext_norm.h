// dril_sac_ext_norm.h — what is the DRIL_ENV_EXTERNAL SAC handle's own of NormalizeWrapperEnv / MonitorWrapperEnv around the caller's device-resident envs
// (dril_sac_ext_normalize_enable / dril_sac_ext_monitor_enable, include/dril_sac.h; honoured by dril_sac_ext_act_device / _push_device and
// dril_sac_predict_actions_device).  Scalars, the moments kernel, the head of an apply kernel and the host state are dril_norm_wrap.h; the table shape (at most
// kNzMaxRows rows, column tiles of kNzTile) and the LDS layout are dril_sac_norm.h's; the per-env rules of a recorded step are dril_ext_record.h's.  The launches are
// dril_sac_ext.hip's, the one unit that includes this header.
//
// One verb has one grid-wide dependency (all envs' sums -> the merged statistics -> every env's normalised row), so a verb is
//   moments   norm_moments_kernel<kNzTile> over the CALLER's arrays (act: d_obs, opening act only; push: d_next_obs and `returns` advanced by d_rewards, ONE launch)
//   apply     sac_ext_norm_act_kernel / sac_ext_norm_push_kernel below
// The apply kernels are this handle's because of their data flow: their inputs are the caller's const arrays; the act kernel writes old_obs and the pending
// observation from one read and stands where the unwrapped verb has its device-to-device copy; the push kernel is sac_norm_apply_kernel's twin and stands where
// the unwrapped verb has sac_ext_push_kernel — a NULL terminal_obs is legal, and the next observation is not kept (the next act normalises the caller's array again
// under the same statistics, which gives the same bits).
// No atomics: the launch shape fixes the order of every sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dril_norm_wrap.h"     // NormWrapArgs, nz_fold, nz_statistics, nz_obs, nz_reward
#include "dril_sac_device.h"    // PushArgs
#include "dril_sac_norm.h"      // nz_apply_lds: the LDS layout this one extends
#include "dril_ext_record.h"    // xr_*: the per-env scalar rules of the push

namespace dril::sac {
namespace {

// the dynamic LDS of both kernels: sac_norm_apply_kernel's layout, then (push) the observation statistics as they were before the launch
static_assert(sizeof(double) * (256 + 2 * (size_t)kNzMaxD + 2) + sizeof(float) * (4 * (size_t)kNzMaxD + 2) <= 48 * 1024, "sac_ext_norm_push_kernel's dynamic LDS at the widest observation");
inline size_t xs_push_lds(int D) { return nz_apply_lds(D) + sizeof(float) * 2 * (size_t)D; }

// the observation half of the head both kernels share: the 2 D observation columns of the table (and, with_ret, the two of `returns`) folded 256 at a time
__device__ __forceinline__ void xs_fold(const NormWrapArgs& a, bool obs, bool ret, double* s_part, double* s_col) {
    const int D = a.D, C = 2 * D + 2;
    if (obs) for (int c0 = 0; c0 < 2 * D; c0 += 256) nz_fold(a.partials, a.rows, C, min(256, 2 * D - c0), [=](int j) { return c0 + j; }, s_part, s_col + c0);
    if (ret) nz_fold(a.partials, a.rows, C, 2, [=](int j) { return 2 * D + j; }, s_part, s_col + 2 * D);
}

// ---- observe (normalizeWrapperEnv.jl:123-137) of dril_sac_ext_act_device / dril_sac_predict_actions_device -----------------------------------------------------
// Block b owns the rows [b epb, b epb + epb).  Head: the observation columns of the table, the merge, the new statistics in LDS; block 0 stores them (and carries
// the return pair).  Body: ONE flat (row, column) pass — a wave's loads and stores are contiguous runs for any D.
// w.partials == null: nothing is updated (a later act of the collection, frozen statistics, predict); old_obs == null: the wrapper's cache stays (predict)
struct XsActArgs { NormWrapArgs w; float* old_obs; };
__global__ __launch_bounds__(256) void sac_ext_norm_act_kernel(XsActArgs p) {
    extern __shared__ double nz_sh[];
    const NormWrapArgs& a = p.w;
    const int t = threadIdx.x, D = a.D, C = 2 * D + 2;
    double* s_part = nz_sh; double* s_col = nz_sh + 256;
    float* s_mean = reinterpret_cast<float*>(s_col + C); float* s_var = s_mean + D; float* s_rvar = s_var + D;
    const bool upd_obs = a.partials && a.upd_obs;
    xs_fold(a, upd_obs, false, s_part, s_col);
    nz_statistics(a, upd_obs, false, 0, D, true, 0, blockIdx.x == 0, s_col, s_mean, s_var, s_rvar);
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    for (int i = t; i < n * D; i += 256) {
        const int d = i % D; const size_t j = (size_t)(e0 + i / D) * D + d;
        float v = a.raw[j];
        if (p.old_obs) p.old_obs[j] = v;                                                 // old_obs, :127
        if (a.norm_obs) v = nz_obs(v, s_mean[d], s_var[d], a.eps, a.clip_obs);           // the NEW statistics
        a.obs_out[j] = v;                                                                // norm_obs == 0: the raw bits
    }
}

// ---- act! (:139-165) + observe (:123-137) + push! (replay_buffer.jl:98-114) of dril_sac_ext_push_device, MonitorWrapperEnv inside -----------------------------
// The same grid.  Head (has_norm): the observation statistics in force into LDS (the terminal observations' — :157-163 runs before this push's observe), then the
// fold, the merge of both statistics and the new ones in LDS.  Flat (env, column) pass: the ring's observation row from the pending observation, its next-observation
// row from d_terminal_obs under the OLD statistics where the env was truncated (only those rows of it are read) and from d_next_obs under the NEW ones elsewhere,
// old_obs.  Per env (dril_ext_record.h): sticky error, old_rewards, normalised reward, flags, the `returns` reset, the monitor's sums and its row of the block.
// Flat (env, action) pass: the stored action.  has_norm == 0: MonitorWrapperEnv alone — sac_ext_push_kernel's rows, plus the sums.
struct XsPushArgs {
    NormWrapArgs w;                                                                      // w.raw: d_next_obs; w.rew / w.term / w.trunc: the caller's; w.returns
    int has_norm; const float* tobs;                                                     // tobs null: the caller states that no env was truncated
    float* old_obs; float* old_rew; PushArgs push; int* err;                             // push.obs: the normalised pending observation, push.raw: the stored action
    float* mon_cur_ret; int32_t* mon_cur_len; float* ep_ret; int32_t* ep_len; uint8_t* ep_flags;   // null: monitor off; ep_*: this step's row of the block
};
__global__ __launch_bounds__(256) void sac_ext_norm_push_kernel(XsPushArgs p) {
    extern __shared__ double nz_sh[];
    const NormWrapArgs& a = p.w;
    const int t = threadIdx.x, D = a.D, C = 2 * D + 2;
    double* s_part = nz_sh; double* s_col = nz_sh + 256;
    float* s_mean = reinterpret_cast<float*>(s_col + C); float* s_var = s_mean + D; float* s_rvar = s_var + D;
    float* s_omean = s_rvar + 2; float* s_ovar = s_omean + D;
    const bool norm_obs = p.has_norm && a.norm_obs;
    if (p.has_norm) {
        const bool upd_obs = a.partials && a.upd_obs, upd_ret = a.partials && a.upd_ret;
        for (int d = t; d < D; d += 256) { s_omean[d] = a.st_in[d]; s_ovar[d] = a.st_in[D + d]; }
        xs_fold(a, upd_obs, upd_ret, s_part, s_col);
        nz_statistics(a, upd_obs, upd_ret, 0, D, true, 0, blockIdx.x == 0, s_col, s_mean, s_var, s_rvar);   // (ends on a barrier: s_omean / s_ovar are visible too)
    }
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    const PushArgs& g = p.push;
    for (int i = t; i < n * D; i += 256) {
        const int e = e0 + i / D, d = i % D; const size_t j = (size_t)e * D + d;
        const long long slot = (g.tail + e) % g.cap;
        g.rb_obs[slot * D + d] = g.obs[j];
        float v = a.raw[j];
        if (p.old_obs) p.old_obs[j] = v;                                                 // old_obs of the observe that follows act!
        if (a.trunc[e] && p.tobs) {                                                      // terminal_observation, :157-163: the statistics as they are before this observe
            v = p.tobs[j];
            if (norm_obs) v = nz_obs(v, s_omean[d], s_ovar[d], a.eps, a.clip_obs);
        } else if (norm_obs) v = nz_obs(v, s_mean[d], s_var[d], a.eps, a.clip_obs);      // the NEW statistics
        g.rb_next[slot * D + d] = v;                                                     // truncated_observation | next observation
    }
    const float rvar = p.has_norm ? *s_rvar : 1.f;
    for (int i = t; i < n; i += 256) {
        const int e = e0 + i;
        const float r = a.rew[e];
        const bool te = a.term[e] != 0, tr = a.trunc[e] != 0, done = te || tr;
        if (dril::xr_sticky(tr, p.tobs != nullptr)) *p.err = 1;
        float rn = r;
        if (p.has_norm) {
            p.old_rew[e] = r;                                                            // old_rewards, :141
            if (a.norm_reward) rn = nz_reward(r, rvar, a.eps, a.clip_reward);
            a.returns[e] = dril::xr_returns_reset(a.returns[e], done);                   // :149-153
        }
        const long long slot = (g.tail + e) % g.cap;
        g.rb_rew[slot] = rn; g.rb_term[slot] = te; g.rb_trunc[slot] = tr;
        if (p.mon_cur_ret) {                                                             // the monitor sits inside: the raw reward
            float cr = p.mon_cur_ret[e]; int32_t cl = p.mon_cur_len[e];
            dril::xr_monitor(r, done, cr, cl, p.ep_ret + e, p.ep_len + e);
            p.mon_cur_ret[e] = cr; p.mon_cur_len[e] = cl; p.ep_flags[e] = done;
        }
    }
    const int A = g.A;
    for (int i = t; i < n * A; i += 256) {
        const int e = e0 + i / A, k = i % A;
        g.rb_act[((g.tail + e) % g.cap) * A + k] = g.raw[(size_t)e * A + k];             // unprocessed action, off_policy_collection.jl:72
    }
}

}  // namespace
}  // namespace dril::sac
