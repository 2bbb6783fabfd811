// dril_ext_norm.h — what is the DRIL_ENV_EXTERNAL handle's own of NormalizeWrapperEnv / MonitorWrapperEnv around the caller's device-resident envs
// (dril_ext_normalize_enable / dril_ext_monitor_enable, include/dril_hip.h; honoured by dril_ext_act_device / _record_device / _finish_device and
// dril_predict_actions_device).  Scalars, the moments kernel, the head of an apply kernel and the host state are dril_norm_wrap.h; the table shape (pn_rows, pn_tiles,
// column tiles of 64) is dril_ppo_norm.h's: like a plug-in rollout, an external one has many envs per step.  The launches are dril_wrap.hip's.
//
// One env step has one grid-wide dependency per half (all envs' sums -> the merged statistics -> every env's normalised value), so each half is
//   moments   norm_moments_kernel<kPnTile> over the CALLER's array (d_obs, or `returns` advanced by d_rewards)
//   apply     ext_norm_observe_kernel / ext_norm_record_kernel below
// The apply kernels are this handle's because their data flow is: the observation is read once from the caller's array and written to the rollout row AND to
// old_obs (the unwrapped verb's device-to-device copy is gone); the record kernel is ext_record_kernel (dril_ext_device.hip) with the wrapper's act! and the
// monitor's sums fused in, and the caller's terminal observations — a const array — normalised into a scratch array of the handle.
// No atomics: the launch shape fixes the order of every sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dril_norm_wrap.h"    // NormWrapArgs, nz_fold, nz_statistics, nz_obs, nz_reward
#include "dril_ppo_norm.h"     // kPnTile
#include "dril_ext_record.h"   // xr_*: the per-env scalar rules of the record

namespace {

// ---- observe (normalizeWrapperEnv.jl:123-137) -------------------------------------------------------------------------------------------------------------------------
// grid (env ranges, tiles): block (b, y) owns the envs [b epb, b epb + epb) and the columns [c0, c0 + W) of tile y (D <= 64: all of them).
// Head: the column sums of its tile, the merge, the new statistics of its columns in LDS; the blocks b == 0 store theirs (tile 0: and the untouched return pair).
// Body: ONE flat (env, column) pass — a wave's loads and stores are contiguous runs of the arrays for any D.
// w.partials == null: nothing is updated (training == 0, norm_obs == 0, or dril_predict_actions_device); old_obs == null: the wrapper's cache stays (evaluation)
struct XnObserveArgs { NormWrapArgs w; float* old_obs; };
__global__ __launch_bounds__(256) void ext_norm_observe_kernel(XnObserveArgs p) {
    __shared__ double s_part[256], s_col[2 * kPnTile + 2];
    __shared__ float s_mean[kPnTile], s_var[kPnTile], s_rvar;
    const NormWrapArgs& a = p.w;
    const int t = threadIdx.x, D = a.D;
    const int c0 = D > kPnTile ? blockIdx.y * kPnTile : 0, W = D > kPnTile ? min(kPnTile, D - c0) : D;
    __builtin_assume(W <= kPnTile);                                                      // (nz_statistics: one pass over the columns)
    const bool upd_obs = a.partials && a.upd_obs;
    if (upd_obs)                                                                         // local column j: sum x of c0 + j | sum x^2 of c0 + j - W
        nz_fold(a.partials, a.rows, 2 * D + 2, 2 * W, [=](int j) { return j < W ? c0 + j : D + c0 + (j - W); }, s_part, s_col);
    nz_statistics(a, upd_obs, false, c0, W, blockIdx.y == 0, 64, blockIdx.x == 0, s_col, s_mean, s_var, &s_rvar);
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    for (int i = t; i < n * W; i += 256) {
        const int e = e0 + i / W, d = i % W; const size_t j = (size_t)e * D + c0 + d;
        float v = a.raw[j];
        if (p.old_obs) p.old_obs[j] = v;                                                 // old_obs, :127
        if (a.norm_obs) v = nz_obs(v, s_mean[d], s_var[d], a.eps, a.clip_obs);           // the NEW statistics
        a.obs_out[j] = v;                                                                // norm_obs == 0: the raw bits
    }
}

// ---- act! (:139-165) with dril_ext_record_device's own work and MonitorWrapperEnv inside ---------------------------------------------------------------------------
// The same grid.  Head: tile 0 folds the two `returns` columns and merges them; every tile reads the observation statistics IN FORCE (this launch does not update
// them: they are the ones before the following observe) and, where the launch updates, carries them to the other half.
// Per env (tile 0; the scalar rules are dril_ext_record.h): flags byte, sticky error, boot[t] = 0 (the selection behind the critic forward fills the truncated
// envs), old_rewards, the normalised reward into row t, the `returns` reset, the monitor's sums and ep rows.
// Flat (env, column) pass (every tile): terminal observation -> normalised scratch where truncated, 0 elsewhere (a NaN of a row that is not the env's to give
// never reaches the critic).
struct XnRecordArgs {
    NormWrapArgs w;                                                                      // w.rew: the caller's rewards; w.term / w.trunc: its flags; w.returns
    int has_norm;                                                                        // 0: MonitorWrapperEnv alone — the reward passes, nothing of the normaliser is read
    const float* tobs; float* tobs_out;                                                  // the caller's terminal_obs (null: none) -> the scratch (null: norm_obs == 0, the critic reads the caller's array)
    float* old_rew; float* rew_out; uint8_t* flags; float* boot; int* err;               // rew_out / flags / boot: row t of the buffer
    float* mon_cur_ret; int32_t* mon_cur_len; float* ep_ret; int32_t* ep_len;            // null: monitor off; ep_*: row t
};
__global__ __launch_bounds__(256) void ext_norm_record_kernel(XnRecordArgs p) {
    __shared__ double s_part[256], s_col[2 * kPnTile + 2];
    __shared__ float s_mean[kPnTile], s_var[kPnTile], s_rvar;
    const NormWrapArgs& a = p.w;
    const int t = threadIdx.x, D = a.D;
    const int c0 = D > kPnTile ? blockIdx.y * kPnTile : 0, W = D > kPnTile ? min(kPnTile, D - c0) : D;
    __builtin_assume(W <= kPnTile);
    const bool tile0 = blockIdx.y == 0, do_tobs = p.tobs_out != nullptr;
    if (!tile0 && !do_tobs && !(a.st_out && blockIdx.x == 0)) return;                    // (uniform per block) a further tile with no column work and no statistics to carry
    const bool upd_ret = p.has_norm && a.partials && a.upd_ret && tile0;
    if (upd_ret) nz_fold(a.partials, a.rows, 2 * D + 2, 2, [=](int j) { return 2 * D + j; }, s_part, s_col + 2 * W);
    if (p.has_norm) nz_statistics(a, false, upd_ret, c0, W, tile0, 64, blockIdx.x == 0, s_col, s_mean, s_var, &s_rvar);
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    if (do_tobs) {
        for (int i = t; i < n * W; i += 256) {
            const int e = e0 + i / W, d = i % W; const size_t j = (size_t)e * D + c0 + d;
            p.tobs_out[j] = a.trunc[e] ? nz_obs(p.tobs[j], s_mean[d], s_var[d], a.eps, a.clip_obs) : 0.f;   // terminal_observation, :157-163
        }
    }
    if (!tile0) return;
    const float rvar = p.has_norm ? s_rvar : 1.f;
    for (int i = t; i < n; i += 256) {
        const int e = e0 + i;
        const float r = a.rew[e];
        const bool te = a.term[e] != 0, tr = a.trunc[e] != 0, done = te || tr;
        p.flags[e] = dril::xr_flags(te, tr);
        p.boot[e] = 0.f;
        if (dril::xr_sticky(tr, p.tobs != nullptr)) *p.err = 1;
        float rn = r;
        if (p.has_norm) {
            p.old_rew[e] = r;                                                            // old_rewards, :141
            if (a.norm_reward) rn = nz_reward(r, rvar, a.eps, a.clip_reward);
            a.returns[e] = dril::xr_returns_reset(a.returns[e], done);                   // :149-153
        }
        p.rew_out[e] = rn;
        if (p.mon_cur_ret) {                                                             // the monitor sits inside: the raw reward
            float cr = p.mon_cur_ret[e]; int32_t cl = p.mon_cur_len[e];
            dril::xr_monitor(r, done, cr, cl, p.ep_ret + e, p.ep_len + e);
            p.mon_cur_ret[e] = cr; p.mon_cur_len[e] = cl;
        }
    }
}

}  // namespace
