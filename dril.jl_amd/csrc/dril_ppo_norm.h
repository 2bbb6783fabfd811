// dril_ppo_norm.h — what is the PPO handle's own of NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) around its device env plug-in
// (dril_normalize_enable, include/dril_hip.h), for every observation width a plug-in may have (1 .. 1024).  Everything it shares with the SAC handle's wrapper —
// scalars, the moments kernel, the head of the apply kernel, the host state — is dril_norm_wrap.h; the launches are dril_wrap.hip's.  Built-in envs keep their own
// wrapper (cfg.norm_*: RmsState with 8 dims, the fused norm_step_kernel / norm_apply_kernel of dril_kernels.hip); this file is never launched for them.
//
// After the plug-in's own step kernel (raw reward, flags, terminal observation and next observation into the per-step arrays) two launches follow:
//   moments   norm_moments_kernel<kPnTile> over the E x D raw observations and the E rewards
//   apply     ppo_norm_apply_kernel: every block folds the columns it needs of the table (or reads the one all-reduced row of a data-parallel job), merges them into
//             the running statistics, writes the normalised reward into the rollout row, normalises the terminal observation of truncated envs with the OLD
//             observation statistics and the next observation with the NEW ones
// The opening observe of a rollout and dril_env_observe are the same two launches with the reward half off; dril_env_step is the pair with the observation half off.
//
// PPO collects with many envs per step (the rollout is E x T, T short), so both kernels are laid out for E up to 65 536:
//   * observations wider than 64 are cut into column tiles of 64 (one wave's width) in BOTH kernels: the moments kernel has rows x tiles workgroups, and an apply
//     block folds only its tile's 2 x 64 (+ 2) columns instead of all 2 D + 2;
//   * the table may have up to 256 rows for narrow observations: kPnFoldDoubles bounds what one apply block re-reads (rows x folded columns), not a fixed row count.
#pragma once
#include <hip/hip_runtime.h>

#include "dril_norm_wrap.h"   // NormWrapArgs, nz_fold, nz_statistics, nz_obs, nz_reward

namespace {

constexpr int kPnTile = 64;           // columns per tile when D > 64: a wave reads 64 consecutive floats of an env's row
constexpr int kPnMaxRows = 256;        // rows of the partial table (= workgroup rows of the moments kernel), and
constexpr int kPnFoldDoubles = 8192;   // rows x columns an apply block folds, at most: 64 KB from L2 per block, 32 loads per thread
constexpr int kPnMinEnvsPerRow = 16;

inline int pn_tiles(int D) { return D > kPnTile ? (D + kPnTile - 1) / kPnTile : 1; }
// rows of the table for E envs of width D: enough workgroups (rows x tiles >= 256 where E allows), bounded by the apply kernel's fold
inline int pn_rows(int E, int D, int cap) {
    const int tiles = pn_tiles(D), cols = D > kPnTile ? 2 * kPnTile + 2 : 2 * D + 2;
    int rows = D > kPnTile ? (kPnMaxRows + tiles - 1) / tiles : kPnMaxRows;
    if (rows > kPnFoldDoubles / cols) rows = kPnFoldDoubles / cols;
    if (rows < 16) rows = 16;
    if (cap > 0 && rows > cap) rows = cap;
    const int by_envs = (E + kPnMinEnvsPerRow - 1) / kPnMinEnvsPerRow;
    return rows < by_envs ? rows : by_envs;
}

// data-parallel jobs: this rank's table folded to ONE row of 2 D + 2 doubles (rows in index order), which the all-reduce then sums over the ranks
__global__ __launch_bounds__(256) void ppo_norm_fold_kernel(const double* __restrict__ partials, int rows, int C, double* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double u = 0;
    for (int b = 0; b < rows; ++b) u += partials[(size_t)b * C + c];
    out[c] = u;
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------------------------------------------
// grid (env ranges, tiles): block (b, y) owns the envs [b epb, b epb + epb) and the columns [c0, c0 + W) of tile y (D <= 64: all of them).
// Head (dril_norm_wrap.h): the column sums it needs — W of sum x, W of sum x^2 and, for tile 0, the two of `returns` — then the merge, the new statistics of its
// columns in LDS; the blocks b == 0 store theirs to st_out.
// Body: flat (env, column) loop, so a wave's loads and stores are contiguous runs of the arrays for any D.
// raw == null: act! alone (dril_env_step); rew == null: observe alone.
struct PnApplyArgs { NormWrapArgs w; float* rew_out; float* tobs; };                   // tobs (E x D): normalised in place where truncated
__global__ __launch_bounds__(256) void ppo_norm_apply_kernel(PnApplyArgs p) {
    __shared__ double s_part[256], s_col[2 * kPnTile + 2];
    __shared__ float s_mean[kPnTile], s_var[kPnTile], s_rvar;
    const NormWrapArgs& a = p.w;
    const int t = threadIdx.x, D = a.D;
    const int c0 = D > kPnTile ? blockIdx.y * kPnTile : 0, W = D > kPnTile ? min(kPnTile, D - c0) : D;
    __builtin_assume(W <= kPnTile);                                                      // (nz_statistics: one pass over the columns)
    const bool tile0 = blockIdx.y == 0;
    const bool upd_obs = a.partials && a.upd_obs, upd_ret = a.partials && a.upd_ret && a.rew && tile0;
    if (upd_obs || upd_ret)                                                              // local column j: sum x of c0 + j | sum x^2 of c0 + j - W | the two of returns
        nz_fold(a.partials, a.rows, 2 * D + 2, 2 * W + 2, [=](int j) { return j < W ? c0 + j : j < 2 * W ? D + c0 + (j - W) : 2 * D + (j - 2 * W); }, s_part, s_col);
    nz_statistics(a, upd_obs, upd_ret, c0, W, tile0, 64, blockIdx.x == 0, s_col, s_mean, s_var, &s_rvar);
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    const bool do_tobs = p.tobs && a.trunc && a.norm_obs;
    if (a.raw || do_tobs) {
        for (int i = t; i < n * W; i += 256) {
            const int e = e0 + i / W, d = i % W; const size_t j = (size_t)e * D + c0 + d;
            if (do_tobs && a.trunc[e]) p.tobs[j] = nz_obs(p.tobs[j], a.st_in[c0 + d], a.st_in[D + c0 + d], a.eps, a.clip_obs);   // terminal_observation, :157-163: the statistics before the following observe
            if (a.raw) {
                float v = a.raw[j];
                if (a.norm_obs) v = nz_obs(v, s_mean[d], s_var[d], a.eps, a.clip_obs);   // observe :123-137: the NEW statistics
                a.obs_out[j] = v;
            }
        }
    }
    if (a.rew && tile0) {
        const float rvar = s_rvar;
        for (int i = t; i < n; i += 256) {
            const int e = e0 + i;
            float rn = a.rew[e];
            if (a.norm_reward) rn = nz_reward(rn, rvar, a.eps, a.clip_reward);
            p.rew_out[e] = rn;
            if ((a.term[e] | a.trunc[e]) != 0) a.returns[e] = 0.f;                        // :152-155
        }
    }
}

}  // namespace
