// dril_ppo_norm.h — NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) around the device env plug-in of a PPO handle (dril_normalize_enable,
// include/dril_hip.h), for every observation width a plug-in may have (1 .. 1024).  Included by dril_api.hip inside its anonymous namespace.  Built-in envs keep
// their own wrapper (cfg.norm_*: RmsState with 8 dims, the fused norm_step_kernel / norm_apply_kernel of dril_kernels.hip); this file is never launched for them.
//
// The structure is that of dril_sac_norm.h, whose two scalar definitions (nz_merge, nz_obs: dril_norm_math.h) it shares: one env step has ONE grid-wide dependency —
// every env's raw observation -> the merged statistics -> every env's normalised row -> the policy's next forward — so after the plug-in's own step kernel (raw
// reward, flags, terminal observation and next observation into the per-step arrays) two launches follow:
//   moments   ppo_norm_moments_kernel over the E x D raw observations and the E rewards: per-dimension sum x / sum x^2, the `returns` recursion of act! and its two
//             sums, one row of the partial table [rows][2 D + 2] (f64) per workgroup row
//   apply     ppo_norm_apply_kernel: every block folds the columns it needs of the table (or reads the one all-reduced row of a data-parallel job) in the same fixed
//             order, merges them into the running statistics (update_from_moments! :28-50 in float32), writes the normalised reward into the rollout row,
//             normalises the terminal observation of truncated envs with the OLD observation statistics and the next observation with the NEW ones
// The opening observe of a rollout and dril_env_observe are the same two launches with the reward half off; dril_env_step is the pair with the observation half off.
// Statistics: a ping-pong pair [mean D | var D | ret_mean ret_var]; every block reads the old half, the blocks of env range 0 write the new one.  The two counts are
// host integers and travel as kernel arguments.  No atomics: the launch shape fixes the order of every sum, so two runs give the same bits.
//
// What differs from the SAC kernels, and why: PPO collects with many envs per step (the rollout is E x T, T short), so both kernels are laid out for E up to 65 536:
//   * observations wider than 64 are cut into column tiles of 64 (one wave's width) in BOTH kernels.  The moments kernel then has rows x tiles workgroups (the SAC
//     kernel: at most 32 x ceil(D / 256)), and an apply block folds only its tile's 2 x 64 (+ 2) columns instead of all 2 D + 2;
//   * the table may have up to 256 rows for narrow observations: kPnFoldDoubles bounds what one apply block re-reads (rows x folded columns), not a fixed row count.
#pragma once

#include "dril_norm_math.h"

constexpr int kPnTile = 64;            // columns per tile when D > 64: a wave reads 64 consecutive floats of an env's row
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

// ---- moments ---------------------------------------------------------------------------------------------------------------------------------------------------------
// grid (rows, tiles): block (b, y) owns the envs [b R, b R + R) and the columns of tile y, and writes its part of row b of the table.
//   D > 64   lane l of every wave owns column 64 y + l; wave w takes the envs e0 + w, e0 + w + 4, ...: each load of a wave is 64 consecutive floats of one env's
//            row.  The sums stay in the thread; the four waves meet in LDS and are added in wave order.
//   D <= 64  one tile; a wave reads floor(64 / D) whole envs at a time, lane l the flat element l of that run: contiguous along the flattened (env, dim) array.
//            Lanes of equal column are folded by a shuffle tree over multiples of D, then the four waves through LDS in wave order (as sac_norm_moments_kernel).
// rew != null: also the `returns` recursion of act! (:167-171) and its two sums, by the blocks of tile 0.  All sums in f64.
struct PnMomArgs { int E, D, R; const float* raw; const float* rew; float* returns; float gamma; double* partials; };
__global__ __launch_bounds__(256) void ppo_norm_moments_kernel(PnMomArgs a) {
    __shared__ double sh[2][4][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, D = a.D, C = 2 * D + 2;
    const int e0 = blockIdx.x * a.R, e1 = min(a.E, e0 + a.R);
    double* row = a.partials + (size_t)blockIdx.x * C;
    if (a.raw) {
        double s = 0, q = 0;
        int ncol, c0 = 0;                                                                // columns this block writes: [c0, c0 + ncol)
        if (D > kPnTile) {
            c0 = blockIdx.y * kPnTile; ncol = min(kPnTile, D - c0);
            if (lane < ncol) {
#pragma unroll 4
                for (int e = e0 + wave; e < e1; e += 4) { const float v = a.raw[(size_t)e * D + c0 + lane]; s += v; q += (double)v * v; }
            }
        } else {
            ncol = D;
            const int G = 64 / D, Sw = G * D, g = lane / D;
            if (lane < Sw)
                for (int e = e0 + wave * G + g; e < e1; e += 4 * G) { const float v = a.raw[(size_t)e * D + (lane - g * D)]; s += v; q += (double)v * v; }
            int P = 1; while (P < G) P <<= 1;
            for (int hh = P >> 1; hh > 0; hh >>= 1) {                                   // group g < hh takes group g + hh: lane l takes lane l + hh D
                const double s2 = __shfl_down(s, hh * D), q2 = __shfl_down(q, hh * D);
                if (g < hh && g + hh < G && lane < Sw) { s += s2; q += q2; }
            }
        }
        if (lane < ncol) { sh[0][wave][lane] = s; sh[1][wave][lane] = q; }
        __syncthreads();
        if (t < ncol) {
            row[c0 + t] = ((sh[0][0][t] + sh[0][1][t]) + sh[0][2][t]) + sh[0][3][t];
            row[D + c0 + t] = ((sh[1][0][t] + sh[1][1][t]) + sh[1][2][t]) + sh[1][3][t];
        }
        __syncthreads();
    }
    if (a.rew && blockIdx.y == 0) {                                                      // (uniform per block: the barrier below is reached by all of it)
        double s = 0, q = 0;
        for (int e = e0 + t; e < e1; e += 256) { const float ret = a.returns[e] * a.gamma + a.rew[e]; a.returns[e] = ret; s += ret; q += (double)ret * ret; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
        if (lane == 0) { sh[0][wave][0] = s; sh[1][wave][0] = q; }
        __syncthreads();
        if (t == 0) {
            row[2 * D] = ((sh[0][0][0] + sh[0][1][0]) + sh[0][2][0]) + sh[0][3][0];
            row[2 * D + 1] = ((sh[1][0][0] + sh[1][1][0]) + sh[1][2][0]) + sh[1][3][0];
        }
    }
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
// Head: the column sums it needs — W of sum x, W of sum x^2 and, for tile 0, the two of `returns` — over the table's rows: columns x row segments in flight
// together, the segments then summed in index order; then the merge, the new statistics of its columns in LDS; the blocks b == 0 store theirs to st_out.
// Body: flat (env, column) loop, so a wave's loads and stores are contiguous runs of the arrays for any D.
// raw == null: act! alone (dril_env_step); rew == null: observe alone; partials == null: nothing is updated (frozen statistics, or a read-only pass).
struct PnApplyArgs {
    int E, D, rows, epb; const double* partials; int upd_obs, upd_ret, norm_obs, norm_reward; long long obs_count, ret_count, n;   // n: the envs behind the table's sums
    float clip_obs, clip_reward, eps; const float* st_in; float* st_out;
    const float* raw; float* obs_out;                                                    // raw (E x D): the wrapper's old_obs; obs_out: what the policy reads next
    const float* rew; float* rew_out; float* returns; const uint8_t *term, *trunc; float* tobs;   // tobs (E x D): normalised in place where truncated
};
__global__ __launch_bounds__(256) void ppo_norm_apply_kernel(PnApplyArgs a) {
    __shared__ double s_part[256], s_col[2 * kPnTile + 2];
    __shared__ float s_mean[kPnTile], s_var[kPnTile], s_rvar;
    const int t = threadIdx.x, D = a.D;
    const int c0 = D > kPnTile ? blockIdx.y * kPnTile : 0, W = D > kPnTile ? min(kPnTile, D - c0) : D;
    const bool tile0 = blockIdx.y == 0;
    const bool upd_obs = a.partials && a.upd_obs, upd_ret = a.partials && a.upd_ret && a.rew && tile0;
    if (upd_obs || upd_ret) {
        const int nc = 2 * W + 2, nseg = 256 / nc, C = 2 * D + 2;                        // local column j: sum x of c0 + j | sum x^2 of c0 + j - W | the two of returns
        if (t < nseg * nc) {
            const int j = t % nc, seg = t / nc;
            const int col = j < W ? c0 + j : j < 2 * W ? D + c0 + (j - W) : 2 * D + (j - 2 * W);
            double u = 0;
#pragma unroll 4
            for (int b = seg; b < a.rows; b += nseg) u += a.partials[(size_t)b * C + col];
            s_part[t] = u;
        }
        __syncthreads();
        if (t < nc) { double u = 0; for (int sg = 0; sg < nseg; ++sg) u += s_part[sg * nc + t]; s_col[t] = u; }
        __syncthreads();
    }
    const bool store = blockIdx.x == 0 && a.st_out;
    if (t < W) {
        float mean = a.st_in[c0 + t], var = a.st_in[D + c0 + t];
        if (upd_obs) {
            const double bm = s_col[t] / (double)a.n; double bv = s_col[W + t] / (double)a.n - bm * bm; if (bv < 0) bv = 0;   // mean / var(corrected = false), :21-26
            nz_merge(mean, var, a.obs_count, (float)bm, (float)bv, a.n);
        }
        s_mean[t] = mean; s_var[t] = var;
        if (store) { a.st_out[c0 + t] = mean; a.st_out[D + c0 + t] = var; }
    }
    if (t == 64 && tile0) {
        float mean = a.st_in[2 * D], var = a.st_in[2 * D + 1];
        if (upd_ret) {
            const double bm = s_col[2 * W] / (double)a.n; double bv = s_col[2 * W + 1] / (double)a.n - bm * bm; if (bv < 0) bv = 0;
            nz_merge(mean, var, a.ret_count, (float)bm, (float)bv, a.n);
        }
        s_rvar = var;
        if (store) { a.st_out[2 * D] = mean; a.st_out[2 * D + 1] = var; }
    }
    __syncthreads();
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    const bool do_tobs = a.tobs && a.trunc && a.norm_obs;
    if (a.raw || do_tobs) {
        for (int i = t; i < n * W; i += 256) {
            const int e = e0 + i / W, d = i % W; const size_t j = (size_t)e * D + c0 + d;
            if (do_tobs && a.trunc[e]) a.tobs[j] = nz_obs(a.tobs[j], a.st_in[c0 + d], a.st_in[D + c0 + d], a.eps, a.clip_obs);   // terminal_observation, :157-163: the statistics before the following observe
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
            if (a.norm_reward) { rn = rn / sqrtf(rvar + a.eps); rn = fminf(fmaxf(rn, -a.clip_reward), a.clip_reward); }   // normalize_rewards! :188-197 (no mean)
            a.rew_out[e] = rn;
            if ((a.term[e] | a.trunc[e]) != 0) a.returns[e] = 0.f;                        // :152-155
        }
    }
}
