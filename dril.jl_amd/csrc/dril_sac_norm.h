// dril_sac_norm.h — NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) around the device envs of a SAC handle, for any observation width the
// handle accepts (1 .. 1024).  Included by dril_sac.hip inside its anonymous namespace, after the collection kernels it builds on (CollectEnvArgs, PushArgs,
// sac_env_thread_mu / sac_env_thread_step, phase_stamp).  The PPO handle's wrapper on built-in envs (RmsState: 8 dims, 16-column partial tables) is not touched; its
// wrapper on device env plug-ins (dril_ppo_norm.h) is built like this file and shares dril_norm_math.h with it.
//
// One collected step has ONE grid-wide dependency: every env's raw observation -> the merged statistics -> every env's normalised row -> the actor's next forward.
// So a step is two launches of this file where the plain collection is one:
//   moments   built-in Box envs: sac_norm_env_kernel<KIND> = head -> act! -> raw observe of sac_collect_env_kernel (the same shared definitions), the `returns`
//             recursion, and the block's partial sums; plug-ins: the plug-in's own step kernel, then sac_norm_moments_kernel over the E x D array it wrote
//   apply     sac_norm_apply_kernel: every block folds the partial table in the same fixed order, merges it into the running statistics (update_from_moments! :28-50
//             in float32), normalises reward / terminal observation (OLD observation statistics) / next observation (NEW ones), and pushes the step's row
// A collection's opening observe (off_policy_collection.jl:42) is one more moments + apply pair: at train_freq = 1 that is four launches of this file per env step.
// The statistics live in a ping-pong pair [mean D | var D | ret_mean ret_var]: every block reads the old half, block 0 writes the new one.  The two counts are host
// integers (every update adds n_envs: nothing about them is decided on the device) and travel as kernel arguments.
// Partial table: [rows][2 D + 2] doubles — columns [0, D) sum x, [D, 2 D) sum x^2, 2 D sum returns, 2 D + 1 sum returns^2.  No atomics anywhere: the order of every
// sum is fixed by the launch shape, so two runs give the same bits.
#pragma once

#include "dril_norm_math.h"                     // kNzMaxD, nz_merge, nz_obs: shared with the PPO handle's wrapper on plug-ins (dril_ppo_norm.h)
static_assert(kNzMaxD == DRIL_ENV_PLUGIN_MAX_D, "the wrapper takes every observation width a plug-in may have");
// rows of the partial table of sac_norm_moments_kernel.  Every block of the apply kernel re-reads rows x (2 D + 2) doubles, so for wide rows this trades the moments
// kernel's parallelism (rows x column tiles workgroups) against that fold; 32 is a choice, not a measured optimum (docs/sac.md: 4 096 envs x 512 dims)
constexpr int kNzMaxRows = 32;

// ---- moments, built-in Box envs (A = 1) -----------------------------------------------------------------------------------------------------------------
// The twin of sac_collect_env_kernel without the push: the 16 env threads of a block sit in lanes 0 - 15 of wave 0, so the block's 2 D + 2 sums are four xor
// steps each and one row of the table per block (rows = ceil(E / kEnvsPerBlock)).  env.nobs points at the wrapper's old_obs: the raw next observation.
struct NormEnvArgs { CollectEnvArgs env; float* returns; int upd_ret; float gamma; double* partials; };
template <int KIND>
__global__ __launch_bounds__(256) void sac_norm_env_kernel(NormEnvArgs c) {
    constexpr int D = EnvSpec<KIND>::D, C = 2 * D + 2;
    __shared__ float mu_s[kEnvsPerBlock];
    int e = 0; float mu_e = 0.f;
    const bool own = sac_env_thread_mu(c.env.head, mu_s, &e, &mu_e);
    if (threadIdx.x >= 64) return;                                                       // (no barrier below: the other three waves only served the output layer)
    double acc[C];
#pragma unroll
    for (int i = 0; i < C; ++i) acc[i] = 0;
    if (own) {
        float r, to[D], no[D];
        const StepOut so = sac_env_thread_step<KIND>(c.env, e, mu_e, &r, to, no);
        if (c.upd_ret) {                                                                 // update_reward_stats! :167-171 (done envs go back to zero in the apply kernel)
            const float ret = c.returns[e] * c.gamma + so.rew;
            c.returns[e] = ret; acc[2 * D] = ret; acc[2 * D + 1] = (double)ret * ret;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) { acc[d] = no[d]; acc[D + d] = (double)no[d] * no[d]; }
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
        double v = acc[i];
#pragma unroll
        for (int o = kEnvsPerBlock / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (threadIdx.x == 0) c.partials[(size_t)blockIdx.x * C + i] = v;
    }
}

// ---- moments, any width: over a row-major E x D array (a plug-in's step / observe kernel wrote it; the collection's first observe of every kind) ---------------
// grid (rows, column tiles): block (b, y) owns the envs [b R, b R + R) and writes row b of the table.
//   D > 64   a thread owns ONE column (column tile y: 256 columns): consecutive lanes read consecutive floats of an env's row, the sum over the block's envs stays in
//            the thread — no reduction at all.
//   D <= 64  one tile; a wave reads floor(64 / D) whole envs at a time, lane l the flat element l of that run (column l % D): contiguous along the flattened
//            array.  Lanes of equal column are folded by a shuffle tree over multiples of D — all D columns of the wave at once, in log2 steps — then the four waves
//            through LDS in wave order.
// rew != null: also the `returns` recursion of act! and its two sums (tile 0).  All sums in f64.
struct NzMomArgs { int E, D, R; const float* raw; const float* rew; float* returns; float gamma; double* partials; };
__global__ __launch_bounds__(256) void sac_norm_moments_kernel(NzMomArgs a) {
    __shared__ double sh[2][4][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, D = a.D, C = 2 * D + 2;
    const int e0 = blockIdx.x * a.R, e1 = min(a.E, e0 + a.R);
    double* row = a.partials + (size_t)blockIdx.x * C;
    if (a.raw) {
        if (D > 64) {
            const int col = blockIdx.y * 256 + t;
            if (col < D) {
                double s = 0, q = 0;
#pragma unroll 4
                for (int e = e0; e < e1; ++e) { const float v = a.raw[(size_t)e * D + col]; s += v; q += (double)v * v; }
                row[col] = s; row[D + col] = q;
            }
        } else {
            const int G = 64 / D, Sw = G * D, g = lane / D;
            double s = 0, q = 0;
            if (lane < Sw)
                for (int e = e0 + wave * G + g; e < e1; e += 4 * G) { const float v = a.raw[(size_t)e * D + (lane - g * D)]; s += v; q += (double)v * v; }
            int P = 1; while (P < G) P <<= 1;
            for (int hh = P >> 1; hh > 0; hh >>= 1) {                                   // group g < hh takes group g + hh: lane l takes lane l + hh D
                const double s2 = __shfl_down(s, hh * D), q2 = __shfl_down(q, hh * D);
                if (g < hh && g + hh < G && lane < Sw) { s += s2; q += q2; }
            }
            if (lane < D) { sh[0][wave][lane] = s; sh[1][wave][lane] = q; }
            __syncthreads();
            if (t < D) {
                row[t] = ((sh[0][0][t] + sh[0][1][t]) + sh[0][2][t]) + sh[0][3][t];
                row[D + t] = ((sh[1][0][t] + sh[1][1][t]) + sh[1][2][t]) + sh[1][3][t];
            }
            __syncthreads();
        }
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

// ---- apply + push -----------------------------------------------------------------------------------------------------------------------------------------
// Block b owns the envs [b epb, b epb + epb).  Head: the column sums of the table (all 256 threads: columns x row segments in flight together, the segments then
// summed in index order — D block-wide reductions one after the other would be D dependent round trips), the merge, the new statistics in LDS; block 0 stores them
// to st_out.  Body: flat (env, dim) loops, so a wave's loads and its stores into obs_out and the ring are contiguous runs for any D.
// rew == null: observe alone (the collection's first observe; a read-only peek with partials == null); push.E == 0: no ring write.
struct NzApplyArgs {
    int E, D, rows, epb; const double* partials; int upd_obs, upd_ret, norm_obs, norm_reward; long long obs_count, ret_count;
    float clip_obs, clip_reward, eps; const float* st_in; float* st_out;
    const float* raw; float* obs_out;                                                    // raw (E x D): the wrapper's old_obs; obs_out: what the actor reads next
    const float* rew; float* old_rew; float* returns; const uint8_t *term, *trunc; const float* tobs;
    PushArgs push;                                                                       // push.obs: the normalised observation the action was chosen on
};
static_assert(sizeof(double) * (256 + 2 * (size_t)kNzMaxD + 2) + sizeof(float) * (2 * (size_t)kNzMaxD + 2) <= 48 * 1024, "sac_norm_apply_kernel's dynamic LDS at the widest observation");
inline size_t nz_apply_lds(int D) { return sizeof(double) * (256 + 2 * (size_t)D + 2) + sizeof(float) * (2 * (size_t)D + 2); }
__global__ __launch_bounds__(256) void sac_norm_apply_kernel(NzApplyArgs a) {
    extern __shared__ double nz_sh[];
    const int t = threadIdx.x, D = a.D, C = 2 * D + 2;
    double* s_part = nz_sh; double* s_col = nz_sh + 256;
    float* s_mean = reinterpret_cast<float*>(s_col + C); float* s_var = s_mean + D; float* s_rvar = s_var + D;
    const bool upd_obs = a.partials && a.upd_obs, upd_ret = a.partials && a.upd_ret && a.rew;
    if (upd_obs || upd_ret) {
        for (int c0 = 0; c0 < C; c0 += 256) {
            const int Ct = min(256, C - c0), nseg = 256 / Ct;
            if (t < nseg * Ct) {
                const int col = t % Ct, seg = t / Ct;
                double u = 0;
#pragma unroll 4
                for (int b = seg; b < a.rows; b += nseg) u += a.partials[(size_t)b * C + c0 + col];
                s_part[t] = u;
            }
            __syncthreads();
            if (t < Ct) { double u = 0; for (int sg = 0; sg < nseg; ++sg) u += s_part[sg * Ct + t]; s_col[c0 + t] = u; }
            __syncthreads();
        }
    }
    for (int d = t; d < D; d += 256) {
        float mean = a.st_in[d], var = a.st_in[D + d];
        if (upd_obs) {
            const double bm = s_col[d] / a.E; double bv = s_col[D + d] / a.E - bm * bm; if (bv < 0) bv = 0;   // mean / var(corrected = false), :21-26
            nz_merge(mean, var, a.obs_count, (float)bm, (float)bv, a.E);
        }
        s_mean[d] = mean; s_var[d] = var;
        if (blockIdx.x == 0 && a.st_out) { a.st_out[d] = mean; a.st_out[D + d] = var; }
    }
    if (t == 0) {
        float mean = a.st_in[2 * D], var = a.st_in[2 * D + 1];
        if (upd_ret) {
            const double bm = s_col[2 * D] / a.E; double bv = s_col[2 * D + 1] / a.E - bm * bm; if (bv < 0) bv = 0;
            nz_merge(mean, var, a.ret_count, (float)bm, (float)bv, a.E);
        }
        *s_rvar = var;
        if (blockIdx.x == 0 && a.st_out) { a.st_out[2 * D] = mean; a.st_out[2 * D + 1] = var; }
    }
    __syncthreads();
    const int e0 = blockIdx.x * a.epb, n = min(a.epb, a.E - e0);
    const bool push = a.push.E > 0;
    for (int i = t; i < n * D; i += 256) {
        const int e = e0 + i / D, d = i % D; const size_t j = (size_t)e * D + d;
        float v = a.raw[j];
        if (a.norm_obs) v = nz_obs(v, s_mean[d], s_var[d], a.eps, a.clip_obs);           // observe :123-137: the NEW statistics
        a.obs_out[j] = v;
        if (push) {
            const long long slot = (a.push.tail + e) % a.push.cap;
            a.push.rb_obs[slot * D + d] = a.push.obs[j];
            if (a.trunc[e]) {                                                            // terminal_observation, :157-163: the statistics as they are before this observe
                v = a.tobs[j];
                if (a.norm_obs) v = nz_obs(v, a.st_in[d], a.st_in[D + d], a.eps, a.clip_obs);
            }
            a.push.rb_next[slot * D + d] = v;                                            // truncated_observation | next observation
        }
    }
    if (a.rew) {
        const float rvar = *s_rvar;
        for (int i = t; i < n; i += 256) {
            const int e = e0 + i;
            const float r = a.rew[e];
            a.old_rew[e] = r;
            float rn = r;
            if (a.norm_reward) { rn = r / sqrtf(rvar + a.eps); rn = fminf(fmaxf(rn, -a.clip_reward), a.clip_reward); }   // normalize_rewards! :188-197 (no mean)
            const bool term = a.term[e] != 0, trunc = a.trunc[e] != 0;
            if (term || trunc) a.returns[e] = 0.f;                                       // :152-155
            if (push) { const long long slot = (a.push.tail + e) % a.push.cap; a.push.rb_rew[slot] = rn; a.push.rb_term[slot] = term; a.push.rb_trunc[slot] = trunc; }
        }
    }
    if (push) {
        const int A = a.push.A;
        for (int i = t; i < n * A; i += 256) {
            const int e = e0 + i / A, k = i % A;
            a.push.rb_act[((a.push.tail + e) % a.push.cap) * A + k] = a.push.raw[(size_t)e * A + k];   // unprocessed action, off_policy_collection.jl:72
        }
    }
    phase_stamp(a.push.stamp);
}

// ---- evaluation: the frozen statistics, no moments, no added launch per step ------------------------------------------------------------------------------
struct NzEvalArgs { const float* st; int norm_obs; float eps, clip; };                   // st == null: the wrapper is off
// plug-ins: the accounting launch that already follows the plug-in's step kernel also normalises the observation that kernel wrote, in place
__global__ __launch_bounds__(256) void sac_eval_account_norm_kernel(EvalAcctArgs a, const float* __restrict__ rew, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
                                                                    NzEvalArgs nz, int D, float* obs) {
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (i0 < a.E) sac_eval_account(a, i0, rew[i0], (term[i0] | trunc[i0]) != 0);
    for (long long i = i0; i < (long long)a.E * D; i += stride) { const int d = (int)(i % D); obs[i] = nz_obs(obs[i], nz.st[d], nz.st[D + d], nz.eps, nz.clip); }
}
