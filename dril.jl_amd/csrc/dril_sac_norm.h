// dril_sac_norm.h — what is the SAC handle's own of NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) around its device envs, for any
// observation width the handle accepts (1 .. 1024).  Everything it shares with the PPO handle's wrapper on device env plug-ins (dril_ppo_norm.h) — scalars, the
// moments kernel, the head of the apply kernel, the host state — is dril_norm_wrap.h, which dril_sac.hip includes first; this file is included inside its anonymous
// namespace, after the collection kernels it builds on (CollectEnvArgs, PushArgs, sac_env_thread_mu / sac_env_thread_step, phase_stamp).
//
// A collected step is two launches of the wrapper where the plain collection is one:
//   moments   built-in Box envs: sac_norm_env_kernel<KIND> = head -> act! -> raw observe of sac_collect_env_kernel (the same shared definitions), the `returns`
//             recursion, and the block's partial sums; plug-ins: the plug-in's own step kernel, then norm_moments_kernel<kNzTile> over the E x D array it wrote
//   apply     sac_norm_apply_kernel: every block folds the partial table in the same fixed order, merges it into the running statistics, normalises reward /
//             terminal observation (OLD observation statistics) / next observation (NEW ones), and pushes the step's row
// A collection's opening observe (off_policy_collection.jl:42) is one more moments + apply pair: at train_freq = 1 that is four launches of the wrapper per env step.
#pragma once

static_assert(kNzMaxD == DRIL_ENV_PLUGIN_MAX_D, "the wrapper takes every observation width a plug-in may have");
// rows of the partial table of norm_moments_kernel<kNzTile>.  Every block of the apply kernel re-reads rows x (2 D + 2) doubles, so for wide rows this trades the moments
// kernel's parallelism (rows x column tiles workgroups) against that fold; 32 is a choice, not a measured optimum (docs/sac.md: 4 096 envs x 512 dims)
constexpr int kNzMaxRows = 32;
constexpr int kNzTile = 256;                    // columns per tile of the moments kernel when D > 64: with so few rows a thread per column, no reduction

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

// ---- apply + push -----------------------------------------------------------------------------------------------------------------------------------------
// Block b owns the envs [b epb, b epb + epb) and keeps the statistics of all D columns in (dynamic) LDS.  Head (dril_norm_wrap.h): the column sums of the table, 256
// columns at a time, the merge, the new statistics in LDS; block 0 stores them to st_out.  Body: flat (env, dim) loops, so a wave's loads and its stores into obs_out
// and the ring are contiguous runs for any D.
// rew == null: observe alone (the collection's first observe; a read-only peek with partials == null); push.E == 0: no ring write.
struct NzApplyArgs {
    NormWrapArgs w; float* old_rew; const float* tobs;
    PushArgs push;                                                                       // push.obs: the normalised observation the action was chosen on
};
static_assert(sizeof(double) * (256 + 2 * (size_t)kNzMaxD + 2) + sizeof(float) * (2 * (size_t)kNzMaxD + 2) <= 48 * 1024, "sac_norm_apply_kernel's dynamic LDS at the widest observation");
inline size_t nz_apply_lds(int D) { return sizeof(double) * (256 + 2 * (size_t)D + 2) + sizeof(float) * (2 * (size_t)D + 2); }
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

// ---- evaluation: the frozen statistics, no moments, no added launch per step ------------------------------------------------------------------------------
struct NzEvalArgs { const float* st; int norm_obs; float eps, clip; };                   // st == null: the wrapper is off
// plug-ins: the accounting launch that already follows the plug-in's step kernel also normalises the observation that kernel wrote, in place
__global__ __launch_bounds__(256) void sac_eval_account_norm_kernel(EvalAcctArgs a, const float* __restrict__ rew, const uint8_t* __restrict__ term, const uint8_t* __restrict__ trunc,
                                                                    NzEvalArgs nz, int D, float* obs) {
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (i0 < a.E) sac_eval_account(a, i0, rew[i0], (term[i0] | trunc[i0]) != 0);
    for (long long i = i0; i < (long long)a.E * D; i += stride) { const int d = (int)(i % D); obs[i] = nz_obs(obs[i], nz.st[d], nz.st[D + d], nz.eps, nz.clip); }
}
