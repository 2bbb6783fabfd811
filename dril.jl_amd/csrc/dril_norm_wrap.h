// dril_norm_wrap.h — NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) for any observation width (1 .. 1024), once: every rule of the wrapper
// that the PPO handle (around a device env plug-in: dril_normalize_*, dril_ppo_norm.h) and the SAC handle (dril_sac_normalize_*, dril_sac_norm.h) both implement.
// The two handle headers hold what is theirs alone: the apply kernels (different launch shapes; SAC's also writes the replay ring) and the kernels without a twin.
// The PPO handle's wrapper on built-in envs (RmsState: 8 dims, fused into the env step, dril_kernels.hip) takes the scalars from here and nothing else.
//
// One env step has ONE grid-wide dependency — every env's raw observation -> the merged statistics -> every env's normalised row -> the next forward — so a step is
// two launches: moments (norm_moments_kernel: one row of the partial table per workgroup row) and the handle's apply kernel (fold of the table, merge, normalise).
//   partial table   [rows][2 D + 2] doubles — columns [0, D) sum x, [D, 2 D) sum x^2, 2 D sum returns, 2 D + 1 sum returns^2
//   statistics      a ping-pong pair [2][mean D | var D | ret_mean ret_var]: every block reads the half in force, block row 0 writes the other, which is then in force
//   counts          host integers (every update adds the number of envs behind the sums: nothing about them is decided on the device); they travel as kernel arguments
// No atomics anywhere: the launch shape fixes the order of every sum, so two runs give the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dril_hip.h"              // dril_normalize_config (the one configuration type in here), the DRIL_ERR_* codes
#include "../../include/device/dril_normalize.h" // normalize_obs: the one definition, shared with the evaluation kernel of a device env plug-in
#include "dril_devmem.h"                         // DevBuf: the wrapper owns its statistics and its table

namespace {

constexpr int kNzMaxD = 1024;                    // the widest observation the wrapper takes (DRIL_ENV_PLUGIN_MAX_D); sizes the SAC apply kernel's LDS

// ---- scalars ------------------------------------------------------------------------------------------------------------------------------------------------------
// update_from_moments! (:28-50) in the reference's float32 arithmetic
__device__ __forceinline__ void nz_merge(float& mean, float& var, long long count, float bmean, float bvar, long long bcount) {
    if (count == 0) { mean = bmean; var = bvar; return; }
    const long long tot = count + bcount;
    const float delta = bmean - mean;
    const float new_mean = mean + delta * (float)bcount / (float)tot;
    const float m_a = var * (float)count, m_b = bvar * (float)bcount;
    const float M2 = m_a + m_b + delta * delta * (float)count * (float)bcount / (float)tot;
    mean = new_mean; var = M2 / (float)tot;
}
// update! (:21-26) from a column's f64 sums over n envs: mean / var(corrected = false) of the batch, then the merge
__device__ __forceinline__ void nz_merge_sums(float& mean, float& var, long long count, double sum, double sumsq, long long n) {
    const double bm = sum / (double)n; double bv = sumsq / (double)n - bm * bm; if (bv < 0) bv = 0;
    nz_merge(mean, var, count, (float)bm, (float)bv, n);
}
// normalize_obs! (:174-179)
__device__ __forceinline__ float nz_obs(float v, float mean, float var, float eps, float clip) { return dril::normalize_obs(v, mean, var, eps, clip); }
// normalize_rewards! (:188-197): no mean subtraction
__device__ __forceinline__ float nz_reward(float r, float var, float eps, float clip) {
    r = r / sqrtf(var + eps);
    return fminf(fmaxf(r, -clip), clip);
}

// ---- moments: over a row-major E x D array and / or the E rewards ---------------------------------------------------------------------------------------------------
// grid (rows, column tiles): block (b, y) owns the envs [b R, b R + R) and writes its part of row b of the table.
//   D <= 64  one tile; a wave reads floor(64 / D) whole envs at a time, lane l the flat element l of that run (column l % D): contiguous along the flattened
//            array.  Lanes of equal column are folded by a shuffle tree over multiples of D — all D columns of the wave at once, in log2 steps — then the four waves
//            meet in LDS and are added in wave order.
//   D > 64   the 256 threads are TILE columns x 256 / TILE env strides, the sums over a thread's envs stay in the thread.  The two handles tile differently because
//            they collect differently:
//              TILE = 64  (PPO: many envs per step, E up to 65 536)  lane l of every wave owns column 64 y + l, wave w the envs e0 + w, e0 + w + 4, ...: rows x tiles
//                         workgroups, and an apply block folds only its tile's columns.  The four waves meet in LDS as above.
//              TILE = 256 (SAC: at most 32 rows)  a thread owns ONE column over all the block's envs — no reduction at all, the sums go straight to the table.
// rew != null: also the `returns` recursion of act! (:167-171) and its two sums, by the blocks of tile 0.  All sums in f64.
struct NormMomArgs { int E, D, R; const float* raw; const float* rew; float* returns; float gamma; double* partials; };
template <int TILE>
__global__ __launch_bounds__(256) void norm_moments_kernel(NormMomArgs a) {
    static_assert(TILE == 64 || TILE == 256, "a wave per env stride (the LDS meet below) or one stride");
    __shared__ double sh[2][4][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, D = a.D, C = 2 * D + 2;
    const int e0 = blockIdx.x * a.R, e1 = min(a.E, e0 + a.R);
    double* row = a.partials + (size_t)blockIdx.x * C;
    if (a.raw) {
        double s = 0, q = 0;
        int ncol = D, c0 = 0;                                                            // columns this block writes: [c0, c0 + ncol)
        if (D > 64) {
            c0 = blockIdx.y * TILE; ncol = min(TILE, D - c0);
            const int j = t % TILE;
            if (j < ncol) {
#pragma unroll 4
                for (int e = e0 + t / TILE; e < e1; e += 256 / TILE) { const float v = a.raw[(size_t)e * D + c0 + j]; s += v; q += (double)v * v; }
                if constexpr (TILE == 256) { row[c0 + j] = s; row[D + c0 + j] = q; }
            }
        } else {
            const int G = 64 / D, Sw = G * D, g = lane / D;
            if (lane < Sw)
                for (int e = e0 + wave * G + g; e < e1; e += 4 * G) { const float v = a.raw[(size_t)e * D + (lane - g * D)]; s += v; q += (double)v * v; }
            int P = 1; while (P < G) P <<= 1;
            for (int hh = P >> 1; hh > 0; hh >>= 1) {                                   // group g < hh takes group g + hh: lane l takes lane l + hh D
                const double s2 = __shfl_down(s, hh * D), q2 = __shfl_down(q, hh * D);
                if (g < hh && g + hh < G && lane < Sw) { s += s2; q += q2; }
            }
        }
        if (TILE == 64 || D <= 64) {                                                     // (uniform per block)
            if (lane < ncol) { sh[0][wave][lane] = s; sh[1][wave][lane] = q; }
            __syncthreads();
            if (t < ncol) {
                row[c0 + t] = ((sh[0][0][t] + sh[0][1][t]) + sh[0][2][t]) + sh[0][3][t];
                row[D + c0 + t] = ((sh[1][0][t] + sh[1][1][t]) + sh[1][2][t]) + sh[1][3][t];
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

// ---- the head of an apply kernel --------------------------------------------------------------------------------------------------------------------------------------
// what both apply kernels take.  raw == null: act! alone; rew == null: observe alone; partials == null: nothing is updated (frozen statistics, or a read-only pass)
struct NormWrapArgs {
    int E, D, rows, epb; const double* partials; int upd_obs, upd_ret, norm_obs, norm_reward; long long obs_count, ret_count, n;   // n: the envs behind the table's sums
    float clip_obs, clip_reward, eps; const float* st_in; float* st_out;
    const float* raw; float* obs_out;                                                    // raw (E x D): the wrapper's old_obs; obs_out: what the policy reads next
    const float* rew; float* returns; const uint8_t *term, *trunc;
};
// column sums of the table with all 256 threads: nc (<= 256) columns x floor(256 / nc) row segments in flight together, the segments then summed in index order (one
// block-wide reduction per column would be that many dependent round trips).  col(j): the table column of local column j; out[j]: its sum.  Ends on a barrier.
template <typename Col>
__device__ __forceinline__ void nz_fold(const double* __restrict__ partials, int rows, int C, int nc, Col col, double* s_part, double* out) {
    const int t = threadIdx.x, nseg = 256 / nc;
    if (t < nseg * nc) {
        const int c = col(t % nc), seg = t / nc;
        double u = 0;
#pragma unroll 4
        for (int b = seg; b < rows; b += nseg) u += partials[(size_t)b * C + c];
        s_part[t] = u;
    }
    __syncthreads();
    if (t < nc) { double u = 0; for (int sg = 0; sg < nseg; ++sg) u += s_part[sg * nc + t]; out[t] = u; }
    __syncthreads();
}
// the statistics of the columns [c0, c0 + W) and, where with_ret, of `returns` (thread ret_thread): the half in force, merged with the folded sums s_col
// [sum x W | sum x^2 W | returns 2] where the launch updates, into LDS; the blocks with store set write them to the other half.  Ends on a barrier.
__device__ __forceinline__ void nz_statistics(const NormWrapArgs& a, bool upd_obs, bool upd_ret, int c0, int W, bool with_ret, int ret_thread, bool store,
                                              const double* s_col, float* s_mean, float* s_var, float* s_rvar) {
    const int t = threadIdx.x, D = a.D;
    store = store && a.st_out;
    for (int d = t; d < W; d += 256) {
        float mean = a.st_in[c0 + d], var = a.st_in[D + c0 + d];
        if (upd_obs) nz_merge_sums(mean, var, a.obs_count, s_col[d], s_col[W + d], a.n);
        s_mean[d] = mean; s_var[d] = var;
        if (store) { a.st_out[c0 + d] = mean; a.st_out[D + c0 + d] = var; }
    }
    if (t == ret_thread && with_ret) {
        float mean = a.st_in[2 * D], var = a.st_in[2 * D + 1];
        if (upd_ret) nz_merge_sums(mean, var, a.ret_count, s_col[2 * W], s_col[2 * W + 1], a.n);
        *s_rvar = var;
        if (store) { a.st_out[2 * D] = mean; a.st_out[2 * D + 1] = var; }
    }
    __syncthreads();
}

// ---- host: the wrapper's state on a handle, and the rules of the verb families ------------------------------------------------------------------------------------
// A rule that can fail returns (code, message); the message is what follows "<verb>: " in the handle's error text.
struct NormErr { int code = DRIL_OK; std::string msg; explicit operator bool() const { return code != DRIL_OK; } };

// the keyword defaults of normalizeWrapperEnv.jl:71-80
inline void norm_config_default(dril_normalize_config* c) {
    std::memset(c, 0, sizeof(*c));
    c->training = 1; c->norm_obs = 1; c->norm_reward = 1; c->clip_obs = 10.0f; c->clip_reward = 10.0f; c->gamma = 0.99f; c->epsilon = 1.0e-8f;
}
inline NormErr norm_config_check(const dril_normalize_config& c, int D) {
    if (!(c.clip_obs >= 0.f) || !(c.clip_reward >= 0.f)) return {DRIL_ERR_INVALID_ARG, "clip_obs and clip_reward must be >= 0"};
    if (!(c.epsilon >= 0.f)) return {DRIL_ERR_INVALID_ARG, "epsilon must be >= 0"};
    if (D > kNzMaxD) return {DRIL_ERR_UNSUPPORTED, "the wrapper's kernels hold up to " + std::to_string(kNzMaxD) + " observation dims"};
    return {};
}
inline dril_normalize_config norm_config_canonical(dril_normalize_config c) {
    c.training = c.training != 0; c.norm_obs = c.norm_obs != 0; c.norm_reward = c.norm_reward != 0; c.reserved = 0;
    return c;
}
inline NormErr norm_set_stats_check(const float* obs_mean, const float* obs_var, int64_t obs_count, int64_t ret_count) {
    if (!obs_mean || !obs_var) return {DRIL_ERR_INVALID_ARG, "null statistics pointer"};
    if (obs_count < 0 || ret_count < 0) return {DRIL_ERR_INVALID_ARG, "counts must be >= 0"};
    return {};
}

struct NormWrap {
    bool on = false; dril_normalize_config cfg{}; int D = 0, cur = 0; int64_t obs_count = 0, ret_count = 0;
    dril::DevBuf<float> stats; dril::DevBuf<double> partials;

    float* half(int i) const { return stats + (size_t)i * (2 * D + 2); }
    size_t stats_floats() const { return 2 * (size_t)D + 2; }
    void release() {
        stats.release(); partials.release(); on = false; cur = 0; obs_count = ret_count = 0;
    }
    // a fresh wrapper over observations of width D_: RunningMeanStd() — mean 0, var 1, count 0 (:12-16) — in both halves, a zeroed table of `rows` rows.  `on` is the caller's
    // to set once its own arrays stand too
    hipError_t alloc(int D_, size_t rows) {
        release(); D = D_;
        const size_t C = stats_floats();
        hipError_t e = stats.alloc(2 * C);
        if (e == hipSuccess) e = partials.alloc_zero(rows * C);
        if (e == hipSuccess) {
            std::vector<float> st(2 * C, 0.f);
            for (size_t hf = 0; hf < 2; ++hf) { for (int d = 0; d < D; ++d) st[hf * C + D + d] = 1.0f; st[hf * C + 2 * D + 1] = 1.0f; }
            e = hipMemcpy(stats, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice);
        }
        return e;
    }
    // enable on a handle that has the wrapper: the same configuration (training apart, which is then set as set_training would) keeps statistics and returns
    bool keeps(const dril_normalize_config& c) {
        dril_normalize_config a = c, b = cfg; a.training = b.training = 0;
        if (!on || std::memcmp(&a, &b, sizeof(a)) != 0) return false;
        cfg.training = c.training;
        return true;
    }
    // [mean D | var D | ret_mean ret_var] as the verbs exchange it; null out pointers are skipped
    void unpack(const std::vector<float>& st, float* obs_mean, float* obs_var, int64_t* obs_count_, float* ret_mean, float* ret_var, int64_t* ret_count_) const {
        if (obs_mean) std::memcpy(obs_mean, st.data(), (size_t)D * 4); if (obs_var) std::memcpy(obs_var, st.data() + D, (size_t)D * 4);
        if (ret_mean) *ret_mean = st[2 * D]; if (ret_var) *ret_var = st[2 * D + 1];
        if (obs_count_) *obs_count_ = obs_count; if (ret_count_) *ret_count_ = ret_count;
    }
    std::vector<float> pack(const float* obs_mean, const float* obs_var, float ret_mean, float ret_var) const {
        std::vector<float> st(stats_floats());
        std::memcpy(st.data(), obs_mean, (size_t)D * 4); std::memcpy(st.data() + D, obs_var, (size_t)D * 4); st[2 * D] = ret_mean; st[2 * D + 1] = ret_var;
        return st;
    }
    // an apply launch over this wrapper's own table (n: the envs behind its sums); one that updates writes the other half ...
    void fill(NormWrapArgs& a, bool upd_obs, bool upd_ret, long long n) const {
        const bool upd = upd_obs || upd_ret;
        a.D = D; a.n = n; a.partials = upd ? partials : nullptr; a.upd_obs = upd_obs; a.upd_ret = upd_ret; a.norm_obs = cfg.norm_obs; a.norm_reward = cfg.norm_reward;
        a.obs_count = obs_count; a.ret_count = ret_count; a.clip_obs = cfg.clip_obs; a.clip_reward = cfg.clip_reward; a.eps = cfg.epsilon;
        a.st_in = half(cur); a.st_out = upd ? half(cur ^ 1) : nullptr;
    }
    // ... which is the one in force once the launch is enqueued
    void commit(const NormWrapArgs& a) {
        if (!a.upd_obs && !a.upd_ret) return;
        cur ^= 1; if (a.upd_obs) obs_count += a.n; if (a.upd_ret) ret_count += a.n;
    }
};

}  // namespace
