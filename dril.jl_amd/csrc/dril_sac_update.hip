// dril_sac_update.hip — one gradient step of the SAC handle (update!, sac.jl:299-404): its kernels — the gather, the loss heads in their fused and unfused
// forms, the reverse of the squashed sample, the two optimiser kernels — sac_one_update, which enqueues them around the contractions of dril_sac_net.hip, the
// statistics rows, and the verbs dril_sac_debug_set_batches, dril_sac_update, dril_sac_update_info and dril_sac_get_last_grads.  The units: dril_sac_handle.h.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "dril_sac_handle.h"

using namespace dril;
using namespace dril::sac;

namespace {

// deterministic block reduction (blockDim.x == 256): pairwise tree in shared memory
__device__ inline double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v; __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (t < s) sh[t] += sh[t + s]; __syncthreads(); }
    const double r = sh[0]; __syncthreads();
    return r;
}

// ---- get_data_loader (replay_buffer.jl:116-157): gather one batch + its three noise draws -------------------------------
struct GatherArgs {
    int B, D, A; long long cap, head, size;
    const float *rb_obs, *rb_next, *rb_act, *rb_rew; const uint8_t* rb_term;
    const long long* inj_idx; const float *inj_ne, *inj_nn, *inj_np;     // injected batch (tests), per sample; null = Philox
    SacRng rng;
    float* xa;        // [2B][D]: rows [0,B) observations, [B,2B) next observations (actor input)
    float* xq;        // [B][D+A]: (obs, stored action)
    float *rew, *ne, *nn, *np; uint8_t* term;
};
__global__ void sac_gather_kernel(GatherArgs g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.B) return;
    long long j;
    if (g.inj_idx) j = g.inj_idx[i];
    else {
        uint32_t o[4];
        philox4x32_10((uint32_t)g.rng.key, (uint32_t)(g.rng.key >> 32), (uint32_t)g.rng.u, (uint32_t)(g.rng.u >> 32), 4u, (uint32_t)i, o);
        j = (long long)(u01_f64(o[0], o[1]) * (double)g.size); if (j >= g.size) j = g.size - 1;
    }
    const long long slot = (g.head + j) % g.cap;
    for (int d = 0; d < g.D; ++d) {
        const float o = g.rb_obs[slot * g.D + d];
        g.xa[(size_t)i * g.D + d] = o; g.xq[(size_t)i * (g.D + g.A) + d] = o;
        g.xa[(size_t)(g.B + i) * g.D + d] = g.rb_next[slot * g.D + d];
    }
    for (int a = 0; a < g.A; ++a) {
        g.xq[(size_t)i * (g.D + g.A) + g.D + a] = g.rb_act[slot * g.A + a];
        g.ne[i * g.A + a] = g.inj_ne ? g.inj_ne[i * g.A + a] : sac_noise(g.rng, 5, i, a);
        g.nn[i * g.A + a] = g.inj_nn ? g.inj_nn[i * g.A + a] : sac_noise(g.rng, 6, i, a);
        g.np[i * g.A + a] = g.inj_np ? g.inj_np[i * g.A + a] : sac_noise(g.rng, 7, i, a);
    }
    g.rew[i] = g.rb_rew[slot]; g.term[i] = g.rb_term[slot];
}

// one sample's first layer h1[u] = act(W1[u, :] . x + b1[u]) for all H1 units by the 256 threads of a block; W1 (H1 x in) column-major; x in shared memory
constexpr int kFusedL1MaxIn = 16;    // the per-sample form re-reads W1 per block: only for small inputs (Pendulum: 3 / 4); wider nets keep the contraction
__device__ __forceinline__ void first_layer_row(const float* __restrict__ W1, const float* __restrict__ b1, const float* x, int in, int H1, int relu, float* __restrict__ h1) {
    for (int u = threadIdx.x; u < H1; u += blockDim.x) {
        float acc = b1[u];
        for (int k = 0; k < in; ++k) acc = fmaf(W1[u + (size_t)k * H1], x[k], acc);
        h1[u] = relu ? relu_nan(acc) : tanhf(acc);
    }
}
// the same with the weights requested EARLY (before the barrier behind which the sample's inputs appear: one round of memory latency less in kernels that are
// nothing but dependent round trips): in <= 4 features, H1 <= 512 (two units per thread of a 256-thread block); same fma order
constexpr int kL1PreMaxIn = 4, kL1PreMaxH = 512;
struct L1Pre { float w[2][kL1PreMaxIn]; float b[2]; };
__device__ __forceinline__ bool first_layer_pre_ok(int in, int H1) { return in <= kL1PreMaxIn && H1 <= kL1PreMaxH; }
__device__ __forceinline__ void first_layer_pre(L1Pre& r, const float* __restrict__ W1, const float* __restrict__ b1, int in, int H1) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int u = threadIdx.x + 256 * t; const bool ok = u < H1;
#pragma unroll
        for (int k = 0; k < kL1PreMaxIn; ++k) r.w[t][k] = (ok && k < in) ? W1[u + (size_t)k * H1] : 0.f;
        r.b[t] = ok ? b1[u] : 0.f;
    }
}
__device__ __forceinline__ void first_layer_post(const L1Pre& r, const float* x, int in, int H1, int relu, float* __restrict__ h1) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int u = threadIdx.x + 256 * t;
        if (u < H1) {
            float acc = r.b[t];
#pragma unroll
            for (int k = 0; k < kL1PreMaxIn; ++k) if (k < in) acc = fmaf(r.w[t][k], x[k], acc);
            h1[u] = relu ? relu_nan(acc) : tanhf(acc);
        }
    }
}
// get_data_loader + the first layer of the actor on (obs | next obs) and of the two critics on (obs, stored action): sac_gather_kernel + the first launch of two
// net_forward calls.  One block per sample.
struct GatherL1Args {
    GatherArgs g; int H1, relu;
    const float *aW1, *ab1; float* ah1;                       // actor: W1 (H1 x D), b1; h1 [2B][H1]
    const float* P; int qw1, qb1; long long zP; long long zh; float* qh1;   // critic z: W1 at P + qw1 + z * zP; h1 [Z][nq][H1] with batch stride zh
};
__global__ __launch_bounds__(256) void sac_gather_l1_kernel(GatherL1Args f) {
    __shared__ float xs[2][kFusedL1MaxIn], xqs[kFusedL1MaxIn];
    const GatherArgs& g = f.g;
    const int i = blockIdx.x, W = g.D + g.A;
    const bool pre = first_layer_pre_ok(W, f.H1);                                    // weights of the three first layers requested before the sample is known
    L1Pre pa, pq[2];
    if (pre) { first_layer_pre(pa, f.aW1, f.ab1, g.D, f.H1); for (int z = 0; z < 2; ++z) first_layer_pre(pq[z], f.P + f.qw1 + z * f.zP, f.P + f.qb1 + z * f.zP, W, f.H1); }
    if (threadIdx.x == 0) {
        long long j;
        if (g.inj_idx) j = g.inj_idx[i];
        else {
            uint32_t o[4];
            philox4x32_10((uint32_t)g.rng.key, (uint32_t)(g.rng.key >> 32), (uint32_t)g.rng.u, (uint32_t)(g.rng.u >> 32), 4u, (uint32_t)i, o);
            j = (long long)(u01_f64(o[0], o[1]) * (double)g.size); if (j >= g.size) j = g.size - 1;
        }
        const long long slot = (g.head + j) % g.cap;
        for (int d = 0; d < g.D; ++d) {
            const float o = g.rb_obs[slot * g.D + d], n = g.rb_next[slot * g.D + d];
            g.xa[(size_t)i * g.D + d] = o; g.xq[(size_t)i * W + d] = o; g.xa[(size_t)(g.B + i) * g.D + d] = n;
            xs[0][d] = o; xs[1][d] = n; xqs[d] = o;
        }
        for (int a = 0; a < g.A; ++a) { const float act = g.rb_act[slot * g.A + a]; g.xq[(size_t)i * W + g.D + a] = act; xqs[g.D + a] = act; }
        g.rew[i] = g.rb_rew[slot]; g.term[i] = g.rb_term[slot];
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + 3 * g.A) {                    // the three noise arrays of the step on their own threads (a Philox block + a normal transform each), in another wave
        const int q = threadIdx.x - 64, which = q / g.A, a = q - which * g.A;
        const float* inj = which == 0 ? g.inj_ne : which == 1 ? g.inj_nn : g.inj_np;
        float* dst = which == 0 ? g.ne : which == 1 ? g.nn : g.np;
        dst[i * g.A + a] = inj ? inj[i * g.A + a] : sac_noise(g.rng, 5 + which, i, a);
    }
    __syncthreads();
    if (pre) {
        first_layer_post(pa, xs[0], g.D, f.H1, f.relu, f.ah1 + (size_t)i * f.H1);
        first_layer_post(pa, xs[1], g.D, f.H1, f.relu, f.ah1 + (size_t)(g.B + i) * f.H1);
#pragma unroll
        for (int z = 0; z < 2; ++z) first_layer_post(pq[z], xqs, W, f.H1, f.relu, f.qh1 + z * f.zh + (size_t)i * f.H1);
        return;
    }
    first_layer_row(f.aW1, f.ab1, xs[0], g.D, f.H1, f.relu, f.ah1 + (size_t)i * f.H1);
    first_layer_row(f.aW1, f.ab1, xs[1], g.D, f.H1, f.relu, f.ah1 + (size_t)(g.B + i) * f.H1);
#pragma unroll
    for (int z = 0; z < 2; ++z) first_layer_row(f.P + f.qw1 + z * f.zP, f.P + f.qb1 + z * f.zP, xqs, W, f.H1, f.relu, f.qh1 + z * f.zh + (size_t)i * f.H1);
}

// ---- entropy-coefficient step (sac.jl:313-343) + next actions for the critic target (:131) ----------------------------------
struct EntNextArgs {
    int B, D, A; const float* mu;    // [2B][A] actor means of (obs | next obs)
    const float* log_std; const float *ne, *nn; const float* xa;
    float* xq_next;   // [B][D+A] (next obs, next action)
    float* nlp;       // [B] next log-probs
    const float* np; float *xq_pi, *a_pi, *g_pi, *lp_pi;   // the actor-loss sample (sac_actor_loss :101): it only depends on the actor, which does not change before the actor step
    SacScalars* sc; float target_entropy, lr, b1, b2, eps, bt1, bt2; int auto_ent;
    float* stats;     // [8]: 0 actor_loss 1 critic_loss 2 entropy_loss 3 mean_q 4 ent_coef 5 |gc|^2 6 |ga|^2
};
__global__ __launch_bounds__(256) void sac_ent_next_kernel(EntNextArgs g) {
    __shared__ double sh[256];
    float ls[kMaxA]; for (int a = 0; a < g.A; ++a) ls[a] = g.log_std[a];
    double s = 0;
    for (int i = threadIdx.x; i < g.B; i += 256) {
        float a_[kMaxA], gg[kMaxA];
        if (g.auto_ent) s += (double)(squashed_sample_logp(g.mu + (size_t)i * g.A, ls, g.ne + (size_t)i * g.A, g.A, a_, gg) + g.target_entropy);
        g.nlp[i] = squashed_sample_logp(g.mu + (size_t)(g.B + i) * g.A, ls, g.nn + (size_t)i * g.A, g.A, a_, gg);
        for (int d = 0; d < g.D; ++d) g.xq_next[(size_t)i * (g.D + g.A) + d] = g.xa[(size_t)(g.B + i) * g.D + d];
        for (int a = 0; a < g.A; ++a) g.xq_next[(size_t)i * (g.D + g.A) + g.D + a] = a_[a];
        g.lp_pi[i] = squashed_sample_logp(g.mu + (size_t)i * g.A, ls, g.np + (size_t)i * g.A, g.A, a_, gg);
        for (int d = 0; d < g.D; ++d) g.xq_pi[(size_t)i * (g.D + g.A) + d] = g.xa[(size_t)i * g.D + d];
        for (int a = 0; a < g.A; ++a) { g.xq_pi[(size_t)i * (g.D + g.A) + g.D + a] = a_[a]; g.a_pi[i * g.A + a] = a_[a]; g.g_pi[i * g.A + a] = gg[a]; }
    }
    const double tot = block_sum(s, sh);
    if (threadIdx.x == 0) {
        float le = g.sc->log_ent;
        if (g.auto_ent) {
            const float cc = (float)(tot / g.B);
            g.stats[2] = -(le * cc);                                                          // loss = -(log_ent_coef * c), :330
            const float gr = -cc;
            const float m = g.b1 * g.sc->ent_m + (1.0f - g.b1) * gr, v = g.b2 * g.sc->ent_v + (1.0f - g.b2) * gr * gr;
            g.sc->ent_m = m; g.sc->ent_v = v;
            le -= m / (1.0f - g.bt1) / (sqrtf(v / (1.0f - g.bt2)) + g.eps) * g.lr;           // Optimisers.Adam
            g.sc->log_ent = le;
        }
        g.sc->alpha = expf(le);
        g.stats[4] = g.sc->alpha;                                                             // :391
    }
}

// ---- Bellman target + critic loss head (sac_critic_loss :136-150) ---------------------------------------------------------
struct CriticHeadArgs {
    int B; const float* q_next;  // [2][B] target-network values of (next obs, next action)
    const float* q;              // [2][B] current values of (obs, action)
    const float *rew, *nlp; const uint8_t* term; const SacScalars* sc; float gamma;
    float* dq;                   // [2][B] dL/dq
    float* stats;
};
__global__ __launch_bounds__(256) void sac_critic_head_kernel(CriticHeadArgs g) {
    __shared__ double sh[256];
    const float alpha = g.sc->alpha;
    double cl = 0, qs = 0;
    for (int i = threadIdx.x; i < g.B; i += 256) {
        const float n0 = g.q_next[i], n1 = g.q_next[g.B + i], mn = n0 < n1 ? n0 : n1;
        const float y = g.term[i] ? g.rew[i] : g.rew[i] + g.gamma * (mn - alpha * g.nlp[i]);
        for (int k = 0; k < 2; ++k) {
            const float qv = g.q[k * g.B + i], d = qv - y;
            cl += 0.5 * (double)d * d / g.B; qs += qv;
            g.dq[k * g.B + i] = d / (float)g.B;
        }
    }
    cl = block_sum(cl, sh); qs = block_sum(qs, sh);
    if (threadIdx.x == 0) { g.stats[1] = (float)cl; g.stats[3] = (float)(qs / (2.0 * g.B)); }
}

// actor loss head (:102-104): min over the critics, dL/dq
struct ActorHeadArgs { int B; const float* q_pi; const float* lp_pi; const SacScalars* sc; float* dq; float* stats; };
__global__ __launch_bounds__(256) void sac_actor_head_kernel(ActorHeadArgs g) {
    __shared__ double sh[256];
    const float alpha = g.sc->alpha;
    double al = 0;
    for (int i = threadIdx.x; i < g.B; i += 256) {
        const float q0 = g.q_pi[i], q1 = g.q_pi[g.B + i];
        const int km = q1 < q0 ? 1 : 0;
        al += ((double)alpha * g.lp_pi[i] - (km ? q1 : q0)) / g.B;
        g.dq[km * g.B + i] = -1.0f / (float)g.B; g.dq[(1 - km) * g.B + i] = 0.f;
    }
    al = block_sum(al, sh);
    if (threadIdx.x == 0) g.stats[0] = (float)al;
}
// reverse of the squashed sample (Zygote through tanh -> clamp -> atanh -> logpdf): dL/dmu per sample, dL/dlog_std summed
struct SquashBwdArgs {
    int B, D, A; const float* mu; const float* log_std; const float* np; const float *a_pi, *g_pi;
    const float* dxq;   // [2][B][D+A] input gradients of the two critics
    const SacScalars* sc; float* dmu; float* g_log_std;
};
__global__ __launch_bounds__(256) void sac_squash_bwd_kernel(SquashBwdArgs g) {
    __shared__ double sh[256];
    const float alpha = g.sc->alpha, eps = 1.0e-6f, lo = -1.0f + eps, hi = 1.0f - eps;
    double dls[kMaxA]; for (int a = 0; a < g.A; ++a) dls[a] = 0;
    const int W = g.D + g.A;
    for (int i = threadIdx.x; i < g.B; i += 256) {
        const float dlogp = alpha / (float)g.B;
        for (int a = 0; a < g.A; ++a) {
            const float da = g.dxq[(size_t)i * W + g.D + a] + g.dxq[((size_t)g.B + i) * W + g.D + a];
            const float ls = g.log_std[a], sig = expf(ls), e2 = expf(-2.0f * ls);
            const float x = g.a_pi[i * g.A + a], gg = g.g_pi[i * g.A + a], mu = g.mu[(size_t)i * g.A + a], d = gg - mu;
            const float inside = (x >= lo && x <= hi) ? 1.0f : 0.0f;
            const float dlp_dg = -d * e2 + 2.0f * tanhf(gg);
            const float du = dlogp * dlp_dg * inside + da * (1.0f - x * x);
            g.dmu[(size_t)i * g.A + a] = dlogp * (d * e2) + du;
            dls[a] += (double)(dlogp * (-1.0f + d * d * e2) + du * sig * g.np[i * g.A + a]);
        }
    }
    for (int a = 0; a < g.A; ++a) { const double t = block_sum(dls[a], sh); if (threadIdx.x == 0) g.g_log_std[a] = (float)t; }
}

// =================================================================================================================
// Fused heads.  A net's OUTPUT layer has one (Q nets) or A (actor) rows: as a contraction it is one launch of ~4.5 us for a few hundred dot
// products, and so is the first stage of the reverse pass (K = 1).  The kernels below do the output-layer dot products, the per-sample loss head and
// the first reverse stage dz2 = (W3' dOut) .* act'(h2) in ONE launch, one wave per sample (lanes stride the hidden units, fixed-order butterfly sum =>
// deterministic), per-block partial sums of the batch statistics folded in index order by the block that finishes last.  25 -> 19 dependent
// launches per update!.  (kHeadSamplesPerBlock: dril_sac_device.h.)
// =================================================================================================================
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// dot of two contiguous, 16-byte-aligned rows of H floats (H % 4 == 0): every lane's float4 loads are issued before the first use
__device__ __forceinline__ float wave_dot(const float* __restrict__ w, const float* __restrict__ x, int H, int lane) {
    float s = 0.f;
    for (int u = lane; u < H / 4; u += 64) {
        const float4 a = reinterpret_cast<const float4*>(w)[u], b = reinterpret_cast<const float4*>(x)[u];
        s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
    }
    return wave_sum(s);
}
// dot of a strided weight row (element u at w[u * stride]) with a contiguous activation row
__device__ __forceinline__ float wave_dot_strided(const float* __restrict__ w, int stride, const float* __restrict__ x, int H, int lane) {
    float s = 0.f;
    for (int u = lane; u < H; u += 64) s = fmaf(w[(size_t)u * stride], x[u], s);
    return wave_sum(s);
}
__device__ __forceinline__ float act_deriv(float hval, int relu) { return relu ? (hval > 0.f ? 1.0f : 0.0f) : 1.0f - hval * hval; }
// last-block fold of per-block values (double, index order): `mine` is this block's value (valid in thread 0); returns true in the block that finished
// last, with the totals in tot[0..NV) (all threads)
template <int NV>
__device__ __forceinline__ bool fold_partials(const double (&mine)[NV], double* partials, unsigned int* counter, double (&tot)[NV], double* sh) {
    __shared__ bool last;
    const int t = threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) partials[(size_t)blockIdx.x * NV + k] = mine[k];
        __threadfence(); last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
#pragma unroll
    for (int k = 0; k < NV; ++k) {                                             // all 256 threads fetch (one round trip), fixed-order tree: deterministic
        double a = 0;
        for (unsigned b = t; b < gridDim.x; b += 256) a += ((volatile const double*)partials)[(size_t)b * NV + k];
        tot[k] = block_sum(a, sh);
    }
    if (t == 0) *counter = 0u;
    return true;
}

// actor output layer on (obs | next obs) + entropy-coefficient step + next actions + the actor-loss sample: net_forward's third launch + sac_ent_next_kernel
struct ActorHeadFusedArgs {
    EntNextArgs e; const float* ah2; int H2; const float* W3; const float* b3;   // W3 (A x H2) column-major: row a strided by A
    float* mu_out; double* partials; unsigned int* counter;
    // first layer of the two TARGET critics on (next obs, next action), when the input is narrow (first_l1 != 0): z = 2, 3 of the four-net forward
    int first_l1, H1, relu; const float* P; int qw1, qb1; long long zP, zh; float* qh1;
};
// PRE (narrow spaces: D + A <= 4, H1 <= 512 when first_l1): everything the later phases read from memory and that does not depend on this kernel's results is
// requested at the top — the noise of the three samples and the two observation rows (lane 0 of waves 0 - 2), the first-layer weights of the two target critics
// (all threads) — and the (next obs, next action) row reaches the first layers through LDS: the kernel was four dependent round trips long, now two.
template <bool PRE>
__global__ __launch_bounds__(256) void sac_actor_out_ent_kernel(ActorHeadFusedArgs f) {
    __shared__ double sh[256];
    __shared__ float mus[2][kMaxA];
    __shared__ double ssum;
    __shared__ float xn[kFusedL1MaxIn];
    const EntNextArgs& g = f.e;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x;
    float ls[kMaxA]; for (int a = 0; a < g.A; ++a) ls[a] = g.log_std[a];
    L1Pre pq[2];
    float nz[kL1PreMaxIn], xrow[kL1PreMaxIn];
    if constexpr (PRE) {
        if (f.first_l1) for (int z = 0; z < 2; ++z) first_layer_pre(pq[z], f.P + f.qw1 + (z + 2) * f.zP, f.P + f.qb1 + (z + 2) * f.zP, g.D + g.A, f.H1);
        if (lane == 0 && wave < 3) {
            const float* src = wave == 0 ? g.ne : wave == 1 ? g.nn : g.np;
            const float* xr = g.xa + (size_t)((wave == 1 ? g.B : 0) + i) * g.D;
#pragma unroll
            for (int a = 0; a < kL1PreMaxIn; ++a) { nz[a] = a < g.A ? src[(size_t)i * g.A + a] : 0.f; xrow[a] = a < g.D ? xr[a] : 0.f; }
        }
    }
    // phase 1: mu = W3 h2 + b3 for row i (obs) and row B + i (next obs): (row, a) pairs over the four waves
    for (int p = wave; p < 2 * g.A; p += 4) {
        const int row = p / g.A, a = p - row * g.A;
        const float d = wave_dot_strided(f.W3 + a, g.A, f.ah2 + (size_t)(row * g.B + i) * f.H2, f.H2, lane) + f.b3[a];
        if (lane == 0) { mus[row][a] = d; f.mu_out[(size_t)(row * g.B + i) * g.A + a] = d; }
    }
    if (threadIdx.x == 0) ssum = 0.0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 192) {                          // phase 2: the three squashed samples of the row on lane 0 of three WAVES (libm-heavy scalar math: on three
        const int which = threadIdx.x >> 6;                                       // lanes of one wave the divergent branches ran one after the other — 3 x ~1.5 us of an 11 us kernel)
        float a_[kMaxA], gg[kMaxA];
        const float* noise = which == 0 ? g.ne + (size_t)i * g.A : which == 1 ? g.nn + (size_t)i * g.A : g.np + (size_t)i * g.A;
        const float* xr = g.xa + (size_t)((which == 1 ? g.B : 0) + i) * g.D;
        float lp;
        if constexpr (PRE) lp = squashed_sample_logp(mus[which == 1 ? 1 : 0], ls, nz, g.A, a_, gg);
        else lp = (which || g.auto_ent) ? squashed_sample_logp(mus[which == 1 ? 1 : 0], ls, noise, g.A, a_, gg) : 0.f;
        auto xv = [&](int d) { if constexpr (PRE) { float v = xrow[0]; for (int t = 1; t < kL1PreMaxIn; ++t) v = d == t ? xrow[t] : v; return v; } else return xr[d]; };
        if (which == 0) { if (g.auto_ent) ssum = (double)(lp + g.target_entropy); }
        else if (which == 1) {
            g.nlp[i] = lp;
            const bool to_lds = f.first_l1 != 0;                                 // (first_l1 implies D + A <= kFusedL1MaxIn)
            for (int d = 0; d < g.D; ++d) { const float v = xv(d); g.xq_next[(size_t)i * (g.D + g.A) + d] = v; if (to_lds) xn[d] = v; }
            for (int a = 0; a < g.A; ++a) { g.xq_next[(size_t)i * (g.D + g.A) + g.D + a] = a_[a]; if (to_lds) xn[g.D + a] = a_[a]; }
        } else {
            g.lp_pi[i] = lp;
            for (int d = 0; d < g.D; ++d) g.xq_pi[(size_t)i * (g.D + g.A) + d] = xv(d);
            for (int a = 0; a < g.A; ++a) { g.xq_pi[(size_t)i * (g.D + g.A) + g.D + a] = a_[a]; g.a_pi[i * g.A + a] = a_[a]; g.g_pi[i * g.A + a] = gg[a]; }
        }
    }
    __syncthreads();
    if (f.first_l1) {                                                             // lane 0 of wave 1 left this sample's (next obs, next action) row in xn
#pragma unroll
        for (int z = 2; z < 4; ++z) {
            if constexpr (PRE) first_layer_post(pq[z - 2], xn, g.D + g.A, f.H1, f.relu, f.qh1 + z * f.zh + (size_t)i * f.H1);
            else first_layer_row(f.P + f.qw1 + z * f.zP, f.P + f.qb1 + z * f.zP, xn, g.D + g.A, f.H1, f.relu, f.qh1 + z * f.zh + (size_t)i * f.H1);
        }
    }
    // the entropy-coefficient step itself (mean over the batch, scalar Adam) runs at the head of the next kernel that needs alpha (sac_q_out_head_kernel, mode 0):
    // every one of its blocks sums these B per-sample terms in the same order — cheaper than a grid-wide fold here (an atomic ticket, a fence and a second phase: ~7 us)
    if (threadIdx.x == 0) f.partials[i] = ssum;
}

// Q output layers (Z nets: the two critics, and with Z = 4 the two targets behind them) + loss head + dz2 of the two critics
struct QHeadFusedArgs {
    int B, H2, nq, relu, Z; long long zP, zh2;     // net z: W3 / b3 at P + w3 + z * zP, h2 at qh2 + z * zh2
    const float* P; int w3, b3; const float* qh2;
    float* q_out;          // [Z][nq]
    float* dz2;            // [2][nq][H2]
    // critic head (mode 0) / actor head (mode 1)
    int mode; const float *rew, *nlp, *lp_pi; const uint8_t* term; const SacScalars* sc; float gamma;
    float* dq; float* stats; double* partials; unsigned int* counter;
    // mode 0 also takes the entropy-coefficient step (sac.jl:313-343): `sc` is the state before it, `sc_next` receives the state after it (block 0), every block uses it in registers;
    // mode 1 and the later kernels are handed sc_next as their `sc`
    const double* ent_terms; SacScalars* sc_next; int auto_ent; float ent_lr, ent_b1, ent_b2, ent_eps, ent_bt1, ent_bt2;
};
__global__ __launch_bounds__(256) void sac_q_out_head_kernel(QHeadFusedArgs g) {
    __shared__ double sh[256];
    __shared__ float qs[4], dqs[2];
    __shared__ double part[2];
    __shared__ float alpha_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x;
    if (g.mode == 0) {
        double t = 0;
        if (g.auto_ent) { for (int k = threadIdx.x; k < g.B; k += 256) t += g.ent_terms[k]; t = block_sum(t, sh); }   // fixed order: the same bits in every block
        if (threadIdx.x == 0) {
            float le = g.sc->log_ent, m = g.sc->ent_m, v = g.sc->ent_v, loss = 0.f;
            if (g.auto_ent) {
                const float cc = (float)(t / g.B);
                loss = -(le * cc);                                                                // loss = -(log_ent_coef * c), sac.jl:330
                const float gr = -cc;
                m = g.ent_b1 * m + (1.0f - g.ent_b1) * gr; v = g.ent_b2 * v + (1.0f - g.ent_b2) * gr * gr;
                le -= m / (1.0f - g.ent_bt1) / (sqrtf(v / (1.0f - g.ent_bt2)) + g.ent_eps) * g.ent_lr;   // Optimisers.Adam
            }
            alpha_s = expf(le);
            if (blockIdx.x == 0) { g.sc_next->log_ent = le; g.sc_next->ent_m = m; g.sc_next->ent_v = v; g.sc_next->alpha = alpha_s; if (g.auto_ent) g.stats[2] = loss; g.stats[4] = alpha_s; }   // :391
        }
    } else if (threadIdx.x == 0) alpha_s = g.sc->alpha;
    if (wave < g.Z) {                                                          // one wave per net: q_z = W3_z . h2_z + b3_z
        const float q = wave_dot(g.P + g.w3 + wave * g.zP, g.qh2 + wave * g.zh2 + (size_t)i * g.H2, g.H2, lane) + g.P[g.b3 + wave * g.zP];
        if (lane == 0) { qs[wave] = q; g.q_out[(size_t)wave * g.nq + i] = q; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float alpha = alpha_s;
        float dq0, dq1; double s0 = 0, s1 = 0;
        if (g.mode == 0) {                                                    // Bellman target + critic loss (sac_critic_loss :136-150)
            const float mn = qs[2] < qs[3] ? qs[2] : qs[3];
            const float y = g.term[i] ? g.rew[i] : g.rew[i] + g.gamma * (mn - alpha * g.nlp[i]);
            const float d0 = qs[0] - y, d1 = qs[1] - y;
            dq0 = d0 / (float)g.B; dq1 = d1 / (float)g.B;
            s0 = 0.5 * (double)d0 * d0 / g.B + 0.5 * (double)d1 * d1 / g.B; s1 = (double)qs[0] + (double)qs[1];
        } else {                                                              // actor loss (:102-104): min over the critics
            const int km = qs[1] < qs[0] ? 1 : 0;
            dq0 = km == 0 ? -1.0f / (float)g.B : 0.f; dq1 = km == 1 ? -1.0f / (float)g.B : 0.f;
            s0 = ((double)alpha * g.lp_pi[i] - (km ? qs[1] : qs[0])) / g.B;
        }
        dqs[0] = dq0; dqs[1] = dq1; g.dq[i] = dq0; g.dq[g.nq + i] = dq1; part[0] = s0; part[1] = s1;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < 2 * g.H2; u += 256) {                        // dz2 = (W3' dq) .* act'(h2): the first stage of the reverse pass (K = 1)
        const int k = u >= g.H2, j = u - k * g.H2;
        g.dz2[((size_t)k * g.nq + i) * g.H2 + j] = g.P[g.w3 + k * g.zP + j] * dqs[k] * act_deriv(g.qh2[k * g.zh2 + (size_t)i * g.H2 + j], g.relu);
    }
    // the sums feed statistics only: per-block values, folded by sac_step_end_kernel (no atomics, no second phase here)
    if (threadIdx.x == 0) { g.partials[(size_t)blockIdx.x * 2] = part[0]; g.partials[(size_t)blockIdx.x * 2 + 1] = part[1]; }
}

// action columns of dx = W1' dz1 of both critics + reverse of the squashed sample + dz2 of the ACTOR: net_backward's last launch (dX), sac_squash_bwd_kernel
// and the first stage of the actor's reverse pass
struct SquashFusedArgs {
    SquashBwdArgs s; int H1, H2, relu, nq; const float* P; int qw1; long long zP;   // critic k: W1 (H1 x (D+A)) column-major at P + qw1 + k * zP
    const float* dz1;      // [2][nq][H1]
    const float* aW3; const float* ah2; float* adz2;   // actor: W3 (A x H2), h2 [.][H2], dz2 out [nq][H2]
    double* partials; unsigned int* counter;
};
__global__ __launch_bounds__(256) void sac_dx_squash_kernel(SquashFusedArgs f) {
    __shared__ double sh[256];
    __shared__ float das[2][kMaxA], dmus[kMaxA];
    __shared__ double dlss[kMaxA];
    const SquashBwdArgs& g = f.s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = blockIdx.x;
    const float alpha = g.sc->alpha, eps = 1.0e-6f, lo = -1.0f + eps, hi = 1.0f - eps;
    for (int p = wave; p < 2 * g.A; p += 4) {                                  // d Q_k / d action_a = W1_k[:, D + a] . dz1_k: (critic, a) pairs over the four waves
        const int kk = p / g.A, a = p - kk * g.A;
        const float d = wave_dot(f.P + f.qw1 + kk * f.zP + (size_t)(g.D + a) * f.H1, f.dz1 + ((size_t)kk * f.nq + i) * f.H1, f.H1, lane);
        if (lane == 0) das[kk][a] = d;
    }
    __syncthreads();
    if (threadIdx.x < g.A) {
        const int a = threadIdx.x;
        const float dlogp = alpha / (float)g.B, da = das[0][a] + das[1][a];
        const float ls = g.log_std[a], sig = expf(ls), e2 = expf(-2.0f * ls);
        const float x = g.a_pi[i * g.A + a], gg = g.g_pi[i * g.A + a], mu = g.mu[(size_t)i * g.A + a], d = gg - mu;
        const float inside = (x >= lo && x <= hi) ? 1.0f : 0.0f;
        const float dlp_dg = -d * e2 + 2.0f * tanhf(gg);
        const float du = dlogp * dlp_dg * inside + da * (1.0f - x * x);
        const float dm = dlogp * (d * e2) + du;
        dmus[a] = dm; g.dmu[(size_t)i * g.A + a] = dm;
        dlss[a] = (double)(dlogp * (-1.0f + d * d * e2) + du * sig * g.np[i * g.A + a]);
    }
    __syncthreads();
    for (int u = threadIdx.x; u < f.H2; u += 256) {                            // actor dz2 = (W3' dmu) .* act'(h2)
        float t = 0.f;
        for (int a = 0; a < g.A; ++a) t = fmaf(f.aW3[a + (size_t)u * g.A], dmus[a], t);
        f.adz2[(size_t)i * f.H2 + u] = t * act_deriv(f.ah2[(size_t)i * f.H2 + u], f.relu);
    }
    if (threadIdx.x < g.A) f.partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = dlss[threadIdx.x];   // log_std gradient: per-sample terms, summed by sac_step_end_kernel right before its Adam step
}

// ---- Optimisers.Adam on a parameter range; grads == nullptr applies ZERO gradients (zero_critic_grads! then apply_gradients,
// sac.jl:381-382: the moments decay and the parameters keep moving along the remaining momentum) ---------------------------
__device__ __forceinline__ float adam_one(float* p, float* m, float* v, int i, float gi, float lr, float b1, float b2, float eps, float bt1, float bt2) {
    const float mm = b1 * m[i] + (1.0f - b1) * gi, vv = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mm; v[i] = vv;
    const float np_ = p[i] - mm / (1.0f - bt1) / (sqrtf(vv / (1.0f - bt2)) + eps) * lr;
    p[i] = np_; return np_;
}
__device__ __forceinline__ float4 adam_vec(float* p, float* m, float* v, int i, float4 g, float lr, float b1, float b2, float eps, float bt1, float bt2) {
    float4 pp = *reinterpret_cast<float4*>(p + i), mm = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
    float* P = reinterpret_cast<float*>(&pp); float* M = reinterpret_cast<float*>(&mm); float* V = reinterpret_cast<float*>(&vv); const float* G = reinterpret_cast<const float*>(&g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        M[t] = b1 * M[t] + (1.0f - b1) * G[t]; V[t] = b2 * V[t] + (1.0f - b2) * G[t] * G[t];
        P[t] -= M[t] / (1.0f - bt1) / (sqrtf(V[t] / (1.0f - bt2)) + eps) * lr;
    }
    *reinterpret_cast<float4*>(p + i) = pp; *reinterpret_cast<float4*>(m + i) = mm; *reinterpret_cast<float4*>(v + i) = vv;
    return pp;
}
// ---- the first layer's parameter gradients INSIDE the optimiser kernels ------------------------------------------------------
// [dW1 | db1] = dz1 . [x' | 1] of a narrow input (Pendulum: 3 / 4 features) is a (H1 x 5) x B contraction: 0.7 MFLOP in a launch of its own (7 us: the floor
// of a dependent launch), followed by the optimiser kernel that consumes it — and, on the critic side, by another small launch that re-evaluates the first layer
// with the stepped parameters for the actor loss.  Here extra blocks at the END of the optimiser kernel's grid own the first layer: a block takes kOptL1Units hidden
// units of one net; thread = (unit, one of 16 sample groups): per-thread sums over its samples (all loads in flight), the 16 groups folded through LDS in
// index order (deterministic), 5 x 16 threads then write the gradient (dril_sac_get_last_grads), take the Adam step and — x2 given — all threads evaluate the
// layer on x2 with the stepped parameters in the order of first_layer_row.  The elementwise loop of the kernel skips these parameters.
// (kOptL1MaxIn, kOptL1Units, kOptL1Groups, kOptL1MaxB: dril_sac_device.h.)
struct FirstLayerOpt {
    int nblocks;                      // 0: off.  Z * ceil(H1 / kOptL1Units) blocks behind the elementwise ones
    int Z, in, H1, B, relu;
    int w1, b1; long long zP;         // W1 (H1 x in, column-major) / b1 of net z at index w1 / b1 + z zP of the kernel's parameter, moment and gradient arrays
    const float* dz1; long long zdz;  // [Z][B][H1]
    const float* x; int ldx;          // [B][ldx] rows (the same input for every z)
    const float* x2; float* h1; long long zh;   // x2 != null: h1[z][b][:] = act(W1 x2[b] + b1) with the stepped parameters; x2 [B][in]
};
__device__ __forceinline__ double first_layer_opt_block(const FirstLayerOpt& f, int blk, float* p, float* m, float* v, float* g,
                                                        float lr, float b1c, float b2c, float eps, float bt1, float bt2) {
    // ONE round of memory latency: the block's dz1 values (16 per thread at B = 256), both input matrices (into LDS) and the parameters / moments it will step are
    // all requested before anything waits
    extern __shared__ __attribute__((aligned(16))) float fl_x[];      // [B][4] x, then [B][4] x2 (launch: first_layer_opt_lds bytes)
    __shared__ float part[kOptL1Groups][kOptL1MaxIn + 1][kOptL1Units];
    __shared__ float wnew[kOptL1MaxIn + 1][kOptL1Units];
    const int nbu = (f.H1 + kOptL1Units - 1) / kOptL1Units, z = blk / nbu, u = threadIdx.x & (kOptL1Units - 1), grp = threadIdx.x / kOptL1Units;
    const int unit = (blk - z * nbu) * kOptL1Units + u;
    const bool live = unit < f.H1;
    const float* __restrict__ dz = f.dz1 + (size_t)z * f.zdz + (live ? unit : 0);
    float4* xs = reinterpret_cast<float4*>(fl_x); float4* x2s = xs + f.B;      // rows padded to four features (zeros): one ds_read_b128 per sample, no branches on `in`
    const int kk = threadIdx.x / kOptL1Units;                         // the parameter row this thread steps (threads < 5 x 16): k < in a column of W1, k == 4 the bias
    const bool steps = threadIdx.x < (kOptL1MaxIn + 1) * kOptL1Units && live && (kk < f.in || kk == kOptL1MaxIn);
    const int idx = (int)(z * f.zP) + (kk == kOptL1MaxIn ? f.b1 + unit : f.w1 + unit + kk * f.H1);
    float p0 = 0.f, m0 = 0.f, v0 = 0.f;
    if (steps) { p0 = p[idx]; m0 = m[idx]; v0 = v[idx]; }
    float acc[kOptL1MaxIn + 1];
#pragma unroll
    for (int k = 0; k <= kOptL1MaxIn; ++k) acc[k] = 0.f;
    for (int b0 = 0; b0 < f.B; b0 += kOptL1Groups * 16) {
        float d[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) { const int b = b0 + grp + kOptL1Groups * j; d[j] = dz[(size_t)(b < f.B ? b : f.B - 1) * f.H1]; }
        if (b0 == 0) {
            for (int i = threadIdx.x; i < f.B * kOptL1MaxIn; i += blockDim.x) {
                const int b = i / kOptL1MaxIn, k = i % kOptL1MaxIn;
                fl_x[i] = k < f.in ? f.x[(size_t)b * f.ldx + k] : 0.f;
                if (f.x2) fl_x[(size_t)f.B * kOptL1MaxIn + i] = k < f.in ? f.x2[(size_t)b * f.in + k] : 0.f;
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int b = b0 + grp + kOptL1Groups * j;
            const float dd = b < f.B ? d[j] : 0.f;                    // (rows past B re-read the last one and count as zero)
            const float4 xv = xs[b < f.B ? b : f.B - 1];
            acc[0] = fmaf(dd, xv.x, acc[0]); acc[1] = fmaf(dd, xv.y, acc[1]); acc[2] = fmaf(dd, xv.z, acc[2]); acc[3] = fmaf(dd, xv.w, acc[3]);
            acc[kOptL1MaxIn] += dd;
        }
    }
#pragma unroll
    for (int k = 0; k <= kOptL1MaxIn; ++k) part[grp][k][u] = acc[k];
    __syncthreads();
    double ss = 0;
    if (threadIdx.x < (kOptL1MaxIn + 1) * kOptL1Units) {
        float gs = 0.f, np_ = 0.f;
#pragma unroll
        for (int q = 0; q < kOptL1Groups; ++q) gs += part[q][kk][u];
        if (steps) {                                                   // adam_one on the values requested at the top
            if (g) g[idx] = gs;
            const float mm = b1c * m0 + (1.0f - b1c) * gs, vv = b2c * v0 + (1.0f - b2c) * gs * gs;
            m[idx] = mm; v[idx] = vv;
            np_ = p0 - mm / (1.0f - bt1) / (sqrtf(vv / (1.0f - bt2)) + eps) * lr;
            p[idx] = np_;
            ss = (double)gs * gs;
        }
        wnew[kk][u] = np_;                                             // (rows k >= in: zero weights against the zero padding of x2)
    }
    if (!f.x2) return ss;
    __syncthreads();
    const float w0 = wnew[0][u], w1 = wnew[1][u], w2 = wnew[2][u], w3 = wnew[3][u], bb = wnew[kOptL1MaxIn][u];
    float* __restrict__ out = f.h1 + (size_t)z * f.zh + unit;
#pragma unroll 4
    for (int b = grp; b < f.B; b += kOptL1Groups) {
        const float4 xv = x2s[b];
        float a = fmaf(w0, xv.x, bb); a = fmaf(w1, xv.y, a); a = fmaf(w2, xv.z, a); a = fmaf(w3, xv.w, a);      // the order of first_layer_row (+ exact zero terms)
        if (live) out[(size_t)b * f.H1] = f.relu ? relu_nan(a) : tanhf(a);
    }
    return ss;
}
inline size_t first_layer_opt_lds(const FirstLayerOpt& f) { return f.nblocks ? (size_t)2 * f.B * kOptL1MaxIn * sizeof(float) : 0; }
// is element i one of the first-layer parameters those blocks own (net_off: b1 follows W1, so a net's run is (in + 1) H1 long — a multiple of 4 when H1 % 4 == 0)
__device__ __forceinline__ bool first_layer_opt_owns(const FirstLayerOpt& f, int i) {
    if (!f.nblocks) return false;
    for (int z = 0; z < f.Z; ++z) { const int o = i - (f.w1 + (int)(z * f.zP)); if (o >= 0 && o < (f.in + 1) * f.H1) return true; }
    return false;
}
struct AdamRangeArgs { float* p; float* m; float* v; float* g; int n; float lr, b1, b2, eps, bt1, bt2; double* sumsq_partials; FirstLayerOpt fl; };
__global__ __launch_bounds__(256) void sac_adam_kernel(AdamRangeArgs a) {
    __shared__ double sh[256];
    double ss = 0;
    const int nfl = a.fl.nblocks, nb = gridDim.x - nfl, eb = (int)blockIdx.x - nfl;   // the first nfl blocks own the first layers (the longest dependent chain of the launch: dispatched first), the rest are elementwise
    const bool vec = (a.n & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.m) | reinterpret_cast<uintptr_t>(a.v) | reinterpret_cast<uintptr_t>(a.g)) & 15) == 0;
    if (eb < 0) ss = first_layer_opt_block(a.fl, blockIdx.x, a.p, a.m, a.v, a.g, a.lr, a.b1, a.b2, a.eps, a.bt1, a.bt2);
    else if (vec) {                                                                 // the padded device layout: 16-byte rows
        for (int i = eb * 256 + threadIdx.x; i < a.n / 4; i += nb * 256) {
            if (first_layer_opt_owns(a.fl, 4 * i)) continue;
            const float4 g = a.g ? *reinterpret_cast<const float4*>(a.g + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
            adam_vec(a.p, a.m, a.v, 4 * i, g, a.lr, a.b1, a.b2, a.eps, a.bt1, a.bt2);
            ss += (double)g.x * g.x + (double)g.y * g.y + (double)g.z * g.z + (double)g.w * g.w;
        }
    } else {
        for (int i = eb * 256 + threadIdx.x; i < a.n; i += nb * 256) {
            if (first_layer_opt_owns(a.fl, i)) continue;
            const float gi = a.g ? a.g[i] : 0.f;
            const float m = a.b1 * a.m[i] + (1.0f - a.b1) * gi, v = a.b2 * a.v[i] + (1.0f - a.b2) * gi * gi;
            a.m[i] = m; a.v[i] = v;
            a.p[i] -= m / (1.0f - a.bt1) / (sqrtf(v / (1.0f - a.bt2)) + a.eps) * a.lr;
            ss += (double)gi * gi;
        }
    }
    if (a.sumsq_partials) { ss = block_sum(ss, sh); if (threadIdx.x == 0) a.sumsq_partials[blockIdx.x] = ss; }
}
// End of one update!: apply_gradients(train_state, actor_loss_grad) (sac.jl:382 — actor_head and log_std with their gradients, the
// critic leaves with the ZERO arrays zero_critic_grads! left, :381), polyak_update! of the targets (:385-389, optimization_utils.jl:3-6)
// and the step's statistics, in ONE launch.  The block that finishes last sums the per-block partials in index order (deterministic).
struct StepEndArgs {
    float *p, *m, *v; const float* g_actor; int n_actor, ls_off, n_ls, q_off, n_q;
    float lr, b1, b2, eps, bt1_a, bt2_a, bt1_c, bt2_c;
    float* target; float tau; int do_polyak;
    double* ssq_a; float* stats; float* out;   // ssq_a: this update's row of squared-gradient partials, [end blocks] (the critic's partials sit in front of it)
    // deferred sums of the fused head kernels (nhead = 0: the unfused sequence wrote stats / the log_std gradient itself): per-sample rows [nhead][2] of the critic and
    // actor loss heads, [n_ls][nhead] of the log_std gradient
    int nhead, B; const double *hp_critic, *hp_actor, *hp_ls; float* g_ls;
    unsigned long long* stamp;   // phase_stamp (null: none)
    FirstLayerOpt fl;            // the actor's first layer: gradient + step in blocks of their own (nblocks = 0: its gradient is in g_actor like the rest)
    float* g_actor_w;            // (writable alias of g_actor for those blocks)
};
// n_actor and n_q are multiples of 4 (the device layout pads every net to 16 bytes; pads hold zero parameters and zero gradients)
__global__ __launch_bounds__(256) void sac_step_end_kernel(StepEndArgs a) {
    __shared__ double sh[256];
    const int va = a.n_actor / 4, vq = a.n_q / 4, nb = gridDim.x - a.fl.nblocks;
    double ss = 0;
    if ((int)blockIdx.x >= nb) ss = first_layer_opt_block(a.fl, blockIdx.x - nb, a.p, a.m, a.v, a.g_actor_w, a.lr, a.b1, a.b2, a.eps, a.bt1_a, a.bt2_a);
    else for (int i = blockIdx.x * 256 + threadIdx.x; i < va + vq; i += nb * 256) {
        if (i < va) {
            if (first_layer_opt_owns(a.fl, 4 * i)) continue;
            const float4 g = *reinterpret_cast<const float4*>(a.g_actor + 4 * i);
            adam_vec(a.p, a.m, a.v, 4 * i, g, a.lr, a.b1, a.b2, a.eps, a.bt1_a, a.bt2_a);
            ss += (double)g.x * g.x + (double)g.y * g.y + (double)g.z * g.z + (double)g.w * g.w;
        } else {
            const int k = 4 * (i - va);
            const float4 np_ = adam_vec(a.p, a.m, a.v, a.q_off + k, make_float4(0.f, 0.f, 0.f, 0.f), a.lr, a.b1, a.b2, a.eps, a.bt1_c, a.bt2_c);
            if (a.do_polyak) {
                float4 t = *reinterpret_cast<float4*>(a.target + k);
                t.x = a.tau * np_.x + (1.0f - a.tau) * t.x; t.y = a.tau * np_.y + (1.0f - a.tau) * t.y;
                t.z = a.tau * np_.z + (1.0f - a.tau) * t.z; t.w = a.tau * np_.w + (1.0f - a.tau) * t.w;
                *reinterpret_cast<float4*>(a.target + k) = t;
            }
        }
    }
    if (blockIdx.x == 0 && a.nhead) {                                                          // log_std gradient = sum of the per-sample terms (fixed order)
        for (int d = 0; d < a.n_ls; ++d) {
            double t = 0;
            for (int i = threadIdx.x; i < a.nhead; i += 256) t += a.hp_ls[(size_t)d * a.nhead + i];
            t = block_sum(t, sh);
            if (threadIdx.x == 0) a.g_ls[d] = (float)t;
            __syncthreads();
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < a.n_ls) {                                              // log_std: a handful of scalars
        const int j = a.ls_off + threadIdx.x; const float gi = a.nhead ? a.g_ls[threadIdx.x] : a.g_actor[j];
        adam_one(a.p, a.m, a.v, j, gi, a.lr, a.b1, a.b2, a.eps, a.bt1_a, a.bt2_a);
        ss += (double)gi * gi;
    }
    ss = block_sum(ss, sh);
    if (threadIdx.x == 0) a.ssq_a[blockIdx.x] = ss;          // squared-gradient partial of this block: summed on the host with the critic's (sac.jl:393) — no grid-wide fold for a statistic
    phase_stamp(a.stamp);
    if (blockIdx.x != 0) return;
    if (a.nhead) {                                                                              // statistics of the fused loss heads
        double c0 = 0, c1 = 0, p0 = 0;
        for (int i = threadIdx.x; i < a.nhead; i += 256) { c0 += a.hp_critic[2 * i]; c1 += a.hp_critic[2 * i + 1]; p0 += a.hp_actor[2 * i]; }
        c0 = block_sum(c0, sh); c1 = block_sum(c1, sh); p0 = block_sum(p0, sh);
        if (threadIdx.x == 0) { a.stats[1] = (float)c0; a.stats[3] = (float)(c1 / (2.0 * a.B)); a.stats[0] = (float)p0; }
    }
    if (threadIdx.x == 0) { a.out[0] = a.stats[0]; a.out[1] = a.stats[1]; a.out[2] = a.stats[2]; a.out[3] = a.stats[3]; a.out[4] = a.stats[4]; a.out[5] = 0.f; }
}

int adam_range(dril_sac_handle* h, int lo, int n, float* grads, const float* bt, double* ssq, int blocks, FirstLayerOpt fl = FirstLayerOpt{}) {
    AdamRangeArgs a{h->params + lo, h->adam_m + lo, h->adam_v + lo, grads ? grads + lo : nullptr, n, h->cfg.learning_rate, h->cfg.adam_beta1,
                    h->cfg.adam_beta2, h->cfg.adam_eps, bt[0], bt[1], ssq, fl};
    hipLaunchKernelGGL(sac_adam_kernel, dim3(blocks), dim3(256), first_layer_opt_lds(fl), h->stream, a);
    SHIP(h, hipGetLastError());
    return DRIL_OK;
}
void fill_stats(const dril_sac_handle* h, const float* rows, int n, dril_sac_stats* out) {
    for (int k = 0; k < n; ++k) {
        const float* r = rows + (size_t)k * 8; dril_sac_stats& s = out[k]; memset(&s, 0, sizeof(s));
        s.actor_loss = r[0]; s.critic_loss = r[1]; s.entropy_loss = h->cfg.auto_ent_coef ? r[2] : 0.f; s.mean_q_values = r[3];
        s.entropy_coefficient = r[4]; s.grad_norm = r[5]; s.has_entropy_loss = h->cfg.auto_ent_coef ? 1 : 0;
    }
}
void clear_injected(dril_sac_handle* h) {
    h->inj_idx.release(); h->inj_ne.release(); h->inj_nn.release(); h->inj_np.release(); h->inj_updates = 0;
}

}  // namespace

namespace dril::sac {
// one update!(agent, alg, batch): sac.jl:299-404.  `slot` = index into the injected batches (-1 = Philox), `out` = device stats row
int sac_one_update(dril_sac_handle* h, int slot, float* out, unsigned long long* stamp, double* ssq_row_in) {
    double* ssq_row = ssq_row_in ? ssq_row_in : h->ssq_rows + (size_t)((out - h->stats_out) / 8) * (h->adam_blocks_c + h->end_blocks);   // this update's squared-gradient partials: [critic Adam blocks | end blocks] (ssq_row_in: a row of the pending table, dril_sac_update_enqueue)
    const int B = h->cfg.batch_size, D = h->D, A = h->A, W = D + A;
    const SacRng rng{h->cfg.seed ^ 0x5ac5ac5ac5ac5ac5ull, h->update_counter};
    GatherArgs ga{B, D, A, h->cap, h->head, h->size, h->rb_obs, h->rb_next, h->rb_act, h->rb_rew, h->rb_term,
                  slot >= 0 && h->inj_idx ? h->inj_idx + (size_t)slot * B : nullptr, slot >= 0 && h->inj_ne ? h->inj_ne + (size_t)slot * B * A : nullptr,
                  slot >= 0 && h->inj_nn ? h->inj_nn + (size_t)slot * B * A : nullptr, slot >= 0 && h->inj_np ? h->inj_np + (size_t)slot * B * A : nullptr,
                  rng, h->xa, h->xq, h->b_rew, h->b_ne, h->b_nn, h->b_np, h->b_term};
    const int relu_ = h->cfg.activation ? 1 : 0;
    const bool l1 = h->fused_heads && W <= kFusedL1MaxIn;      // narrow inputs: first layers inside the gather / head kernels (two launches less)
    h->upd_route[0] = l1 ? 1 : 0; h->upd_route[1] = 0; h->upd_route[2] = 1;
    if (l1) {
        GatherL1Args gl{ga, h->H1, relu_, h->params + h->actor.w1, h->params + h->actor.b1, h->ah1, h->params, h->q0.w1, h->q0.b1, h->Pqd, (long long)h->nq * h->H1, h->qh1};
        hipLaunchKernelGGL(sac_gather_l1_kernel, dim3(B), dim3(256), 0, h->stream, gl);
    } else hipLaunchKernelGGL(sac_gather_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, ga);
    const int relu = h->cfg.activation ? 1 : 0, hb = (B + kHeadSamplesPerBlock - 1) / kHeadSamplesPerBlock;
    EntNextArgs en{B, D, A, h->mu, h->params + h->log_std_off, h->b_ne, h->b_nn, h->xa, h->xq_next, h->b_nlp, h->b_np, h->xq_pi, h->a_pi, h->g_pi, h->lp_pi, h->sc, h->target_entropy,
                   h->cfg.learning_rate, h->cfg.adam_beta1, h->cfg.adam_beta2, h->cfg.adam_eps, h->bt_ent[0], h->bt_ent[1], h->cfg.auto_ent_coef, h->stats};
    SquashBwdArgs sb{B, D, A, h->mu, h->params + h->log_std_off, h->b_np, h->a_pi, h->g_pi, h->dxq, h->sc, h->dmu, h->g_actor + h->log_std_off};
    const float ent_bt1 = h->bt_ent[0], ent_bt2 = h->bt_ent[1];
    if (h->fused_heads) {
        sb.sc = h->sc_next;                                                           // the state after this update's entropy step (written by the critic head kernel)
        // actor means of (obs | next obs): hidden layers as contractions, then output layer + entropy-coefficient step + next actions + the actor-loss sample in one launch
        SDO(net_forward(h, h->params, h->actor, 0, D, A, h->xa, D, 0, 2 * B, actor_bufs(h), 1, 1, true, l1));
        double* hp_critic = h->head_partials; double* hp_actor = hp_critic + 2 * (size_t)hb; double* hp_ls = hp_actor + 2 * (size_t)hb; double* hp_ent = hp_ls + (size_t)kMaxA * hb;   // one region per head kernel
        ActorHeadFusedArgs af{en, h->ah2, h->H2, h->params + h->actor.w3, h->params + h->actor.b3, h->mu, hp_ent, h->head_counter,
                              l1 ? 1 : 0, h->H1, relu, h->params, h->q0.w1, h->q0.b1, h->Pqd, (long long)h->nq * h->H1, h->qh1};
        const bool pre = W <= kL1PreMaxIn && (!l1 || h->H1 <= kL1PreMaxH);
        h->upd_route[1] = pre ? 1 : 0;
        if (pre) hipLaunchKernelGGL(sac_actor_out_ent_kernel<true>, dim3(hb), dim3(256), 0, h->stream, af);
        else hipLaunchKernelGGL(sac_actor_out_ent_kernel<false>, dim3(hb), dim3(256), 0, h->stream, af);
        if (h->cfg.auto_ent_coef) { h->bt_ent[0] *= h->cfg.adam_beta1; h->bt_ent[1] *= h->cfg.adam_beta2; }
        // critic: all four Q nets' hidden layers in one pass (z = 0,1 the critics on (obs, action), z = 2,3 the targets on (next obs, next action)), then output
        // layers + Bellman target + loss head + dz2 of the critics in one launch; [dW3|db3], [dW2|db2], dz1 in one launch; [dW1|db1]; Adam (:362)
        SDO(net_forward(h, h->params, h->q0, h->Pqd, W, 1, h->xq, W, (long long)h->nq * W, B, q_bufs(h, h->qh1, h->qh2, h->q_cur), 4, 2, true, l1));
        QHeadFusedArgs qc{B, h->H2, h->nq, relu, 4, h->Pqd, (long long)h->nq * h->H2, h->params, h->q0.w3, h->q0.b3, h->qh2, h->q_cur, h->dz2,
                          0, h->b_rew, h->b_nlp, h->lp_pi, h->b_term, h->sc, h->cfg.gamma, h->dq, h->stats, hp_critic, h->head_counter,
                          hp_ent, h->sc_next, h->cfg.auto_ent_coef, h->cfg.learning_rate, h->cfg.adam_beta1, h->cfg.adam_beta2, h->cfg.adam_eps, ent_bt1, ent_bt2};
        hipLaunchKernelGGL(sac_q_out_head_kernel, dim3(hb), dim3(256), 0, h->stream, qc);
        const bool fl = h->fused_dw1;
        SDO(net_backward(h, h->params, h->q0, h->Pqd, W, 1, h->xq, W, 0, B, q_bufs(h, h->qh1, h->qh2, h->q_cur), h->dq, h->g_critic, nullptr, 2, true, fl));
        FirstLayerOpt flc{};
        if (fl) flc = FirstLayerOpt{h->fl_c, 2, W, h->H1, B, relu, 0, h->q0.b1 - h->q0.w1, h->Pqd, h->dz1, (long long)h->nq * h->H1, h->xq, W, h->xq_pi, h->qh1, (long long)h->nq * h->H1};
        SDO(adam_range(h, h->q0.w1, 2 * h->Pqd, h->g_critic, h->bt_critic, ssq_row, h->adam_blocks_c, flc));
        h->bt_critic[0] *= h->cfg.adam_beta1; h->bt_critic[1] *= h->cfg.adam_beta2;
        // actor (:93-105) with the UPDATED critics: hidden layers, then output layers + loss head + dz2 in one launch; dz1; then the action columns of W1' dz1, the
        // reverse of the squashed sample and the actor's dz2 in one launch; the actor's [dW3|db3], [dW2|db2], dz1 in one launch; [dW1|db1]
        SDO(net_forward(h, h->params, h->q0, h->Pqd, W, 1, h->xq_pi, W, 0, B, q_bufs(h, h->qh1, h->qh2, h->q_pi), 2, 1, true, fl));   // (fl: the critics' Adam launch already evaluated the first layer)
        QHeadFusedArgs qp{B, h->H2, h->nq, relu, 2, h->Pqd, (long long)h->nq * h->H2, h->params, h->q0.w3, h->q0.b3, h->qh2, h->q_pi, h->dz2,
                          1, h->b_rew, h->b_nlp, h->lp_pi, h->b_term, h->sc_next, h->cfg.gamma, h->dq, h->stats, hp_actor, h->head_counter,
                          nullptr, nullptr, 0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        hipLaunchKernelGGL(sac_q_out_head_kernel, dim3(hb), dim3(256), 0, h->stream, qp);
        {   // dz1 = (W2' dz2) .* act'(h1) of both critics (no parameter gradients on this pass: Zygote differentiates the actor loss w.r.t. the actor only)
            const int H1 = h->H1, H2 = h->H2;
            GemmArgs g = gemm_args();
            g.A = h->params + h->q0.w2; g.sAm = H2; g.sAk = 1; g.zA = h->Pqd; g.B = h->dz2; g.sBk = 1; g.sBn = H2; g.zB = (long long)h->nq * H2;
            g.C = h->dz1; g.sCm = 1; g.sCn = H1; g.zC = (long long)h->nq * H1; g.aux = h->qh1; g.zAux = (long long)h->nq * H1; g.M = H1; g.N = B; g.K = H2;
            g.epi = relu ? EPI_MASK_RELU : EPI_MASK_TANH;
            SDO(gemm(h, g, 2));
        }
        SquashFusedArgs sf{sb, h->H1, h->H2, relu, h->nq, h->params, h->q0.w1, h->Pqd, h->dz1, h->params + h->actor.w3, h->ah2, h->dz2, hp_ls, h->head_counter};
        hipLaunchKernelGGL(sac_dx_squash_kernel, dim3(hb), dim3(256), 0, h->stream, sf);
        SDO(net_backward(h, h->params, h->actor, 0, D, A, h->xa, D, 0, B, actor_bufs(h), h->dmu, h->g_actor, nullptr, 1, true, fl));
        std::swap(h->sc, h->sc_next);                                                 // h->sc is the current state again for whoever reads it next
    } else {
        // actor means of (obs | next obs) in one pass: the entropy constant (:318-325) and the actor loss (:101) share the obs half,
        // the critic target (:131) uses the next-obs half; the actor parameters do not change until the actor step
        SDO(net_forward(h, h->params, h->actor, 0, D, A, h->xa, D, 0, 2 * B, actor_bufs(h), 1));
        hipLaunchKernelGGL(sac_ent_next_kernel, dim3(1), dim3(256), 0, h->stream, en);
        if (h->cfg.auto_ent_coef) { h->bt_ent[0] *= h->cfg.adam_beta1; h->bt_ent[1] *= h->cfg.adam_beta2; }
        // critic: target values with the target networks (:133-135), current values (:117), loss head, reverse pass, Adam (:362)
        // all four Q nets in one pass: z = 0,1 the critics on (obs, action), z = 2,3 the targets on (next obs, next action)
        SDO(net_forward(h, h->params, h->q0, h->Pqd, W, 1, h->xq, W, (long long)h->nq * W, B, q_bufs(h, h->qh1, h->qh2, h->q_cur), 4, 2));
        CriticHeadArgs ch{B, h->q_next, h->q_cur, h->b_rew, h->b_nlp, h->b_term, h->sc, h->cfg.gamma, h->dq, h->stats};
        hipLaunchKernelGGL(sac_critic_head_kernel, dim3(1), dim3(256), 0, h->stream, ch);
        SDO(net_backward(h, h->params, h->q0, h->Pqd, W, 1, h->xq, W, 0, B, q_bufs(h, h->qh1, h->qh2, h->q_cur), h->dq, h->g_critic, nullptr, 2));
        SDO(adam_range(h, h->q0.w1, 2 * h->Pqd, h->g_critic, h->bt_critic, ssq_row, h->adam_blocks_c));
        h->bt_critic[0] *= h->cfg.adam_beta1; h->bt_critic[1] *= h->cfg.adam_beta2;
        // actor (:93-105) with the UPDATED critics: sample, values, loss head, input gradients of the critics, squash reverse, actor reverse
        SDO(net_forward(h, h->params, h->q0, h->Pqd, W, 1, h->xq_pi, W, 0, B, q_bufs(h, h->qh1, h->qh2, h->q_pi), 2));
        ActorHeadArgs ah{B, h->q_pi, h->lp_pi, h->sc, h->dq, h->stats};
        hipLaunchKernelGGL(sac_actor_head_kernel, dim3(1), dim3(256), 0, h->stream, ah);
        SDO(net_backward(h, h->params, h->q0, h->Pqd, W, 1, h->xq_pi, W, 0, B, q_bufs(h, h->qh1, h->qh2, h->q_pi), h->dq, nullptr, h->dxq, 2));
        hipLaunchKernelGGL(sac_squash_bwd_kernel, dim3(1), dim3(256), 0, h->stream, sb);
        SDO(net_backward(h, h->params, h->actor, 0, D, A, h->xa, D, 0, B, actor_bufs(h), h->dmu, h->g_actor, nullptr, 1));
    }
    // apply_gradients(train_state, actor_loss_grad) :382 + target networks :385-389 + statistics: one launch
    const int do_polyak = h->grad_updates % h->cfg.target_update_interval == 0;
    StepEndArgs se{h->params, h->adam_m, h->adam_v, h->g_actor, round4(h->actor.end), h->log_std_off, A, h->q0.w1, 2 * h->Pqd,
                   h->cfg.learning_rate, h->cfg.adam_beta1, h->cfg.adam_beta2, h->cfg.adam_eps, h->bt_actor[0], h->bt_actor[1], h->bt_critic[0], h->bt_critic[1],
                   h->target, h->cfg.tau, do_polyak, ssq_row + h->adam_blocks_c, h->stats, out,
                   h->fused_heads ? hb : 0, B, h->head_partials, h->head_partials + 2 * (size_t)hb, h->head_partials + 4 * (size_t)hb, h->g_actor + h->log_std_off, stamp,
                   FirstLayerOpt{}, h->g_actor};
    if (h->fused_heads && h->fused_dw1)      // the actor's [dW1 | db1] = dz1 . [obs' | 1] and its step: blocks of this launch
        se.fl = FirstLayerOpt{h->fl_a, 1, D, h->H1, B, relu_, h->actor.w1, h->actor.b1, 0, h->dz1, 0, h->xa, D, nullptr, nullptr, 0};
    hipLaunchKernelGGL(sac_step_end_kernel, dim3(h->end_blocks), dim3(256), first_layer_opt_lds(se.fl), h->stream, se);
    SHIP(h, hipGetLastError());
    h->bt_actor[0] *= h->cfg.adam_beta1; h->bt_actor[1] *= h->cfg.adam_beta2;
    h->bt_critic[0] *= h->cfg.adam_beta1; h->bt_critic[1] *= h->cfg.adam_beta2;
    h->grad_updates += 1; h->update_counter += 1; h->col_w2_dirty = true;      // (the actor moved: its W2 planes are re-cut by the next collection step)
    return DRIL_OK;
}

int ensure_stats(dril_sac_handle* h, int n) {
    if (n <= 0) return DRIL_OK;
    SHIP(h, h->stats_out.grow_zero((size_t)n * 8)); SHIP(h, h->ssq_rows.grow_zero((size_t)n * (h->adam_blocks_c + h->end_blocks)));
    return DRIL_OK;
}
// the statistics rows of the last n gradient steps (stream drained): device rows + the squared-gradient partials summed here
int fetch_stats(dril_sac_handle* h, int n, dril_sac_stats* out, const float* rows_dev, const double* ssq_dev) {
    std::vector<float> rows((size_t)n * 8);
    SHIP(h, hipMemcpy(rows.data(), rows_dev ? rows_dev : h->stats_out, rows.size() * 4, hipMemcpyDeviceToHost));
    const int nb = h->adam_blocks_c + h->end_blocks;
    std::vector<double> ssq((size_t)n * nb);
    SHIP(h, hipMemcpy(ssq.data(), ssq_dev ? ssq_dev : h->ssq_rows, ssq.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < n; ++k) { double t = 0; for (int b = 0; b < nb; ++b) t += ssq[(size_t)k * nb + b]; rows[(size_t)k * 8 + 5] = (float)sqrt(t); }   // grad_norm, sac.jl:393 (index order: deterministic)
    fill_stats(h, rows.data(), n, out);
    return DRIL_OK;
}
int run_updates(dril_sac_handle* h, int n_updates, bool injected, dril_sac_stats* out) {
    if (h->size <= 0) return sfail(h, DRIL_ERR_NOT_INITIALISED, "the replay buffer is empty");
    SDO(ensure_stats(h, n_updates));
    if (h->cfg.profile_events) hipEventRecord(h->ev_a, h->stream);
    const auto t_enq0 = std::chrono::steady_clock::now();
    for (int k = 0; k < n_updates; ++k) SDO(sac_one_update(h, injected ? k : -1, h->stats_out + (size_t)k * 8));
    if (h->cfg.profile_events) hipEventRecord(h->ev_b, h->stream);
    const auto t_enq1 = std::chrono::steady_clock::now();
    SDO(ssync(h));
    if (h->trace_enqueue) {
        const auto t_done = std::chrono::steady_clock::now();
        fprintf(stderr, "[dril_sac] %d update(s): enqueue %.1f us, until drained %.1f us\n", n_updates,
                std::chrono::duration<double, std::micro>(t_enq1 - t_enq0).count(), std::chrono::duration<double, std::micro>(t_done - t_enq0).count());
    }
    if (h->cfg.profile_events) { float ms = 0; if (hipEventElapsedTime(&ms, h->ev_a, h->ev_b) == hipSuccess) { h->update_ms += ms; h->updates += n_updates; } }
    if (out) SDO(fetch_stats(h, n_updates, out));
    return DRIL_OK;
}
}  // namespace dril::sac

DRIL_EXPORT int32_t dril_sac_debug_set_batches(dril_sac_handle* h, int32_t n_updates, const int64_t* idx, const float* ne, const float* nn, const float* np) {
    SNEED(h); SDO(ssync(h));
    clear_injected(h);
    if (n_updates <= 0) return DRIL_OK;
    const size_t nb = (size_t)n_updates * h->cfg.batch_size, na = nb * h->A;
    if (idx) {
        for (size_t i = 0; i < nb; ++i) if (idx[i] < 0 || idx[i] >= h->size) return sfail(h, DRIL_ERR_INVALID_ARG, "injected replay index out of range");
        SHIP(h, h->inj_idx.alloc_zero(nb)); SHIP(h, hipMemcpy(h->inj_idx, idx, nb * 8, hipMemcpyHostToDevice));
    }
    if (ne) { SHIP(h, h->inj_ne.alloc_zero(na)); SHIP(h, hipMemcpy(h->inj_ne, ne, na * 4, hipMemcpyHostToDevice)); }
    if (nn) { SHIP(h, h->inj_nn.alloc_zero(na)); SHIP(h, hipMemcpy(h->inj_nn, nn, na * 4, hipMemcpyHostToDevice)); }
    if (np) { SHIP(h, h->inj_np.alloc_zero(na)); SHIP(h, hipMemcpy(h->inj_np, np, na * 4, hipMemcpyHostToDevice)); }
    h->inj_updates = n_updates;
    return DRIL_OK;
}
DRIL_EXPORT int32_t dril_sac_update(dril_sac_handle* h, int32_t n_updates, dril_sac_stats* out) {
    SNEED(h); if (n_updates <= 0) return sfail(h, DRIL_ERR_INVALID_ARG, "n_updates must be positive");
    if (h->inj_updates && h->inj_updates != n_updates) return sfail(h, DRIL_ERR_INVALID_ARG, "injected batches were set for a different n_updates");
    const int rc = run_updates(h, n_updates, h->inj_updates != 0, out);
    clear_injected(h);
    return rc;
}
// which launches the last sac_one_update enqueued, from what that function decided (no launch, no device read): the route of tests/sac_update_cases.py
DRIL_EXPORT const char* dril_sac_update_info(const dril_sac_handle* h) {
    if (!h) return "";
    if (!h->upd_route[2]) return "none";
    const int B = h->cfg.batch_size, hb = (B + kHeadSamplesPerBlock - 1) / kHeadSamplesPerBlock;
    const bool l1 = h->upd_route[0] != 0, pre = h->upd_route[1] != 0, fl = h->fused_heads && h->fused_dw1;
    std::snprintf(h->upd_info, sizeof(h->upd_info), "gather=%s head=%s dw1=%s l1pre=%d hb=%d adam_blocks=%d end_blocks=%d fl_blocks=%d",
                  l1 ? "l1" : "plain", !h->fused_heads ? "unfused" : pre ? "fused,pre" : "fused,nopre", fl ? "fused" : "launch", l1 && pre ? 1 : 0,
                  h->fused_heads ? hb : 1, h->adam_blocks_c, h->end_blocks, fl ? h->fl_c + h->fl_a : 0);
    return h->upd_info;
}
DRIL_EXPORT int32_t dril_sac_get_last_grads(dril_sac_handle* h, float* gc, float* ga, size_t n) {
    SNEED(h); if (n != (size_t)h->P) return sfail(h, DRIL_ERR_INVALID_ARG, "dril_sac_get_last_grads: n must equal dril_sac_param_count");
    if (gc) { memset(gc, 0, n * 4); SDO(ssync(h));
        for (int k = 0; k < 2; ++k) SHIP(h, hipMemcpy(gc + h->Pa + (size_t)k * h->Pq, h->g_critic + h->q0.w1 + (size_t)k * h->Pqd, (size_t)h->Pq * 4, hipMemcpyDeviceToHost)); }
    if (ga) { memset(ga, 0, n * 4); SDO(ssync(h));
        SHIP(h, hipMemcpy(ga, h->g_actor, (size_t)h->Pa * 4, hipMemcpyDeviceToHost));
        SHIP(h, hipMemcpy(ga + h->Pa + 2 * (size_t)h->Pq, h->g_actor + h->log_std_off, (size_t)h->A * 4, hipMemcpyDeviceToHost)); }
    return DRIL_OK;
}
