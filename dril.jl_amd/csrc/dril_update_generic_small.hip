// dril_update_generic_small.hip — ppo_update_generic_small_kernel: the epoch x minibatch loop of train! (ppo.jl:205-239) for a handle on the GENERIC path (a device env
// plug-in, DRIL_ENV_EXTERNAL, a built-in env with other hidden_dims / activation) at the reference's own scale (batch_size <= 64), every optimiser step inside one
// launch of ONE workgroup.  Per step the layer-by-layer route (generic_ppo_grad + grad_reduce_kernel + adam_kernel) is 3 nh + 6 dependent launches of a few
// microseconds of work each; here a step is a few dozen workgroup barriers.
//
//   Every net shape is a run-time argument (GuLayout, built on the host from GenericDims): 1..4 hidden layers, any width <= kGuMaxWidth, any of the eight activations.
//   The only synchronisation is the workgroup barrier: no second workgroup, no spin-wait, no atomic; every loop bound is known at launch, so the kernel cannot hang.
//   Arithmetic: f32 FMA on the VALU throughout (as policy_act_kernel and the plug-in rollout), accurate libm in the loss head (dril_ppo_head.h, shared with
//   generic_loss_head_kernel), float64 for the advantage moments, the statistics sums and |g|^2.  Every sum has an order fixed by the launch shape: two runs give the
//   same bits, and since all state a launch leaves (params, adam_m, adam_v, beta powers) goes through global memory as f32, so does any cut of the steps into launches.
//
//   LDS (dynamic): [ parameters, padded | gradients, same layout | activation panels of one sample tile ]
//     a layer's block: (in + 1) rows of OP = roundup(out, 4) floats — row k < in is column k of W (W is out x in, column-major in the flat vector), row `in` the bias;
//       the padding of the PARAMETER block stays zero for the whole launch (Adam walks the real entries only); the gradient block's padding and the panel rows between a
//       width and its multiple of 4 may hold stale finite values: they meet zero parameters or are never read.  log_std follows the critic.
//     a panel: rows of TS + 4 floats, one row per unit, one column per sample of the tile (TS = 32, or 16 where 32 does not fit the 160 KB).
//   per optimiser step:  indices + advantages of the minibatch | B | moments (wave 0) | B | for net in (actor, critic), for tile:  gather | B | nh + 1 forward layers,
//     a barrier each | loss head (one thread per sample) | B | nh + 1 reverse stages ([dW_l | db_l] into the gradient block and dz_(l-1) side by side), a barrier each |
//     then |g|^2 (two barriers), statistics row, NaN / KL decision, Adam on the LDS copy with the moments in global memory | B.
//   Same order of operations per optimiser step as ppo.jl:207-239: gradient -> NaN / Inf check -> norm -> clip -> KL check (skip this apply, stop) -> Adam.
#include <string>

#include "dril_grad_common.h"
#include "dril_ppo_head.h"
#include "dril_pop_map.h"

namespace dril {

namespace {
constexpr int kGuThreads = 512;   // two waves per SIMD: a reverse stage's two pieces ([dW | db] and dz) run side by side on the two halves of the workgroup
constexpr size_t kGuLdsMax = 160 * 1024;
__host__ __device__ inline int gu_pad4(int v) { return (v + 3) & ~3; }

// sum over the 64 lanes of a wave, the same bits in every lane (butterflies: a fixed order)
__device__ __forceinline__ double gu_wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <int TS> struct GuTile { static constexpr int TSP = TS + 4, SG = TS / 2; };

// y[o][s] = act(b[o] + sum_k W[o][k] x[k][s]); a thread owns 4 consecutive units x 2 consecutive samples
template <int TS>
__device__ __forceinline__ void gu_forward(const float* Wp, int lw, int I, int O, int OP, const float* xin, float* yout, float* zout, int act, bool last, int tid) {
    constexpr int TSP = GuTile<TS>::TSP, SG = GuTile<TS>::SG;
    const int items = (OP >> 2) * SG;
    for (int it = tid; it < items; it += kGuThreads) {
        const int sg = it % SG, og = it / SG, o0 = 4 * og, s0 = 2 * sg;
        const float4 b = *reinterpret_cast<const float4*>(Wp + lw + I * OP + o0);
        float acc[4][2] = {{b.x, b.x}, {b.y, b.y}, {b.z, b.z}, {b.w, b.w}};
        const float* wr = Wp + lw + o0; const float* xr = xin + s0;
#pragma unroll 8
        for (int k = 0; k < I; ++k) {                                              // (unrolled: at two waves per SIMD little else covers an LDS round trip, so the loads of eight steps go out together)
            const float4 w = *reinterpret_cast<const float4*>(wr + k * OP);
            const float2 x = *reinterpret_cast<const float2*>(xr + k * TSP);
            acc[0][0] = fmaf(w.x, x.x, acc[0][0]); acc[0][1] = fmaf(w.x, x.y, acc[0][1]);
            acc[1][0] = fmaf(w.y, x.x, acc[1][0]); acc[1][1] = fmaf(w.y, x.y, acc[1][1]);
            acc[2][0] = fmaf(w.z, x.x, acc[2][0]); acc[2][1] = fmaf(w.z, x.y, acc[2][1]);
            acc[3][0] = fmaf(w.w, x.x, acc[3][0]); acc[3][1] = fmaf(w.w, x.y, acc[3][1]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (o0 + j >= O) continue;
            float2 v = make_float2(acc[j][0], acc[j][1]);
            if (zout) *reinterpret_cast<float2*>(zout + (o0 + j) * TSP + s0) = v;
            if (!last) { v.x = activation_forward(act, v.x); v.y = activation_forward(act, v.y); }
            *reinterpret_cast<float2*>(yout + (o0 + j) * TSP + s0) = v;
        }
    }
}
// dz[k][s] = (sum_o W[o][k] up[o][s]) act'(mask[k][s]); a thread owns 4 consecutive units k x 2 consecutive samples
template <int TS>
__device__ __forceinline__ void gu_backward_data(const float* Wp, int lw, int I, int OP, const float* up, const float* mask, float* dz, int act, int tid) {
    constexpr int TSP = GuTile<TS>::TSP, SG = GuTile<TS>::SG;
    const int items = ((I + 3) >> 2) * SG;
    for (int it = tid; it < items; it += kGuThreads) {
        const int sg = it % SG, kg = it / SG, k0 = 4 * kg, s0 = 2 * sg;
        float acc[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
        const float* wr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wr[j] = Wp + lw + (k0 + j < I ? k0 + j : I - 1) * OP;            // (rows past the layer: a real row again, the result is not stored)
#pragma unroll 2
        for (int o4 = 0; o4 < OP; o4 += 4) {
            float2 u[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = *reinterpret_cast<const float2*>(up + (o4 + i) * TSP + s0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 w = *reinterpret_cast<const float4*>(wr[j] + o4);
                acc[j][0] = fmaf(w.x, u[0].x, acc[j][0]); acc[j][1] = fmaf(w.x, u[0].y, acc[j][1]);
                acc[j][0] = fmaf(w.y, u[1].x, acc[j][0]); acc[j][1] = fmaf(w.y, u[1].y, acc[j][1]);
                acc[j][0] = fmaf(w.z, u[2].x, acc[j][0]); acc[j][1] = fmaf(w.z, u[2].y, acc[j][1]);
                acc[j][0] = fmaf(w.w, u[3].x, acc[j][0]); acc[j][1] = fmaf(w.w, u[3].y, acc[j][1]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k0 + j >= I) continue;
            const float2 m = *reinterpret_cast<const float2*>(mask + (k0 + j) * TSP + s0);
            *reinterpret_cast<float2*>(dz + (k0 + j) * TSP + s0) = make_float2(acc[j][0] * activation_grad(act, m.x), acc[j][1] * activation_grad(act, m.y));
        }
    }
}
// G[o][k] (+)= sum_s up[o][s] x[k][s] (a thread owns 4 units o x 4 inputs k), G[o][bias] (+)= sum_s up[o][s]; samples in index order
template <int TS>
__device__ __forceinline__ void gu_backward_weights(float* G, int lw, int I, int O, int OP, const float* up, const float* xin, bool first, int tid) {
    constexpr int TSP = GuTile<TS>::TSP;
    const int OG = OP >> 2, items = OG * ((I + 3) >> 2);
    for (int it = (tid + kGuThreads / 2) % kGuThreads; it < items; it += kGuThreads) {   // (the upper half of the workgroup first: the lower half has the dz items of the same stage)
        const int og = it % OG, kg = it / OG, o0 = 4 * og, k0 = 4 * kg;
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
#pragma unroll 2
        for (int s4 = 0; s4 < TS; s4 += 4) {
            float4 u[4], x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = *reinterpret_cast<const float4*>(up + (o0 + j) * TSP + s4);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const float4*>(xin + (k0 + i) * TSP + s4);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float t = acc[i][j];
                    t = fmaf(u[j].x, x[i].x, t); t = fmaf(u[j].y, x[i].y, t); t = fmaf(u[j].z, x[i].z, t); t = fmaf(u[j].w, x[i].w, t);
                    acc[i][j] = t;
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (k0 + i >= I) continue;
            float4* g = reinterpret_cast<float4*>(G + lw + (k0 + i) * OP + o0);
            float4 v = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
            if (!first) { const float4 p = *g; v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w; }
            *g = v;
        }
    }
    for (int o = tid - 128; o < O; o += kGuThreads) {                                      // (waves 2 and 3, which have the fewest items of either kind)
        if (o < 0) continue;
        float t = 0.f;
        for (int s = 0; s < TS; ++s) t += up[o * TSP + s];
        float* g = G + lw + I * OP + o;
        *g = first ? t : *g + t;
    }
}

// the kernel's body: the run of optimiser steps a.u.step0 .. + a.u.nsteps of ONE handle by ONE workgroup (the solo kernel on its argument, the population kernel on its member's block)
// L: a's LDS plan (a.lay), named apart because its arrays are indexed at run time: the solo kernel reads them from its kernel argument, the population kernel from the
// member table itself — a private copy of such arrays would live in scratch memory
template <int TS>
__device__ __forceinline__ void gu_update_body(const GenericUpdateArgs& a, const GuLayout& L) {
    constexpr int TSP = GuTile<TS>::TSP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ long long sidx[64];
    __shared__ float sadv[64];
    __shared__ float smom[2];
    __shared__ double sacc[8];
    __shared__ double sred[16];
    const SmallUpdateArgs& u = a.u;
    if (*u.stop_flag) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int PP = L.PP, A = a.A, D = a.D, nl = L.nl, act = a.act_code;
    float* Wp = smem; float* G = smem + PP; float* pan = smem + 2 * PP;
    float* X = pan + L.x; float* OUT = pan + L.outb; float* DOUT = pan + L.dout; float* ACT = pan + L.actb; float* SC = pan + L.sc;
    // rows of SC: 0 adv, 1 logp_old, 2 ret, 3 val_old, 4 valid, 5 dLoss/dlogp, 6..11 the six statistics terms of the sample
    // ---- the launch's state into LDS: everything zero first (the padding of every block and panel stays finite), then the parameters into their padded blocks ----
    for (int i = tid; i < 2 * PP + L.total; i += kGuThreads) smem[i] = 0.f;
    __syncthreads();
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l < nl; ++l) {
            const int O = L.out[n][l], OP = L.op[n][l], cnt = (L.in[l] + 1) * O;
            for (int i = tid; i < cnt; i += kGuThreads) { const int k = i / O, o = i - k * O; Wp[L.lw[n][l] + k * OP + o] = u.params[L.fw[n][l] + i]; }
        }
    if (!a.discrete && tid < A) Wp[L.ls + tid] = u.params[u.Pa + u.Pc + tid];
    const float* bt_in = u.bt + 2 * (u.step_parity & 1);
    float bt1 = bt_in[0], bt2 = bt_in[1];
    GradArgs ga{};                                                                    // what the loss head reads
    ga.clip_range = u.clip_range; ga.ent_coef = u.ent_coef; ga.vf_coef = u.vf_coef; ga.clip_range_vf = u.clip_range_vf; ga.has_clip_vf = u.has_clip_vf;
    ga.normalize_adv = u.normalize_adv; ga.action_start = u.action_start;
    __syncthreads();
    const int s_end = u.step0 + u.nsteps;
    for (int s = u.step0; s < s_end; ++s) {
        const int ep = s / u.nb, kb = s - ep * u.nb;
        const int64_t pos0 = (int64_t)kb * u.B;
        const int count = (int)((pos0 + u.B <= u.N) ? u.B : u.N - pos0);
        ga.invB = 1.0f / (float)count;
        // ---- DataLoader order of the minibatch and its advantages ----
        if (tid < 64) {
            long long idx = 0; float av = 0.f;
            if (tid < count) { idx = u.perm ? u.perm[(int64_t)ep * u.N + pos0 + tid] : perm_index(pos0 + tid, u.N, u.keys[ep], u.perm_bits); av = a.adv[idx]; }
            sidx[tid] = idx; sadv[tid] = av;
        }
        if (tid < 8) sacc[tid] = 0.0;
        __syncthreads();
        if (wave == 0) {                                                              // normalize!(advantages) per minibatch, ppo.jl:350-356 (corrected std + 1e-8)
            float mean_f = 0.f, inv_f = 1.f;
            if (u.normalize_adv) {
                const double v = lane < count ? (double)sadv[lane] : 0.0;
                const double sm = gu_wave_sum_f64(v), sq = gu_wave_sum_f64(v * v), n = (double)count;
                const double mean = sm / n;
                double var = (sq - sm * mean) / (n - 1.0);
                if (var < 0) var = 0;
                mean_f = (float)mean; inv_f = 1.0f / ((float)sqrt(var) + 1.0e-8f);
            }
            if (lane == 0) { smom[0] = mean_f; smom[1] = inv_f; }
        }
        __syncthreads();
        const int ntiles = (count + TS - 1) / TS;
        for (int n = 0; n < 2; ++n) {
            for (int tile = 0; tile < ntiles; ++tile) {
                const int t0 = tile * TS; const bool first = tile == 0;
                // ---- gather (DataLoader, ppo.jl:188-195): observations into the X panel, the per-sample scalars and the action (a one-tile minibatch: the actor's gather serves the critic) ----
                if (n == 0 || ntiles > 1) {
                for (int e = tid; e < D * TS; e += kGuThreads) {
                    const int sl = e % TS, k = e / TS; const bool valid = t0 + sl < count;
                    X[k * TSP + sl] = valid ? a.obs[sidx[valid ? t0 + sl : 0] * D + k] : 0.f;
                }
                if (tid < TS) {
                    const bool valid = t0 + tid < count; const long long idx = sidx[valid ? t0 + tid : 0];
                    SC[0 * TSP + tid] = valid ? sadv[t0 + tid] : 0.f; SC[1 * TSP + tid] = valid ? a.logp[idx] : 0.f; SC[2 * TSP + tid] = valid ? a.ret[idx] : 0.f;
                    SC[3 * TSP + tid] = (valid && u.has_clip_vf) ? u.val_old[idx] : 0.f; SC[4 * TSP + tid] = valid ? 1.f : 0.f;
                    if (a.discrete) reinterpret_cast<int*>(ACT)[tid] = valid ? ((const int32_t*)a.actions)[idx] : u.action_start;
                } else if (!a.discrete && tid >= 64 && tid < 64 + TS) {
                    const int sl = tid - 64; const bool valid = t0 + sl < count; const long long idx = sidx[valid ? t0 + sl : 0];
                    for (int k = 0; k < A; ++k) ACT[k * TSP + sl] = valid ? ((const float*)a.actions)[idx * A + k] : 0.f;
                }
                __syncthreads();
                }
                // ---- forward ----
                for (int l = 0; l < nl; ++l) {
                    const bool last = l == nl - 1;
                    gu_forward<TS>(Wp, L.lw[n][l], L.in[l], L.out[n][l], L.op[n][l], l == 0 ? X : pan + L.hb[l - 1], last ? OUT : pan + L.hb[l],
                                   (!last && a.need_z) ? pan + L.zb[l] : nullptr, act, last, tid);
                    __syncthreads();
                }
                // ---- loss head: one thread per sample of the tile ----
                if (tid < TS) {
                    const bool valid = SC[4 * TSP + tid] != 0.f;
                    if (n == 0) {
                        float dlogp, ps[5];
                        const float advn = (SC[0 * TSP + tid] - smom[0]) * smom[1];
                        ppo_policy_sample(ga, A, a.discrete, valid, OUT + tid, TSP, reinterpret_cast<const int*>(ACT)[tid], ACT + tid, TSP, advn, SC[1 * TSP + tid], Wp + L.ls,
                                          DOUT + tid, TSP, dlogp, ps);
                        SC[5 * TSP + tid] = dlogp;
#pragma unroll
                        for (int k = 0; k < 5; ++k) SC[(6 + k) * TSP + tid] = valid ? ps[k] : 0.f;
                    } else {
                        float ve2;
                        DOUT[tid] = ppo_value_sample(ga, valid, SC[2 * TSP + tid], SC[3 * TSP + tid], OUT[tid], ve2);
                        SC[11 * TSP + tid] = valid ? ve2 : 0.f;
                    }
                }
                __syncthreads();
                // ---- the minibatch's statistics sums and the log_std gradient: one thread per sum, samples in index order, beside the first reverse stage ----
                if (wave == 7) {
                    const int q = lane;
                    if ((n == 0 && q < 5) || (n == 1 && q == 5)) {
                        double t = 0;
                        for (int sl = 0; sl < TS; ++sl) t += (double)SC[(6 + q) * TSP + sl];
                        sacc[q] += t;
                    } else if (n == 0 && !a.discrete && q >= 8 && q < 8 + A) {
                        const int k = q - 8; const float iv = expf(-2.0f * Wp[L.ls + k]);
                        double t = 0;
                        for (int sl = 0; sl < TS; ++sl) if (SC[4 * TSP + sl] != 0.f) t += (double)ppo_log_std_term(ga, SC[5 * TSP + sl], ACT[k * TSP + sl], OUT[k * TSP + sl], iv);
                        G[L.ls + k] = first ? (float)t : G[L.ls + k] + (float)t;
                    }
                }
                // ---- reverse pass: stage l writes [dW_l | db_l] and dz_(l-1); up = DOUT, then the dz panels in turn ----
                const float* up = DOUT;
                for (int l = nl - 1; l >= 0; --l) {
                    const float* xin = l == 0 ? X : pan + L.hb[l - 1];
                    float* dzn = pan + L.dz[l & 1];
                    if (l > 0) gu_backward_data<TS>(Wp, L.lw[n][l], L.in[l], L.op[n][l], up, a.need_z ? pan + L.zb[l - 1] : xin, dzn, act, tid);
                    gu_backward_weights<TS>(G, L.lw[n][l], L.in[l], L.out[n][l], L.op[n][l], up, xin, first, tid);
                    __syncthreads();
                    up = dzn;
                }
            }
        }
        // ---- |g|^2 over all leaves: per thread in layer order, then the workgroup (fixed order) ----
        double ss = 0;
        for (int n = 0; n < 2; ++n)
            for (int l = 0; l < nl; ++l) {
                const int O = L.out[n][l], OP = L.op[n][l], cnt = (L.in[l] + 1) * O, dq = kGuThreads / O, dr = kGuThreads - dq * O;
                int k = tid / O, o = tid - k * O;
                for (int i = tid; i < cnt; i += kGuThreads) {
                    const double g = (double)G[L.lw[n][l] + k * OP + o]; ss += g * g;
                    k += dq; o += dr; if (o >= O) { o -= O; k += 1; }
                }
            }
        if (!a.discrete && tid < A) { const double g = (double)G[L.ls + tid]; ss += g * g; }
        const float norm = sqrtf((float)block_sum_f64(ss, sred));
        const float nf = (float)count;
        const float st3 = (float)sacc[3], kl = st3 / nf;
        const bool bad = !(norm == norm) || isinf(norm);                              // NaN / Inf anywhere poisons the norm (ppo.jl:213-214)
        const bool kl_stop = u.has_target_kl && kl > 1.5f * u.target_kl;              // ppo.jl:235-238: skip this apply, stop
        if (tid == 0) {
            float* o = u.step_stats + (size_t)s * 16;
            const float pl = (float)sacc[0] / nf, ent = (float)sacc[1] / nf, vl = (float)sacc[5] / nf;
            o[0] = pl; o[1] = vl; o[2] = -ent; o[3] = (float)sacc[2] / nf; o[4] = kl; o[5] = ent; o[6] = (float)sacc[4] / nf;
            o[7] = pl + u.ent_coef * (-ent) + u.vf_coef * vl;                          // loss, ppo.jl:386
            o[8] = norm; o[9] = (bad || kl_stop) ? 0.f : 1.f; o[10] = bad ? 1.f : 0.f; o[11] = kl_stop ? 1.f : 0.f;
            if (u.norm_out) *u.norm_out = norm;
            if (bad) { *u.nan_flag = 1; *u.stop_flag = 1; }
            if (kl_stop) *u.stop_flag = 1;
        }
        if (bad || kl_stop) break;                                                    // uniform: every thread computed the same norm / kl
        const float scale = (u.has_max_grad_norm && norm > u.max_grad_norm) ? u.max_grad_norm / norm : 1.0f;   // optimization_utils.jl:98-107
        // ---- Adam (Optimisers.Adam, eps = 1e-5, ppo.jl:64-66): the moments in global memory, the parameters in LDS ----
        float* __restrict__ am = u.adam_m; float* __restrict__ av = u.adam_v;           // (no two threads share an entry: the loads of an unrolled batch go out together)
        auto adam = [&](int p, int off) {
            float g = G[off];
            if (scale != 1.0f) g = g * scale;
            // which of the two products joins the FMA is written out: left to the compiler the solo and the population kernel contracted the first line differently
            // (one rounding apart).  These are the forms the solo kernel has always compiled to
            const float m = fmaf(g, 1.0f - u.beta1, u.beta1 * am[p]);
            const float v = fmaf(u.beta2, av[p], (1.0f - u.beta2) * g * g);
            am[p] = m; av[p] = v;
            Wp[off] -= m / (1.0f - bt1) / (sqrtf(v / (1.0f - bt2)) + u.eps) * u.lr;
        };
        for (int n = 0; n < 2; ++n)
            for (int l = 0; l < nl; ++l) {
                const int O = L.out[n][l], OP = L.op[n][l], cnt = (L.in[l] + 1) * O, dq = kGuThreads / O, dr = kGuThreads - dq * O;
                int k = tid / O, o = tid - k * O;
#pragma unroll 4
                for (int i = tid; i < cnt; i += kGuThreads) {
                    adam(L.fw[n][l] + i, L.lw[n][l] + k * OP + o);
                    k += dq; o += dr; if (o >= O) { o -= O; k += 1; }
                }
            }
        if (!a.discrete && tid < A) adam(u.Pa + u.Pc + tid, L.ls + tid);
        bt1 *= u.beta1; bt2 *= u.beta2;
        __syncthreads();
    }
    // ---- state back to global memory ----
    __syncthreads();
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l < nl; ++l) {
            const int O = L.out[n][l], OP = L.op[n][l], cnt = (L.in[l] + 1) * O;
            for (int i = tid; i < cnt; i += kGuThreads) { const int k = i / O, o = i - k * O; u.params[L.fw[n][l] + i] = Wp[L.lw[n][l] + k * OP + o]; }
        }
    if (!a.discrete && tid < A) u.params[u.Pa + u.Pc + tid] = Wp[L.ls + tid];
    if (tid == 0) { u.bt[0] = bt1; u.bt[1] = bt2; u.bt[2] = bt1; u.bt[3] = bt2; }     // both ping-pong slots: the host's step parity no longer matters
}

template <int TS>
__global__ __launch_bounds__(kGuThreads, 1) void ppo_update_generic_small_kernel(GenericUpdateArgs a) { gu_update_body<TS>(a, a.lay); }

// ppo_update_generic_small_pop_kernel — n members of a population (dril_population_*, docs/population.md, "Plug-in members") in one launch: workgroup m copies
// members[m] (uniform loads), takes what it dereferences through the global address space once (pop_global) and runs the body above on the copy (the LDS plan is read from the table in place): the solo kernel's
// device code on the solo launch's own argument block.  Workgroups share nothing (each member has its own parameters, moments, buffers, flags and statistics rows) and
// never wait for one another: no co-residency is needed, no cap on n — workgroups beyond what is resident start when others have finished.  A member whose stop_flag
// is set (target_kl, a non-finite gradient in an earlier launch of the chunked sequence) leaves at once, as in the solo kernel.
template <int TS>
__global__ __launch_bounds__(kGuThreads, 1) void ppo_update_generic_small_pop_kernel(const GenericUpdateArgs* __restrict__ members, int n) {
    if ((int)blockIdx.x >= n) return;
    const GenericUpdateArgs& src = members[blockIdx.x];
    GenericUpdateArgs a;                                                               // every field but lay, which the body reads in place
    a.u = src.u; a.D = src.D; a.A = src.A; a.discrete = src.discrete; a.act_code = src.act_code; a.need_z = src.need_z;
    a.obs = src.obs; a.actions = src.actions; a.adv = src.adv; a.ret = src.ret; a.logp = src.logp;
    SmallUpdateArgs& u = a.u;
    u.params = pop_global(u.params); u.adam_m = pop_global(u.adam_m); u.adam_v = pop_global(u.adam_v); u.bt = pop_global(u.bt); u.val_old = pop_global(u.val_old);
    u.perm = pop_global(u.perm); u.keys = pop_global(u.keys); u.step_stats = pop_global(u.step_stats); u.norm_out = pop_global(u.norm_out);
    u.nan_flag = pop_global(u.nan_flag); u.stop_flag = pop_global(u.stop_flag);
    a.obs = pop_global(a.obs); a.actions = pop_global(a.actions); a.adv = pop_global(a.adv); a.ret = pop_global(a.ret); a.logp = pop_global(a.logp);
    gu_update_body<TS>(a, src.lay);
}

// the LDS plan of a net shape at a tile width; total_bytes includes the static words of the kernel
GuLayout gu_layout(const GenericDims& d, int TS) {
    GuLayout L{}; const int TSP = TS + 4;
    L.nl = d.nh + 1;
    int off = 0, flat = 0;
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l < L.nl; ++l) {
            const int I = l == 0 ? d.D : d.H[l - 1], O = l == d.nh ? (n == 0 ? d.A : 1) : d.H[l];
            L.in[l] = I; L.out[n][l] = O; L.op[n][l] = gu_pad4(O);
            L.lw[n][l] = off; off += (I + 1) * gu_pad4(O);
            L.fw[n][l] = flat; flat += (I + 1) * O;
        }
    L.ls = off; off += gu_pad4(d.discrete ? 0 : d.A);
    L.PP = off;
    int p = 0;
    L.x = p; p += gu_pad4(d.D) * TSP;
    for (int l = 0; l < d.nh; ++l) { L.hb[l] = p; p += gu_pad4(d.H[l]) * TSP; }
    const bool need_z = d.act == 6 || d.act == 7;
    for (int l = 0; l < d.nh; ++l) { L.zb[l] = need_z ? p : 0; if (need_z) p += gu_pad4(d.H[l]) * TSP; }
    int hmax = 4; for (int l = 0; l < d.nh; ++l) hmax = std::max(hmax, gu_pad4(d.H[l]));
    L.dz[0] = p; p += hmax * TSP; L.dz[1] = p; p += hmax * TSP;
    L.outb = p; p += 8 * TSP; L.dout = p; p += 8 * TSP; L.actb = p; p += 8 * TSP; L.sc = p; p += 12 * TSP;
    L.total = p;
    return L;
}
size_t gu_lds_bytes(const GuLayout& L) { return sizeof(float) * ((size_t)2 * L.PP + L.total); }
constexpr size_t kGuStaticLds = 64 * 8 + 64 * 4 + 16 + 8 * 8 + 16 * 8;
}  // namespace

int generic_update_tile(const GenericDims& d) {
    for (int TS : {32, 16}) if (gu_lds_bytes(gu_layout(d, TS)) + kGuStaticLds <= kGuLdsMax) return TS;
    return 0;
}
std::string generic_update_unfit(const GenericDims& d, int P) {
    if (d.nh < 1 || d.nh > kMaxHidden) return "the net has " + std::to_string(d.nh) + " hidden layers (the kernel takes 1 to " + std::to_string(kMaxHidden) + ")";
    for (int l = 0; l < d.nh; ++l) if (d.H[l] > kGuMaxWidth) return "hidden width " + std::to_string(d.H[l]) + " is above the kernel's cap of " + std::to_string(kGuMaxWidth) + " units per layer: use narrower layers, or keep the per-step route, which is the default";
    if (d.D > kGuMaxObs) return "observation width " + std::to_string(d.D) + " is above the kernel's cap of " + std::to_string(kGuMaxObs) + ": keep the per-step route, which is the default";
    if (d.A > kGuMaxAct) return "action width " + std::to_string(d.A) + " is above the kernel's cap of " + std::to_string(kGuMaxAct) + ": keep the per-step route, which is the default";
    if (P > kGuMaxParams) return std::to_string(P) + " parameters are above the kernel's cap of " + std::to_string(kGuMaxParams) + " (parameters and gradients both live in the 160 KB of one CU's LDS): use a smaller net, or keep the per-step route, which is the default";
    if (!generic_update_tile(d)) return "the net's parameters, gradients and a 16-sample tile of activations do not fit one CU's LDS: keep the per-step route, which is the default";
    return "";
}

hipError_t launch_ppo_update_generic_small(const GenericDims& d, GenericUpdateArgs a, hipStream_t s) {
    const SmallUpdateArgs& u = a.u;
    const int TS = generic_update_tile(d);
    // host-side preconditions of the kernel: a violated one would be an access out of bounds
    if (!TS || !generic_update_unfit(d, u.P).empty() || u.B < 1 || u.B > 64 || u.nb < 1 || u.nsteps < 0 || u.step0 < 0 || !u.params || !u.adam_m || !u.adam_v || !u.bt || !u.step_stats ||
        !u.stop_flag || !u.nan_flag || !u.keys || !a.obs || !a.actions || !a.adv || !a.ret || !a.logp || !u.val_old) return hipErrorInvalidValue;
    a.lay = gu_layout(d, TS); a.D = d.D; a.A = d.A; a.discrete = d.discrete;
    a.act_code = d.act; a.need_z = (d.act == 6 || d.act == 7) ? 1 : 0;
    const size_t lds = gu_lds_bytes(a.lay);
    if (TS == 32) {
        { hipError_t e = set_max_dynamic_lds((const void*)ppo_update_generic_small_kernel<32>, lds); if (e != hipSuccess) return e; }
        ppo_update_generic_small_kernel<32><<<1, kGuThreads, lds, s>>>(a);
    } else {
        { hipError_t e = set_max_dynamic_lds((const void*)ppo_update_generic_small_kernel<16>, lds); if (e != hipSuccess) return e; }
        ppo_update_generic_small_kernel<16><<<1, kGuThreads, lds, s>>>(a);
    }
    return hipGetLastError();
}

// n members in one launch: h_members (host copies of the blocks at d_members, as the caller filled them; lay, D .. need_z are set HERE in both, so call before the copy
// to the device) are checked like a solo launch's block; GenericDims is equal across the members, and with it the tile width and the LDS plan
hipError_t prepare_ppo_update_generic_small_pop(const GenericDims& d, GenericUpdateArgs* h_members, int n) {
    const int TS = generic_update_tile(d);
    if (!TS || n < 1 || !h_members) return hipErrorInvalidValue;
    const GuLayout lay = gu_layout(d, TS);
    for (int m = 0; m < n; ++m) {
        GenericUpdateArgs& a = h_members[m]; const SmallUpdateArgs& u = a.u;
        if (!generic_update_unfit(d, u.P).empty() || u.B < 1 || u.B > 64 || u.nb < 1 || u.nsteps < 0 || u.step0 < 0 || !u.params || !u.adam_m || !u.adam_v || !u.bt || !u.step_stats ||
            !u.stop_flag || !u.nan_flag || !u.keys || !a.obs || !a.actions || !a.adv || !a.ret || !a.logp || !u.val_old) return hipErrorInvalidValue;
        a.lay = lay; a.D = d.D; a.A = d.A; a.discrete = d.discrete; a.act_code = d.act; a.need_z = (d.act == 6 || d.act == 7) ? 1 : 0;
    }
    return hipSuccess;
}
hipError_t launch_ppo_update_generic_small_pop(const GenericDims& d, const GenericUpdateArgs* d_members, int n, hipStream_t s) {
    const int TS = generic_update_tile(d);
    if (!TS || n < 1 || !d_members) return hipErrorInvalidValue;
    const size_t lds = gu_lds_bytes(gu_layout(d, TS));
    if (TS == 32) {
        { hipError_t e = set_max_dynamic_lds((const void*)ppo_update_generic_small_pop_kernel<32>, lds); if (e != hipSuccess) return e; }
        ppo_update_generic_small_pop_kernel<32><<<n, kGuThreads, lds, s>>>(d_members, n);
    } else {
        { hipError_t e = set_max_dynamic_lds((const void*)ppo_update_generic_small_pop_kernel<16>, lds); if (e != hipSuccess) return e; }
        ppo_update_generic_small_pop_kernel<16><<<n, kGuThreads, lds, s>>>(d_members, n);
    }
    return hipGetLastError();
}

}  // namespace dril
