// dril_ppo_head.h — the PPO loss of ONE sample at a runtime action width (ppo.jl:377-404), in one place: generic_loss_head_kernel (dril_generic.hip, one launch per
// optimiser step) and ppo_update_generic_small_kernel (dril_update_generic_small.hip, every optimiser step of an update in one launch) expand these lines.
// Accurate libm (expf / logf), like the oracle.  Strides: `os` between the components of a logit / mean row, `xs` between the components of a Box action, `ds`
// between the components of the gradient row (1: a row-major row; the tile's row stride: a column of an activation panel).
#pragma once
#include "dril_internal.h"

namespace dril {

// value head: dLoss/dV of the sample; ve2 = (V_clipped - R)^2 (ppo.jl:344-346,378,385)
__device__ __forceinline__ float ppo_value_sample(const GradArgs& a, bool valid, float R, float ov, float val, float& ve2) {
    const float dcl = val - ov;
    const bool vpass = !a.has_clip_vf || (dcl >= -a.clip_range_vf && dcl <= a.clip_range_vf);                  // clip_range, ppo.jl:344-346,378
    const float value = a.has_clip_vf ? ov + fminf(fmaxf(dcl, -a.clip_range_vf), a.clip_range_vf) : val;
    const float ve = value - R;
    ve2 = ve * ve;
    return (valid && vpass) ? a.invB * a.vf_coef * 2.0f * ve : 0.f;
}

// policy head: dLoss/d(actor out) into d_o, dLoss/dlogp returned in dlogp; st = {-min term, entropy, clipped, kl term, ratio} of the sample (:382,:383,:390,:393,:402).
// act_i: the sample's Categorical action as stored (action_start-based); x: its Box action
__device__ __forceinline__ void ppo_policy_sample(const GradArgs& a, int A, int discrete, bool valid, const float* o, int os, int act_i, const float* x, int xs,
                                                  float advn, float lpo, const float* ls, float* d_o, int ds, float& dlogp_out, float (&st)[5]) {
    float logp, ent, m = 0.f, s = 1.f; int act = 0;
    if (discrete) {
        softmax_stats(o, A, m, s, os);
        act = act_i - a.action_start; act = act < 0 ? 0 : (act >= A ? A - 1 : act);
        logp = logf(expf(o[act * os] - m) / s);
        float e = 0.f; for (int i = 0; i < A; ++i) { const float p = expf(o[i * os] - m) / s; e += p * logf(p); }      // categorical_entropy_rt at a stride
        ent = -e;
    } else {
        float lss = 0.f, dss = 0.f;                                                                               // gauss_logpdf_rt at two strides
        for (int i = 0; i < A; ++i) { lss += ls[i]; const float d = x[i * xs] - o[i * os]; dss += d * d * expf(-2.0f * ls[i]); }
        logp = -0.5f * (2.0f * lss + dss + (float)A * kLog2PiG);
        ent = gauss_entropy_rt(ls, A);
    }
    const float lr = logp - lpo;
    const float r = expf(lr);                                                     // :380
    const float lo = 1.0f - a.clip_range, hi = 1.0f + a.clip_range;
    const float rc = fminf(fmaxf(r, lo), hi);                                     // :381
    const float t1 = r * advn, t2 = rc * advn;
    const float mn = t2 < t1 ? t2 : t1;                                           // :382
    const float dm_dr = (t2 < t1) ? ((r >= lo && r <= hi) ? advn : 0.f) : advn;
    const float dlogp = valid ? -a.invB * dm_dr * r : 0.f;
    const float dent = valid ? -a.invB * a.ent_coef : 0.f;                        // ent_loss = -mean(entropy), :383,:386
    dlogp_out = dlogp;
    if (discrete) {
        for (int k = 0; k < A; ++k) { const float p = expf(o[k * os] - m) / s; d_o[k * ds] = dlogp * ((k == act ? 1.0f : 0.0f) - p) + dent * (-p * (logf(p) + ent)); }
    } else {
        for (int k = 0; k < A; ++k) { const float iv = expf(-2.0f * ls[k]), d = x[k * xs] - o[k * os]; d_o[k * ds] = dlogp * d * iv; }
    }
    st[0] = -mn; st[1] = ent; st[2] = (r != rc) ? 1.0f : 0.0f; st[3] = (r - 1.0f) - lr; st[4] = r;
}
// one sample's term of dLoss/dlog_std_k (DiagGaussian): dlogp (d^2 exp(-2 ls) - 1) + dent
__device__ __forceinline__ float ppo_log_std_term(const GradArgs& a, float dlogp, float xk, float ok, float iv) {
    const float d = xk - ok, dent = -a.invB * a.ent_coef;
    return dlogp * (d * d * iv - 1.0f) + dent;
}

}  // namespace dril
