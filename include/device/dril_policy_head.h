// dril_policy_head.h — the sampling head of the on-policy collection, in ONE place: the action noise of a device env (Philox stream 1 of the table in
// dril_device.h) and the per-sample Categorical / DiagGaussian arithmetic at a runtime action width.  generic_policy_head_kernel and the loss head of
// dril_generic.hip (the step-granular path) and the fused rollout of a device env plug-in (device/dril_env_rollout.h, compiled into the plug-in's own code object)
// expand these lines.  Accurate libm (expf / logf), like the oracle.  `zs` / `ms`: the stride between the components of a logit / mean row (1: a row-major row; the
// tile width: a column of an activation panel).
// Compiles under hipcc and under a plain C++ compiler (DRIL_ENV_PLUGIN_HOST builds of a plug-in: no HIP headers needed).
#pragma once
#include <stdint.h>

#include "dril_activations.h"   // DRIL_DEVICE_FN
#include "dril_philox.h"

namespace dril {

// ---- the action noise of a device env at its global step (stream 1): the same draw on every collection path ----
DRIL_DEVICE_FN double env_noise_u01(uint64_t env_seed, uint32_t gstep) {                      // Categorical: the uniform of the inverse-CDF draw
    uint32_t r[4]; philox4x32_10((uint32_t)env_seed, (uint32_t)(env_seed >> 32), gstep, 0, 1, 0, r);
    return u01_f64(r[0], r[1]);
}
DRIL_DEVICE_FN float env_noise_randn(uint64_t env_seed, uint32_t gstep, int i) {              // DiagGaussian: the standard normal of action component i (two per block)
    uint32_t r[4]; philox4x32_10((uint32_t)env_seed, (uint32_t)(env_seed >> 32), gstep, 0, 1, (uint32_t)(i / 2), r);
    return (i & 1) ? randn_f32(r[2], r[3]) : randn_f32(r[0], r[1]);
}

// ---- per-sample distribution math (runtime action width) ----
constexpr float kLog2PiG = 1.8378770664093453f;
// Lux.softmax statistics of one logit row: max and sum(exp(z - max)); p_i = exp(z_i - m) / s (layer_forward.jl:141-149)
DRIL_DEVICE_FN void softmax_stats(const float* z, int A, float& m, float& s, int zs = 1) {
    m = z[0]; for (int i = 1; i < A; ++i) m = fmaxf(m, z[i * zs]);
    s = 0.f; for (int i = 0; i < A; ++i) s += expf(z[i * zs] - m);
}
// rand(d): findfirst(cumsum(p) .>= u), categorical.jl:47-52
DRIL_DEVICE_FN int categorical_draw(const float* z, int A, float m, float s, double u, int zs = 1) {
    float cs = 0.f; int act = A - 1;
    for (int k = 0; k < A; ++k) { cs += expf(z[k * zs] - m) / s; if ((double)cs >= u) { act = k; break; } }
    return act;
}
DRIL_DEVICE_FN float categorical_logp(const float* z, int act, float m, float s, int zs = 1) { return logf(expf(z[act * zs] - m) / s); }
DRIL_DEVICE_FN float categorical_entropy_rt(const float* z, int A, float m, float s) {        // -sum(p log p), categorical.jl:38-40
    float e = 0.f; for (int i = 0; i < A; ++i) { const float p = expf(z[i] - m) / s; e += p * logf(p); }
    return -e;
}
// rand(d) = mean + exp(log_std) * N(0, 1), diagGaussian.jl:13-17
DRIL_DEVICE_FN float gauss_draw(float mu, float log_std, float n01) { return mu + expf(log_std) * n01; }
DRIL_DEVICE_FN float gauss_logpdf_rt(const float* x, const float* mu, const float* ls, int A, int ms = 1) {   // diagGaussian.jl:25-36
    float lss = 0.f, dss = 0.f;
    for (int i = 0; i < A; ++i) { lss += ls[i]; const float d = x[i] - mu[i * ms]; dss += d * d * expf(-2.0f * ls[i]); }
    return -0.5f * (2.0f * lss + dss + (float)A * kLog2PiG);
}
DRIL_DEVICE_FN float gauss_entropy_rt(const float* ls, int A) {                                 // diagGaussian.jl:38-43
    float lss = 0.f; for (int i = 0; i < A; ++i) lss += ls[i];
    return 0.5f * (float)A * (1.0f + kLog2PiG) + lss;
}

}  // namespace dril
