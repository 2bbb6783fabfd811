// dril_activations.h — the forward formulas of the eight activations of dril_config.activation, in ONE place: the epilogues of the layer contractions
// (dril_gemm.hip: gemm_epilogue / gemm_epilogue_rare), the one-launch deployment actor (dril_policy.hip: policy_act_kernel) and the fused rollout of a device env
// plug-in (device/dril_env_rollout.h, compiled into the plug-in's own code object) all expand these lines.
// NNlib's definitions: sigmoid, elu (alpha = 1), leakyrelu (a = 0.01), softplus, gelu (the tanh form), swish; relu keeps a NaN (relu_nan, dril_device.h).
// Compiles under hipcc and under a plain C++ compiler (DRIL_ENV_PLUGIN_HOST builds of a plug-in: no HIP headers needed).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DRIL_DEVICE_FN __device__ __forceinline__
#else
#include <math.h>
#define DRIL_DEVICE_FN inline
#endif

namespace dril {

DRIL_DEVICE_FN float act_relu(float v) { return (v > 0.f || v != v) ? v : 0.f; }
DRIL_DEVICE_FN float act_tanh(float v) { return tanhf(v); }
DRIL_DEVICE_FN float act_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
DRIL_DEVICE_FN float act_elu(float v) { return v > 0.f ? v : expm1f(v); }
DRIL_DEVICE_FN float act_leakyrelu(float v) { return v > 0.f ? v : 0.01f * v; }
DRIL_DEVICE_FN float act_softplus(float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }
DRIL_DEVICE_FN float act_gelu(float v) { const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v); return 0.5f * v * (1.0f + tanhf(u)); }
DRIL_DEVICE_FN float act_swish(float v) { return v / (1.0f + expf(-v)); }

// by the code of dril_config.activation: 0 tanh, 1 relu, 2 sigmoid, 3 elu, 4 leakyrelu, 5 softplus, 6 gelu, 7 swish
DRIL_DEVICE_FN float activation_forward(int act, float v) {
    switch (act) {
        case 1: return act_relu(v);
        case 2: return act_sigmoid(v);
        case 3: return act_elu(v);
        case 4: return act_leakyrelu(v);
        case 5: return act_softplus(v);
        case 6: return act_gelu(v);
        case 7: return act_swish(v);
        default: return act_tanh(v);
    }
}

}  // namespace dril
