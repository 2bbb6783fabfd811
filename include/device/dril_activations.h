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

// the derivatives the reverse pass multiplies with, by the same codes.  tanh, relu, sigmoid, elu, leakyrelu and softplus are functions of the activation's OUTPUT y;
// gelu and swish need the pre-activation x (activation_grad_reads_preactivation): `u` is whichever of the two the activation asks for.  The formulas are those of the
// masked epilogues of dril_gemm.hip.
DRIL_DEVICE_FN bool activation_grad_reads_preactivation(int act) { return act == 6 || act == 7; }
DRIL_DEVICE_FN float activation_grad(int act, float u) {
    switch (act) {
        case 1: return u > 0.f ? 1.0f : 0.f;
        case 2: return u * (1.0f - u);
        case 3: return u > 0.f ? 1.0f : u + 1.0f;                                    // alpha e^x = elu(x) + alpha
        case 4: return u > 0.f ? 1.0f : 0.01f;
        case 5: return -expm1f(-u);                                                  // sigmoid(x) = 1 - e^(-softplus(x))
        case 6: {
            const float w = 0.7978845608028654f * (u + 0.044715f * u * u * u), t = tanhf(w);
            return 0.5f * (1.0f + t) + 0.5f * u * (1.0f - t * t) * 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * u * u);
        }
        case 7: { const float sg = 1.0f / (1.0f + expf(-u)); return sg * (1.0f + u * (1.0f - sg)); }
        default: return 1.0f - u * u;
    }
}

}  // namespace dril
