// dril_ext_device.hip — the small kernels of the device-array verbs on a DRIL_ENV_EXTERNAL handle (dril_ext_act_device / dril_ext_record_device /
// dril_predict_actions_device, include/dril_hip.h): what the host verbs do with host loops between a copy and a drain, done where the data already is.
//   ext_actions_out_kernel   row t of the action buffer -> the caller's raw actions and, through the ClampAdapter (default_adapters.jl:4-11), its env actions
//   ext_record_kernel        the caller's rewards / terminated / truncated -> rew[t], flags[t], boot[t] (trajectory.jl:52-61)
// Both are one element per thread and bound by launch latency (E x A <= a few MB); the policy forward between them is generic_policy.
// With NormalizeWrapperEnv / MonitorWrapperEnv on the handle (dril_ext_normalize_enable / dril_ext_monitor_enable) ext_norm_record_kernel stands where ext_record_kernel
// stands here: dril_ext_norm.h, compiled into dril_wrap.hip next to the normaliser core it shares with the plug-in wrapper.
#include "dril_internal.h"

namespace dril {

namespace {

struct ExtActionsOutArgs { const uint32_t* act; uint32_t* raw; float* env; int64_t n; int A, clamp; ExtBounds b; };

// n = E actions (Discrete: i32 words, DiscreteAdapter is the identity, default_adapters.jl:34-38) or E x A floats (Box)
__global__ __launch_bounds__(256) void ext_actions_out_kernel(ExtActionsOutArgs g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t w = g.act[i];
    if (g.raw) g.raw[i] = w;
    if (!g.env) return;
    float a = __uint_as_float(w);
    if (g.clamp) {
        const int k = (int)(i % g.A);
        const float lo = g.b.lo[k], hi = g.b.hi[k];
        if (lo < hi) a = a < lo ? lo : (a > hi ? hi : a);                              // low >= high: this dimension is not clamped (the host verb's rule)
    }
    g.env[i] = a;                                                                      // Discrete: the same 32 bits
}

// one thread per env.  v_all: V(terminal_obs) of ALL E columns (null: the caller passed no terminal_obs); kept where the env was truncated, 0 elsewhere
__global__ __launch_bounds__(256) void ext_record_kernel(int E, const float* rewards, const uint8_t* terminated, const uint8_t* truncated, const float* v_all,
                                                         float* rew, uint8_t* flags, float* boot, int* err) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const bool te = terminated[e] != 0, tr = truncated[e] != 0;
    rew[e] = rewards[e];
    flags[e] = (uint8_t)((te ? 1 : 0) | (tr ? 2 : 0));
    boot[e] = (tr && v_all) ? v_all[e] : 0.f;
    if (tr && !v_all) *err = 1;                                                        // sticky: dril_ext_finish_device reads it after its drain
}

}  // namespace

hipError_t launch_ext_actions_out(const void* act, void* raw, void* env, int64_t E, int A, int discrete, const ExtBounds* bounds, hipStream_t s) {
    ExtActionsOutArgs g{};
    g.act = (const uint32_t*)act; g.raw = (uint32_t*)raw; g.env = (float*)env; g.n = discrete ? E : E * (int64_t)A; g.A = A;
    g.clamp = (!discrete && bounds) ? 1 : 0;
    if (g.clamp) g.b = *bounds;
    if (g.n < 1) return hipSuccess;
    ext_actions_out_kernel<<<(unsigned)((g.n + 255) / 256), 256, 0, s>>>(g);
    return hipGetLastError();
}

hipError_t launch_ext_record(int E, const float* rewards, const uint8_t* terminated, const uint8_t* truncated, const float* v_all,
                             float* rew, uint8_t* flags, float* boot, int* err, hipStream_t s) {
    if (E < 1) return hipSuccess;
    ext_record_kernel<<<(unsigned)((E + 255) / 256), 256, 0, s>>>(E, rewards, terminated, truncated, v_all, rew, flags, boot, err);
    return hipGetLastError();
}

}  // namespace dril
