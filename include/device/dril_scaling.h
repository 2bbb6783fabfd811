// dril_scaling.h — the two affine maps of ScalingWrapperEnv (scalingWrapperEnv.jl), in ONE place: included by dril_device.h (the built-in scaled kinds,
// DRIL_ENV_PENDULUM_SCALED / DRIL_ENV_MOUNTAINCAR_CONTINUOUS_SCALED) and by device/dril_env_plugin.h (the _scaled kernels of a device env plug-in), so a plug-in
// under the wrapper and a built-in scaled kind evaluate the same float operations in the same order.
// Compiles under hipcc (host + device) and under a plain C++ compiler (DRIL_ENV_PLUGIN_HOST builds of a plug-in).
#pragma once
#if defined(__HIPCC__)
#define DRIL_SCALING_HD __host__ __device__
#else
#define DRIL_SCALING_HD
#endif
namespace dril {
// scale! :71-74 `(x - low) * sf - 1`, unscale! :76-79 `(x + 1) / sf + low`, sf = 2 / (high - low) :36-44
DRIL_SCALING_HD inline float scale_to_unit(float x, float low, float high) { const float sf = 2.0f / (high - low); return (x - low) * sf - 1.0f; }
DRIL_SCALING_HD inline float unscale_from_unit(float x, float low, float high) { const float sf = 2.0f / (high - low); return (x + 1.0f) / sf + low; }
}  // namespace dril
