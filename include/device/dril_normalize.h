// dril_normalize.h — normalize_obs! of NormalizeWrapperEnv (normalizeWrapperEnv.jl:174-179) per element, in ONE place: the library's wrapper kernels
// (dril_norm_wrap.h: nz_obs) and the evaluation kernel of a device env plug-in (device/dril_env_evaluate.h, compiled into the plug-in's own code object, where the
// statistics are frozen and only read) expand this line.  Compiles under hipcc and under a plain C++ compiler (DRIL_ENV_PLUGIN_HOST builds, CPU tests).
#pragma once
#include "dril_activations.h"   // DRIL_DEVICE_FN

namespace dril {
DRIL_DEVICE_FN float normalize_obs(float v, float mean, float var, float eps, float clip) {
    v = (v - mean) / sqrtf(var + eps);
    return fminf(fmaxf(v, -clip), clip);
}
}  // namespace dril
