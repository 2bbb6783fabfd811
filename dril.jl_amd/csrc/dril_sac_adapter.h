// dril_sac_adapter.h — TanhScaleAdapter on a Box with per-dimension bounds (default_adapters.jl:13-30) and rand(action_space): the ONE definition behind
// sac_collect_action (dril_sac_device.h) and sac_squash_eval_kernel (dril_sac.hip).  Plain float arithmetic with no HIP dependency, so the same lines compile with a host C++
// compiler (tests/test_sac_env_plugin.py builds them with g++ and follows them with NumPy).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DRIL_SAC_FN __host__ __device__ inline
#else
#define DRIL_SAC_FN inline
#endif

namespace dril {
// scale_to_space(t, space), t in [-1, 1]: low + (t + 1) (high - low) / 2, in the operation order the scalar-bounds kernels have always used
DRIL_SAC_FN float sac_scale_to_space(float t, float low, float high) { return t * (high - low) / 2.0f + (low + high) / 2.0f; }
// to_env(TanhScaleAdapter, raw, space): the adapter squashes again, as the reference has it
DRIL_SAC_FN float sac_to_env(float raw, float low, float high) { return sac_scale_to_space(tanhf(raw), low, high); }
// from_env(TanhScaleAdapter, action, space): an env action in [low, high] back to [-1, 1] (the inverse of scale_to_space; needs low < high)
DRIL_SAC_FN float sac_from_env(float action, float low, float high) { return 2.0f * (action - (low + high) / 2.0f) / (high - low); }
// rand(rng, Box) of one dimension from a uniform u in [0, 1)
DRIL_SAC_FN float sac_rand_box(float u, float low, float high) { return low + u * (high - low); }
}  // namespace dril
