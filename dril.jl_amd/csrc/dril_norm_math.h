// dril_norm_math.h — the two scalar definitions of NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) that every general-width wrapper kernel
// shares: the SAC handle's (dril_sac_norm.h) and the PPO handle's on device env plug-ins (dril_ppo_norm.h).  Included inside the including file's namespace.
#pragma once

constexpr int kNzMaxD = 1024;                    // the widest observation the wrapper takes (DRIL_ENV_PLUGIN_MAX_D); sizes the SAC apply kernel's LDS

// update_from_moments! (normalizeWrapperEnv.jl:28-50) in the reference's float32 arithmetic — the arithmetic of rms_merge (dril_kernels.hip)
__device__ __forceinline__ void nz_merge(float& mean, float& var, long long count, float bmean, float bvar, long long bcount) {
    if (count == 0) { mean = bmean; var = bvar; return; }
    const long long tot = count + bcount;
    const float delta = bmean - mean;
    const float new_mean = mean + delta * (float)bcount / (float)tot;
    const float m_a = var * (float)count, m_b = bvar * (float)bcount;
    const float M2 = m_a + m_b + delta * delta * (float)count * (float)bcount / (float)tot;
    mean = new_mean; var = M2 / (float)tot;
}
// normalize_obs! (:174-179)
__device__ __forceinline__ float nz_obs(float v, float mean, float var, float eps, float clip) {
    v = (v - mean) / sqrtf(var + eps);
    return fminf(fmaxf(v, -clip), clip);
}
