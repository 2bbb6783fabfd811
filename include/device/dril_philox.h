// dril_philox.h — the library's counter RNG and its conversions, in ONE place: included by dril_device.h (every kernel of libdril_hip.so) and by
// device/dril_env_plugin.h (a user's device env compiled on its own), so an env inside the library and the same env in a plug-in draw the same words.
// Philox4x32-10 is the published generator (Salmon et al., SC'11); oracle/dril_oracle.c restates it independently.
// Compiles under hipcc (host + device) and under a plain C++ compiler (DRIL_ENV_PLUGIN_HOST builds of a plug-in: no HIP headers needed).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define DRIL_PHILOX_HD __host__ __device__
#define DRIL_PHILOX_D __device__
#else
#include <math.h>
#define DRIL_PHILOX_HD
#define DRIL_PHILOX_D
#endif
namespace dril {

DRIL_PHILOX_HD inline void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                         uint32_t c3, uint32_t out[4]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
DRIL_PHILOX_HD inline float u01_f32(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }
DRIL_PHILOX_HD inline double u01_f64(uint32_t hi, uint32_t lo) {
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}
DRIL_PHILOX_D inline float randn_f32(uint32_t a, uint32_t b) {
    const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

}  // namespace dril
