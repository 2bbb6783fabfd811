// pendulum_plugin.hip — Pendulum-v1 as a device env plug-in: a TWIN of the built-in DRIL_ENV_PENDULUM (env_reset<1> / env_obs<1> / env_step<1> of
// dril.jl_amd/csrc/dril_device.h, same f32 operation order, same reset words).  The Box(-2, 2) bound is the ClampAdapter of the wrapper; the physics
// clamps again exactly as the built-in does.
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/pendulum_plugin.hip -o examples/envs/pendulum_plugin.hsaco
#include "device/dril_env_plugin.h"

struct PendulumPlugin {
    static constexpr int S = 2, D = 3, A = 1;
    static constexpr bool discrete = false;
    static constexpr int episode_len = 200;
    static constexpr float action_low[A] = {-2.0f}, action_high[A] = {2.0f};
    static constexpr float obs_low[D] = {-1.0f, -1.0f, -8.0f}, obs_high[D] = {1.0f, 1.0f, 8.0f};   // Gymnasium's Box: (cos, sin, theta_dot clipped to max_speed)
    static constexpr const char* name = "Pendulum-v1 (plug-in)";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) {                 // theta ~ U(-pi, pi), theta_dot ~ U(-1, 1)
        const DrilEnvWords r = rng.words(0);
        st[0] = DrilEnvRng::u01(r.w[0]) * 6.28318530717958647692f - 3.14159265358979323846f;
        st[1] = DrilEnvRng::u01(r.w[1]) * 2.0f - 1.0f;
    }
    DRIL_ENV_FN static void observe(const float* st, float* obs) { obs[0] = cosf(st[0]); obs[1] = sinf(st[0]); obs[2] = st[1]; }
    DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated) {
        const float max_speed = 8.0f, max_torque = 2.0f, dt = 0.05f, g = 10.0f, m = 1.0f, l = 1.0f;
        const float pi = 3.14159265358979323846f;
        const float th = st[0], thdot = st[1];
        const float u = fminf(fmaxf(act_f[0], -max_torque), max_torque);
        float an = fmodf(th + pi, 2.0f * pi); if (an < 0) an += 2.0f * pi; an -= pi;
        const float cost = an * an + 0.1f * thdot * thdot + 0.001f * u * u;
        float nthdot = thdot + (3.0f * g / (2.0f * l) * sinf(th) + 3.0f / (m * l * l) * u) * dt;
        nthdot = fminf(fmaxf(nthdot, -max_speed), max_speed);
        st[0] = th + nthdot * dt; st[1] = nthdot;
        *terminated = false;
        return -cost;
    }
};
DRIL_ENV_PLUGIN(PendulumPlugin)
