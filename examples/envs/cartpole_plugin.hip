// cartpole_plugin.hip — CartPole-v1 as a device env plug-in: a TWIN of the built-in DRIL_ENV_CARTPOLE (env_reset<0> / env_obs<0> / env_step<0> of
// dril.jl_amd/csrc/dril_device.h, restated with the same f32 operation order and the same use of the reset words), so that the plug-in seam can be
// tested to the bit against an env the CPU oracle already pins.
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/cartpole_plugin.hip -o examples/envs/cartpole_plugin.hsaco
#include "device/dril_env_plugin.h"

struct CartPolePlugin {
    static constexpr int S = 4, D = 4, A = 2;
    static constexpr bool discrete = true;
    static constexpr int episode_len = 500;
    // Gymnasium's observation space: twice the termination thresholds for x and theta, unbounded velocities (so ScalingWrapperEnv cannot wrap it, and as a
    // Discrete env it could not anyway)
    static constexpr float obs_low[D] = {-4.8f, -INFINITY, -0.41887903f, -INFINITY}, obs_high[D] = {4.8f, INFINITY, 0.41887903f, INFINITY};
    static constexpr const char* name = "CartPole-v1 (plug-in)";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) {                 // U(-0.05, 0.05)^4 from the four words of block 0
        const DrilEnvWords r = rng.words(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) st[i] = DrilEnvRng::u01(r.w[i]) * 0.1f - 0.05f;
    }
    DRIL_ENV_FN static void observe(const float* st, float* obs) {
#pragma unroll
        for (int i = 0; i < 4; ++i) obs[i] = st[i];
    }
    DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated) {
        const float gravity = 9.8f, masspole = 0.1f, total_mass = 1.1f, length = 0.5f;
        const float polemass_length = 0.05f, force_mag = 10.0f, tau = 0.02f;
        float x = st[0], x_dot = st[1], th = st[2], th_dot = st[3];
        const float force = act_i == 1 ? force_mag : -force_mag;
        const float c = cosf(th), s = sinf(th);
        const float temp = (force + polemass_length * th_dot * th_dot * s) / total_mass;
        const float thacc = (gravity * s - c * temp) / (length * (4.0f / 3.0f - masspole * c * c / total_mass));
        const float xacc = temp - polemass_length * thacc * c / total_mass;
        x = x + tau * x_dot; x_dot = x_dot + tau * xacc;
        th = th + tau * th_dot; th_dot = th_dot + tau * thacc;
        st[0] = x; st[1] = x_dot; st[2] = th; st[3] = th_dot;
        *terminated = (x < -2.4f) || (x > 2.4f) || (th < -0.20943951023931953f) || (th > 0.20943951023931953f);
        return 1.0f;
    }
};
DRIL_ENV_PLUGIN(CartPolePlugin)
