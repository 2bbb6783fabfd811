// reacher3_plugin.hip — an env the built-in kinds cannot express (three action dims, twelve observation dims): a unit point mass in 3-D, pushed by the action
// towards a target that is drawn anew for every episode.
//   state  S = 9 : position p, velocity v, target g
//   obs    D = 12: p, v, g, p - g
//   action A = 3 : force in Box(-1, 1)^3
//   step         : v <- (v + dt a) * damping;  p <- p + dt v;  reward = -|p - g|^2 - 0.01 |a|^2;  terminated when |p_i| > 2 for some i;  time limit 100
// The arithmetic is + - * only, every product and sum written as its own statement on purpose: tests/test_env_plugin.py follows it with a NumPy float32 twin.
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/reacher3_plugin.hip -o examples/envs/reacher3_plugin.hsaco
#include "device/dril_env_plugin.h"

struct Reacher3 {
    static constexpr int S = 9, D = 12, A = 3;
    static constexpr bool discrete = false;
    static constexpr int episode_len = 100;
    static constexpr float action_low[A] = {-1.0f, -1.0f, -1.0f}, action_high[A] = {1.0f, 1.0f, 1.0f};
    // observation space: |p_i| <= 2 + one move while the episode lasts (a step past 2 terminates; |move| <= dt |v|), |v_i| < dt damping / (1 - damping) = 1.9,
    // |g_i| <= 1, |p_i - g_i| <= 3.2
    static constexpr float obs_low[D] = {-2.2f, -2.2f, -2.2f, -2.0f, -2.0f, -2.0f, -1.0f, -1.0f, -1.0f, -3.2f, -3.2f, -3.2f};
    static constexpr float obs_high[D] = {2.2f, 2.2f, 2.2f, 2.0f, 2.0f, 2.0f, 1.0f, 1.0f, 1.0f, 3.2f, 3.2f, 3.2f};
    static constexpr const char* name = "Reacher3";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) {                 // p ~ U(-0.5, 0.5)^3 (block 0), v = 0, g ~ U(-1, 1)^3 (block 1)
        const DrilEnvWords r0 = rng.words(0), r1 = rng.words(1);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            st[i] = DrilEnvRng::u01(r0.w[i]) - 0.5f;
            st[3 + i] = 0.0f;
            const float u2 = DrilEnvRng::u01(r1.w[i]) * 2.0f;
            st[6 + i] = u2 - 1.0f;
        }
    }
    DRIL_ENV_FN static void observe(const float* st, float* obs) {
#pragma unroll
        for (int i = 0; i < 9; ++i) obs[i] = st[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) obs[9 + i] = st[i] - st[6 + i];
    }
    DRIL_ENV_FN static float step(float* st, const float* act_f, int act_i, bool* terminated) {
        const float dt = 0.1f, damping = 0.95f;
        float dist2 = 0.0f, act2 = 0.0f; bool out = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float push = dt * act_f[i];
            const float v = (st[3 + i] + push) * damping;
            const float move = dt * v;
            const float p = st[i] + move;
            st[i] = p; st[3 + i] = v;
            const float d = p - st[6 + i];
            const float dd = d * d;
            dist2 = dist2 + dd;
            const float aa = act_f[i] * act_f[i];
            act2 = act2 + aa;
            out = out || (p < -2.0f) || (p > 2.0f);
        }
        *terminated = out;
        const float pen = 0.01f * act2;
        return -dist2 - pen;
    }
};
DRIL_ENV_PLUGIN(Reacher3)
