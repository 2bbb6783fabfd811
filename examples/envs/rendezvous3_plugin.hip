// rendezvous3_plugin.hip — a WORLD (include/device/dril_env_world.h): three point agents in the plane that share one state and are rewarded for meeting.  One shared
// policy acts for all three; the library sees agent i of world w as row 3 w + i.
//   state  S = 12: per agent i the four floats at 4 i: position p (2), velocity v (2)
//   obs    D = 8 : own p, own v, position of the next agent minus own, position of the agent after that minus own ("next": (i + 1) % 3, (i + 2) % 3)
//   action A = 2 : force in Box(-1, 1)^2, per agent
//   step         : v <- (v + 0.1 a) * 0.95;  p <- p + 0.1 v, for every agent; then
//                  reward_i = -(mean over the two others of the squared distance) - 0.01 |a_i|^2;  the world terminates when some |p| > 3;  time limit 50
//   reset        : p ~ U(-3, 3)^2 and v ~ U(-1, 1)^2 per agent (blocks 0..2 of the world's stream): some agents start on their way out of the arena
// The arithmetic is + - * only, every product and sum written as its own statement on purpose: tests/test_env_world.py follows it with a NumPy float32 twin.
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/rendezvous3_plugin.hip -o examples/envs/rendezvous3_plugin.hsaco
#include "device/dril_env_world.h"

struct Rendezvous3 {
    static constexpr int N = 3;
    static constexpr int S = 12, D = 8, A = 2;
    static constexpr bool discrete = false;
    static constexpr int episode_len = 50;
    static constexpr float action_low[A] = {-1.0f, -1.0f}, action_high[A] = {1.0f, 1.0f};
    static constexpr const char* name = "Rendezvous3";
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) {                 // agent i draws from block i: words 0, 1 -> p, words 2, 3 -> v
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const DrilEnvWords r = rng.words((uint32_t)i);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float centred = DrilEnvRng::u01(r.w[k]) - 0.5f;                 // (exact, and a product with no sum after it: the same bits with or without FMA contraction)
                st[4 * i + k] = centred * 6.0f;
                const float uv = DrilEnvRng::u01(r.w[2 + k]) * 2.0f;
                st[4 * i + 2 + k] = uv - 1.0f;
            }
        }
    }
    DRIL_ENV_FN static void observe(const float* st, int agent, float* obs) {
        const int j = agent + 1 < N ? agent + 1 : agent + 1 - N, k = agent + 2 < N ? agent + 2 : agent + 2 - N;
#pragma unroll
        for (int c = 0; c < 4; ++c) obs[c] = st[4 * agent + c];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            obs[4 + c] = st[4 * j + c] - st[4 * agent + c];
            obs[6 + c] = st[4 * k + c] - st[4 * agent + c];
        }
    }
    DRIL_ENV_FN static void step(float* st, const float* act_f, const int* act_i, float* rew, bool* terminated) {
        const float dt = 0.1f, damping = 0.95f;
        bool out = false;
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float push = dt * act_f[2 * i + c];
                const float v = (st[4 * i + 2 + c] + push) * damping;
                const float move = dt * v;
                const float p = st[4 * i + c] + move;
                st[4 * i + c] = p; st[4 * i + 2 + c] = v;
                out = out || (p < -3.0f) || (p > 3.0f);
            }
        }
        float d2[N];                                                                  // d2[i]: squared distance between agents i and (i + 1) % 3
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int j = i + 1 < N ? i + 1 : 0;
            const float dx = st[4 * j] - st[4 * i];
            const float dy = st[4 * j + 1] - st[4 * i + 1];
            const float xx = dx * dx;
            const float yy = dy * dy;
            d2[i] = xx + yy;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int h = i > 0 ? i - 1 : N - 1;                                      // the pair (h, i) is d2[h], the pair (i, i + 1) is d2[i]
            const float sum = d2[i] + d2[h];
            const float mean = sum * 0.5f;
            const float ax = act_f[2 * i] * act_f[2 * i];
            const float ay = act_f[2 * i + 1] * act_f[2 * i + 1];
            const float act2 = ax + ay;
            const float pen = 0.01f * act2;
            rew[i] = -mean - pen;
        }
        *terminated = out;
    }
};
DRIL_ENV_PLUGIN_WORLD(Rendezvous3)
