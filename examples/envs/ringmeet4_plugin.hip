// ringmeet4_plugin.hip — a WORLD (include/device/dril_env_world.h) with a Discrete action space: four agents on a ring of 16 cells that are rewarded for gathering.
// One shared policy acts for all four; the library sees agent i of world w as row 4 w + i.
//   state  S = 4 : the cell of each agent, an integer 0..15 kept in a float
//   obs    D = 5 : sin and cos of the own cell's angle (a table: sixteenths of a turn), then the signed ring offset to the three others ((i + 1) % 4, (i + 2) % 4,
//                  (i + 3) % 4), in -7..8 cells, divided by 8
//   action       : Discrete(3): left / stay / right, per agent
//   step         : every agent moves by -1 / 0 / +1 cell around the ring; then
//                  reward_i = -(sum over the three others of the ring distance) / 8;  the world terminates when all four share a cell;  time limit 40
//   reset        : each cell from the top four bits of a word of block 0 of the world's stream
// The state is integer-valued and the only float arithmetic is a sum of small integers times 0.125, so a NumPy twin follows it exactly (tests/test_env_world.py).
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/ringmeet4_plugin.hip -o examples/envs/ringmeet4_plugin.hsaco
#include "device/dril_env_world.h"

struct RingMeet4 {
    static constexpr int N = 4;
    static constexpr int S = 4, D = 5, A = 3;
    static constexpr bool discrete = true;
    static constexpr int episode_len = 40;
    static constexpr const char* name = "RingMeet4";
    static constexpr int cells = 16;
    // sin(2 pi k / 16), k = 0..15; the cosine is the same table four cells on
    static constexpr float sine[cells] = {0.0f, 0.382683432f, 0.707106781f, 0.923879533f, 1.0f, 0.923879533f, 0.707106781f, 0.382683432f,
                                          0.0f, -0.382683432f, -0.707106781f, -0.923879533f, -1.0f, -0.923879533f, -0.707106781f, -0.382683432f};
    DRIL_ENV_FN static float table(int k) {                                            // (a chain of selects: no table in memory, on the device or the host)
        float v = sine[0];
#pragma unroll
        for (int i = 1; i < cells; ++i) v = k == i ? sine[i] : v;
        return v;
    }
    // the signed offset from cell `from` to cell `to` the short way round: -7..8
    DRIL_ENV_FN static int offset(int from, int to) {
        const int d = (to - from + cells) % cells;
        return d > cells / 2 ? d - cells : d;
    }
    DRIL_ENV_FN static void reset(const DrilEnvRng& rng, float* st) {
        const DrilEnvWords r = rng.words(0);
#pragma unroll
        for (int i = 0; i < N; ++i) st[i] = (float)(r.w[i] >> 28);
    }
    DRIL_ENV_FN static void observe(const float* st, int agent, float* obs) {
        const int own = (int)st[agent];
        obs[0] = table(own);
        obs[1] = table((own + cells / 4) % cells);
#pragma unroll
        for (int k = 1; k < N; ++k) {
            const int other = (int)st[(agent + k) % N];
            obs[1 + k] = (float)offset(own, other) * 0.125f;
        }
    }
    DRIL_ENV_FN static void step(float* st, const float* act_f, const int* act_i, float* rew, bool* terminated) {
        int cell[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int move = act_i[i] == 0 ? -1 : act_i[i] == 2 ? 1 : 0;
            cell[i] = ((int)st[i] + move + cells) % cells;
            st[i] = (float)cell[i];
        }
        bool together = true;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            int total = 0;
#pragma unroll
            for (int k = 1; k < N; ++k) {
                const int off = offset(cell[i], cell[(i + k) % N]);
                total += off < 0 ? -off : off;
            }
            rew[i] = -(float)total * 0.125f;
            together = together && cell[i] == cell[0];
        }
        *terminated = together;
    }
};
DRIL_ENV_PLUGIN_WORLD(RingMeet4)
