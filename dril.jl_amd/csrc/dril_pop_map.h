// dril_pop_map.h — where the members of one launch of ppo_update_small_pop_kernel sit in its 1-D grid.  Plain C++ (host and device; tests/test_population.py compiles it
// with g++).  Workgroup ids are dealt round-robin over the eight XCDs, so two ids that are equal mod 8 share an XCD and with it an L2: member m of a launch takes the
// actor block 16 (m / 8) + m % 8 and the critic block eight further — for m = 0 the ids 0 and 8 of ppo_update_small_kernel.  A group of 16 ids holds eight members, one per
// XCD; the grid is 16 ceil(n / 8) and a block without a member leaves at once.  Placement is for speed only: the messages are agent-scope accesses wherever the pair sits.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRIL_POP_HD __host__ __device__
#else
#define DRIL_POP_HD
#endif

namespace dril {

constexpr int kPopXcds = 8;
DRIL_POP_HD constexpr int pop_actor_block(int m) { return 2 * kPopXcds * (m / kPopXcds) + m % kPopXcds; }
DRIL_POP_HD constexpr int pop_critic_block(int m) { return pop_actor_block(m) + kPopXcds; }
DRIL_POP_HD constexpr int pop_grid(int n) { return 2 * kPopXcds * ((n + kPopXcds - 1) / kPopXcds); }
// the inverse: the member of block b and its role (0 actor, 1 critic); member >= n: the block has none
DRIL_POP_HD constexpr int pop_block_member(int b) { return kPopXcds * (b / (2 * kPopXcds)) + b % kPopXcds; }
DRIL_POP_HD constexpr int pop_block_role(int b) { return (b / kPopXcds) & 1; }

}  // namespace dril

// pop_global (device code): the global-address-space round trip of a pointer read out of a member's argument block, shared with the plug-ins' population kernels
#if defined(__HIPCC__)
#include "../../include/device/dril_pop_global.h"
#endif
