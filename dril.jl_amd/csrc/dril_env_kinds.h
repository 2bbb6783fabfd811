// dril_env_kinds.h — the built-in envs on the host side: the ONE list of the kinds that have a simulator in this library, what the host needs to know of each
// (derived from EnvSpec<KIND> / act_bound<KIND>(), the kernels' truth in dril_device.h), which kinds may share a kernel instantiation, and the one dispatcher
// from a run-time env_kind to a compile-time KIND.  DRIL_ENV_EXTERNAL (host envs) and DRIL_ENV_MODULE (device env plug-ins, dril_env_side.h) are not in the list:
// they have no EnvSpec, no simulator and no per-kind kernel.
// No launcher, no create function and no verb names a kind: what is particular to one (its time limit, which kinds share a kernel, the boxes of the scaled ones) is
// stated here; adding one: DESIGN.md §5, "Env kinds on the host".
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "dril_device.h"

namespace dril {

template <int... K> struct KindList {};
using BuiltinKinds = KindList<0, 1, 2, 3, 4, 6, 7>;   // DRIL_ENV_* (include/dril_hip.h): CartPole, Pendulum, scaled Pendulum, MountainCar, MountainCarContinuous, Acrobot, scaled MountainCarContinuous
using BoxKinds = KindList<1, 2, 4, 7>;                // the built-ins with a Box action space: what SAC takes, and what its fused env kernels are built for
// Gymnasium's TimeLimit of each kind: the default episode_len of dril_config_default / dril_sac_config_default
constexpr int kind_time_limit(int kind) { return (kind == 0 || kind == 6) ? 500 : (kind == 4 || kind == 7) ? 999 : 200; }

// what the host needs of a built-in kind; box: a Box action space of A dims inside [act_lo, act_hi] (the bounds mean nothing for a Discrete kind)
struct EnvKindInfo { int D, A, S; bool discrete; int default_episode_len; float act_lo, act_hi; bool box; };
template <int K> constexpr EnvKindInfo make_kind_info() {
    return EnvKindInfo{EnvSpec<K>::D, EnvSpec<K>::A, EnvSpec<K>::S, EnvSpec<K>::discrete, kind_time_limit(K), -act_bound<K>(), act_bound<K>(), !EnvSpec<K>::discrete};
}
template <int... K> const EnvKindInfo* find_kind_info(int kind, KindList<K...>) {
    static constexpr int kinds[] = {K...};
    static constexpr EnvKindInfo table[] = {make_kind_info<K>()...};
    for (size_t i = 0; i < sizeof...(K); ++i) if (kinds[i] == kind) return &table[i];
    return nullptr;
}
// null: a kind with no built-in simulator (DRIL_ENV_EXTERNAL, DRIL_ENV_MODULE, any number out of range)
inline const EnvKindInfo* env_kind_info(int kind) { return find_kind_info(kind, BuiltinKinds{}); }
// The built-ins that are a ScalingWrapperEnv (kinds 2 and 7) and the boxes of the env they wrap — its observation space (D entries) and its action space (A = 1) — as
// the trajectory recordings need them to undo the maps.  The host's copy of the literals in env_obs<2 / 7> and env_step<2 / 7> (dril_device.h): the two change together
struct ScaledKindBoxes { int kind, D; float obs_low[3], obs_high[3], act_low, act_high; };
inline const ScaledKindBoxes* scaled_kind_boxes(int kind) {   // null: not a ScalingWrapperEnv
    static constexpr ScaledKindBoxes table[] = {{2, EnvSpec<2>::D, {-1.0f, -1.0f, -8.0f}, {1.0f, 1.0f, 8.0f}, -2.0f, 2.0f},
                                                {7, EnvSpec<7>::D, {-1.2f, -0.07f}, {0.6f, 0.07f}, -1.0f, 1.0f}};
    static_assert(EnvSpec<2>::D == 3 && EnvSpec<7>::D == 2 && EnvSpec<2>::A == 1 && EnvSpec<7>::A == 1, "the boxes above are written for these shapes");
    for (const ScaledKindBoxes& b : table) if (b.kind == kind) return &b;
    return nullptr;
}

// Which kinds may run the same instantiation of a kernel depends on what the kernel touches of the simulator.  canonical(kind) is the kind whose instantiation runs:
//
//   rule     what the kernel touches                      sharing        used by
//   Shape    nothing of the simulator (net shapes only)   2->1, 7->4     forward, gradient kernels, pack_records, ppo_update_small
//   Reset    the initial-state distribution only          2->1; 4,7->3   env_reset_kernel
//   Observe  the observation map only                     4->3           env_observe_kernel, obs_partials_kernel
//   None     the transition                               none           env_step_kernel, norm_step_kernel, the rollout kernels, the SAC env kernels
//
// (2 and 7 are ScalingWrapperEnv around 1 and 4: the same simulator and net shapes, affine maps on observations and actions; 3, 4 and 7 draw MountainCar's one initial
// state, and 3 and 4 observe the state as it is.)
namespace KindShare {
struct Shape { static constexpr int canonical(int k) { return k == 2 ? 1 : k == 7 ? 4 : k; } };
struct Reset { static constexpr int canonical(int k) { return k == 2 ? 1 : (k == 4 || k == 7) ? 3 : k; } };
struct Observe { static constexpr int canonical(int k) { return k == 4 ? 3 : k; } };
struct None { static constexpr int canonical(int k) { return k; } };
}  // namespace KindShare

template <class Share, int K, class F> void run_if_canonical(int canonical, F& f, hipError_t& r) {
    if constexpr (Share::canonical(K) == K) { if (canonical == K) r = f(std::integral_constant<int, K>{}); }   // f is instantiated for the canonical kinds only
}
// r = f(std::integral_constant<int, KIND>{}) with KIND = Share::canonical(kind) for a kind of the list; hipErrorInvalidValue, and nothing launched, for any other
// number.  The list is what the kernel is built for: every built-in kind, or BoxKinds for the SAC env kernels.
template <class Share, class F, int... K> hipError_t with_env_kind(KindList<K...>, int kind, F&& f) {
    hipError_t r = hipErrorInvalidValue;
    if (((kind == K) || ...)) (run_if_canonical<Share, K>(Share::canonical(kind), f, r), ...);
    return r;
}
template <class Share, class F> hipError_t with_env_kind(int kind, F&& f) { return with_env_kind<Share>(BuiltinKinds{}, kind, std::forward<F>(f)); }

}  // namespace dril
