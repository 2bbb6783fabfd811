// dril_env_rollout_pop.h — the fused rollout of a device env plug-in for a POPULATION: n members' collections in one launch.
//
// A plug-in author adds two more lines to a source that ends in DRIL_ENV_PLUGIN_ROLLOUT(MyEnv):
//
//     #include "device/dril_env_rollout_pop.h"
//     DRIL_ENV_PLUGIN_ROLLOUT_POP(MyEnv)
//
// and the code object gains dril_env_plugin_rollout_pop, dril_env_plugin_rollout_pop_scaled (exactly when dril_env_plugin_scalable<MyEnv>(), the rule of the other
// _scaled kernels) and the descriptor dril_env_plugin_rollout_pop_desc.  dril_population_join (include/dril_hip.h) takes handles of such a code object whose solo
// iteration is the fused rollout plus the one-launch update (docs/population.md, "Plug-in members").  The rollout body, DrilEnvRolloutArgs, DRIL_ENV_ROLLOUT_ABI and
// DRIL_ENV_PLUGIN_ABI do not change, and a source without this macro compiles to exactly the symbols it had.
//
// The kernel: grid (ceil(E / DRIL_ENV_ROLLOUT_TILE), n).  The workgroups of row y run DrilEnvRolloutBody<Env, scaled>::run, the body of the solo kernel,
// on members[y] — the argument block dril_env_plugin_rollout takes by value, read in place through the constant address space (pop_member_block): every field is a
// uniform load, as the solo kernel's loads of its kernel argument are, and every pointer of the block is a global pointer to the compiler, so the member's loop issues
// the global loads and stores of its solo twin, not flat ones.  The same device code on the solo launch's own arguments: a member's rows are the solo handle's, bit
// for bit.  Members share nothing; as in the solo kernel the only synchronisation is the workgroup barrier: no grid barrier, no atomics, no spin-waits, and
// workgroups beyond what is resident start when others have finished — no cap on n.
//   Why not a private copy of the block with pop_global on its pointers, as the library's own population kernels do: DrilEnvRolloutArgs holds hidden[], which the
//   body indexes at run time, and a private struct that is indexed at run time is not split into registers — the whole copy would live in scratch memory and its
//   pointers would come back from there as flat ones.
//
// With DRIL_ENV_PLUGIN_HOST the macro emits dril_env_plugin_host_rollout_pop (and _scaled): a serial loop over the members of the host rollout.
#pragma once
#include "dril_env_rollout.h"
#include "dril_pop_global.h"

#ifndef DRIL_ENV_ROLLOUT_POP_ABI
#define DRIL_ENV_ROLLOUT_POP_ABI 1u      // bumps whenever the entry points' signature or the meaning of the descriptor changes
#endif

// same fields as DrilEnvRolloutDesc: the ABI number is this header's, args_size the size of ONE member's block
typedef DrilEnvRolloutDesc DrilEnvRolloutPopDesc;
template <class Env> constexpr DrilEnvRolloutPopDesc dril_env_rollout_pop_make_desc() {
    DrilEnvRolloutPopDesc d = dril_env_rollout_make_desc<Env>();
    d.abi_version = DRIL_ENV_ROLLOUT_POP_ABI;
    return d;
}

#if defined(DRIL_ENV_PLUGIN_HOST)
#define DRIL_ENV_ROLLOUT_POP_ENTRY(name) __attribute__((visibility("default"))) void dril_env_plugin_host_##name(const DrilEnvRolloutArgs* members, int n)
template <class Env, bool scaled> inline void dril_env_rollout_pop_host(const DrilEnvRolloutArgs* members, int n) { for (int m = 0; m < n; ++m) DrilEnvRolloutBody<Env, scaled>::run(members[m]); }
#define DRIL_ENV_ROLLOUT_POP_RUN(Env, scaled) dril_env_rollout_pop_host<Env, scaled>(members, n)
typedef void (*DrilEnvRolloutPopEntry)(const DrilEnvRolloutArgs*, int);
#else
#define DRIL_ENV_ROLLOUT_POP_ENTRY(name) __global__ void __launch_bounds__(DRIL_ENV_ROLLOUT_THREADS) dril_env_plugin_##name(const DrilEnvRolloutArgs* __restrict__ members, int n)
#define DRIL_ENV_ROLLOUT_POP_RUN(Env, scaled) do { if ((int)blockIdx.y >= n) return; DrilEnvRolloutBody<Env, scaled>::run(dril::pop_member_block(members, blockIdx.y)); } while (0)
typedef void (*DrilEnvRolloutPopEntry)(const DrilEnvRolloutArgs*, int);
#endif

// the optional _scaled entry point: declared here, DEFINED as a friend of the specialisation that fits the env (the mechanism of DrilEnvRolloutScaledEntry)
extern "C" { DRIL_ENV_ROLLOUT_POP_ENTRY(rollout_pop_scaled); }
template <class Env, bool scalable> struct DrilEnvRolloutPopScaledEntry {};
template <class Env> struct DrilEnvRolloutPopScaledEntry<Env, true> {
    friend DRIL_ENV_ROLLOUT_POP_ENTRY(rollout_pop_scaled) { DRIL_ENV_ROLLOUT_POP_RUN(Env, true); }
#if defined(DRIL_ENV_PLUGIN_HOST)
    static constexpr DrilEnvRolloutPopEntry rollout_pop_scaled = &dril_env_plugin_host_rollout_pop_scaled;
#else
    static constexpr DrilEnvRolloutPopEntry rollout_pop_scaled = &dril_env_plugin_rollout_pop_scaled;
#endif
};

#define DRIL_ENV_PLUGIN_ROLLOUT_POP(Env)                                                                                 \
    static_assert(DrilEnvRolloutCheck<Env>::ok, "");                                                                     \
    extern "C" {                                                                                                         \
    DRIL_ENV_ROLLOUT_DESC_QUAL extern const DrilEnvRolloutPopDesc dril_env_plugin_rollout_pop_desc = dril_env_rollout_pop_make_desc<Env>(); \
    DRIL_ENV_ROLLOUT_POP_ENTRY(rollout_pop) { DRIL_ENV_ROLLOUT_POP_RUN(Env, false); }                                    \
    }                                                                                                                    \
    template struct DrilEnvRolloutPopScaledEntry<Env, dril_env_plugin_scalable<Env>()>;
