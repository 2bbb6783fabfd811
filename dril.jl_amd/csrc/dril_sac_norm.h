// dril_sac_norm.h — what is the SAC handle's own of NormalizeWrapperEnv (src/environment_wrappers/normalizeWrapperEnv.jl) around its device envs, for any
// observation width the handle accepts (1 .. 1024): the table shape and the argument blocks of its kernels.  Everything it shares with the PPO handle's wrapper on
// device env plug-ins (dril_ppo_norm.h) — scalars, the moments kernel, the head of the apply kernel, the host state — is dril_norm_wrap.h.  The kernels stand with
// their launches: sac_norm_env_kernel in dril_sac_collect.hip, sac_norm_apply_kernel in dril_sac_wrap.hip, sac_eval_account_norm_kernel in dril_sac_eval.hip; the wrapper of an external
// handle (dril_sac_ext_norm.h) shares the table shape and the LDS layout.
//
// A collected step is two launches of the wrapper where the plain collection is one:
//   moments   built-in Box envs: sac_norm_env_kernel<KIND> = head -> act! -> raw observe of sac_collect_env_kernel (the same shared definitions), the `returns`
//             recursion, and the block's partial sums; plug-ins: the plug-in's own step kernel, then norm_moments_kernel<kNzTile> over the E x D array it wrote
//   apply     sac_norm_apply_kernel: every block folds the partial table in the same fixed order, merges it into the running statistics, normalises reward /
//             terminal observation (OLD observation statistics) / next observation (NEW ones), and pushes the step's row
// A collection's opening observe (off_policy_collection.jl:42) is one more moments + apply pair: at train_freq = 1 that is four launches of the wrapper per env step.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/device/dril_env_plugin.h"   // DRIL_ENV_PLUGIN_MAX_D
#include "dril_norm_wrap.h"     // NormWrapArgs, kNzMaxD
#include "dril_sac_device.h"    // CollectEnvArgs, PushArgs

namespace dril::sac {

static_assert(kNzMaxD == DRIL_ENV_PLUGIN_MAX_D, "the wrapper takes every observation width a plug-in may have");
// rows of the partial table of norm_moments_kernel<kNzTile>.  Every block of the apply kernel re-reads rows x (2 D + 2) doubles, so for wide rows this trades the moments
// kernel's parallelism (rows x column tiles workgroups) against that fold; 32 is a choice, not a measured optimum (docs/sac.md: 4 096 envs x 512 dims)
constexpr int kNzMaxRows = 32;
constexpr int kNzTile = 256;                    // columns per tile of the moments kernel when D > 64: with so few rows a thread per column, no reduction

// ---- moments, built-in Box envs (A = 1): sac_norm_env_kernel ----------------------------------------------------------------------------------------------
struct NormEnvArgs { CollectEnvArgs env; float* returns; int upd_ret; float gamma; double* partials; };

// ---- apply + push: sac_norm_apply_kernel --------------------------------------------------------------------------------------------------------------------
// rew == null: observe alone (the collection's first observe; a read-only peek with partials == null); push.E == 0: no ring write.
struct NzApplyArgs {
    NormWrapArgs w; float* old_rew; const float* tobs;
    PushArgs push;                                                                       // push.obs: the normalised observation the action was chosen on
};
static_assert(sizeof(double) * (256 + 2 * (size_t)kNzMaxD + 2) + sizeof(float) * (2 * (size_t)kNzMaxD + 2) <= 48 * 1024, "sac_norm_apply_kernel's dynamic LDS at the widest observation");
inline size_t nz_apply_lds(int D) { return sizeof(double) * (256 + 2 * (size_t)D + 2) + sizeof(float) * (2 * (size_t)D + 2); }

// ---- evaluation: the frozen statistics, no moments, no added launch per step ------------------------------------------------------------------------------
struct NzEvalArgs { const float* st; int norm_obs; float eps, clip; };                   // st == null: the wrapper is off

}  // namespace dril::sac
