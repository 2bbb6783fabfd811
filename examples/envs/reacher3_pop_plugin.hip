// reacher3_pop_plugin.hip — the reacher3 plug-in of reacher3_fused_plugin.hip with the population entry (include/device/dril_env_rollout_pop.h): the same env and rollout
// kernel, and a code object that also holds dril_env_plugin_rollout_pop — the collections of all members of a population in one launch (docs/population.md).
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/reacher3_pop_plugin.hip -o examples/envs/reacher3_pop_plugin.hsaco
#include "reacher3_fused_plugin.hip"
#include "device/dril_env_rollout_pop.h"
DRIL_ENV_PLUGIN_ROLLOUT_POP(Reacher3)
