// cartpole_eval_plugin.hip — the cartpole plug-in of cartpole_fused_plugin.hip with the fused evaluation (include/device/dril_env_evaluate.h): the same env and rollout kernel, and a
// code object that also holds dril_env_plugin_evaluate — K env steps of dril_evaluate_agent_device / dril_collect_trajectory_device per launch where the caller asks
// for the persistent form (docs/evaluation.md, path 2).
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/cartpole_eval_plugin.hip -o examples/envs/cartpole_eval_plugin.hsaco
#include "cartpole_fused_plugin.hip"
#include "device/dril_env_evaluate.h"
DRIL_ENV_PLUGIN_EVALUATE(CartPolePlugin)
