// cartpole_fused_plugin.hip — the CartPole-v1 plug-in of cartpole_plugin.hip with the fused rollout (include/device/dril_env_rollout.h): the same env, and a code object
// that also holds dril_env_plugin_rollout — one launch per PPO collection once dril_rollout_fused_enable has switched the handle to it.
//     hipcc --genco --offload-arch=gfx950 --no-gpu-bundle-output -O3 -fno-slp-vectorize -I include examples/envs/cartpole_fused_plugin.hip -o examples/envs/cartpole_fused_plugin.hsaco
#include "cartpole_plugin.hip"
#include "device/dril_env_rollout.h"
DRIL_ENV_PLUGIN_ROLLOUT(CartPolePlugin)
