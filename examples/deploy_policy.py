#!/usr/bin/env python3
"""From a training run to a deployed policy: train PPO on the reacher3 device env plug-in under NormalizeWrapperEnv, extract_policy(agent, env) — actor, action
adapter and the frozen observation statistics, nothing else —, save_policy, destroy everything the training run owned, load_policy as a machine that never saw the
run would, and drive one episode from a host-side loop with single RAW observations: one kernel launch per action (docs/deployment.md).

usage: python examples/deploy_policy.py [n_envs=64] [iterations=3]"""
import sys
import tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
n_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 64
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 3
code_object = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"        # built by `make -C dril.jl_amd/csrc` (__graft_entry__.build())

# ---- the training run ----
env = pkg.DeviceModuleEnv(code_object, n_envs, seed=0, normalize=dict(clip_obs=5.0))
alg = pkg.PPO(n_steps=50, batch_size=n_envs * 50 // 4, epochs=4, learning_rate=1e-3)
agent = pkg.Agent(pkg.ActorCriticLayer(env.observation_space(), env.action_space(), hidden_dims=(48, 48)), alg, seed=0)
pkg.train_(agent, env, alg, iters * alg.n_steps * n_envs)
policy = pkg.extract_policy(agent, env)                                     # NormWrapperPolicy: obs_rms, epsilon, clip_obs read from the wrapper
print(f"extracted: {type(policy).__name__}, obs {policy.D}, actions {policy.A}, hidden {policy.hidden_dims}, clip_obs {policy.clip_obs}")
path = pkg.save_policy(policy, Path(tempfile.mkdtemp()) / "reacher3_policy")
policy.close(); env.handle.close(); del policy, agent, env                   # nothing of the training run is left

# ---- deployment ----
policy = pkg.load_policy(path)
print(f"loaded {path}: {type(policy).__name__} over {policy.action_space}")
world = pkg.Handle(pkg.make_config(pkg.host.ModuleEnv(str(code_object), pkg.describe_env_module(code_object), 100), 1, pkg.PPO(n_steps=1, batch_size=1)),
                   env_module=code_object)                                  # one env to act in (its own handle: the world, not the agent)
world.env_reset(123)
ret, steps, done = 0.0, 0, False
while not done:
    obs = world.env_observe()[0]                                            # one RAW observation ...
    action = policy(obs)                                                    # ... in, one env action out
    rew, term, trunc, _ = world.env_step(action.reshape(1, -1))
    ret += float(rew[0]); steps += 1; done = bool(term[0] or trunc[0])
print(f"episode return {ret:.3f} over {steps} steps")
