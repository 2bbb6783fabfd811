#!/usr/bin/env python3
"""SAC on the caller's OWN env, living on the device: examples/envs/reacher3_plugin.hip (a point mass in 3-D pushed towards a per-episode random target; 12
observation dims, a three-dimensional force Box) is compiled by the library's Makefile into a gfx950 code object; the library loads it
(dril_sac_create_with_env_module) and steps it with its own kernels between the actor's forward and the replay ring.  No host env anywhere in the loop:
off-policy collection, the ring and every gradient step stay on the device.  The PPO twin of this file is examples/ppo_device_plugin.py.

usage: python examples/sac_device_plugin.py [n_envs=16] [max_steps=30000]"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g

pkg = g.load_package()
n_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 16
max_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30000
code_object = ROOT / "examples" / "envs" / "reacher3_plugin.hsaco"        # built by `make -C dril.jl_amd/csrc` (__graft_entry__.build())
info = pkg.describe_env_module(code_object)
print("env:", info)
env = pkg.DeviceModuleEnv(code_object, n_envs, seed=0)
alg = pkg.SAC(learning_rate=1e-3, buffer_capacity=100_000, start_steps=100 * n_envs, batch_size=256, gradient_steps=8)
agent = pkg.SACAgent(pkg.SACLayer(env.observation_space(), env.action_space(), hidden_dims=(64, 64)), alg, seed=0)
T = info["episode_len"]


def episode_return(handle, seed=123):
    """mean return of one episode per env under the current policy: reset, one time limit of policy steps, the rewards of the newest rows of the ring"""
    handle.env_reset(seed)
    handle.collect_rollout(T, False)
    return float(handle.replay(pkg._capi.RB_REWARDS)[-T * n_envs:].reshape(T, n_envs).sum(0).mean())


rb = pkg.ReplayBuffer(env.observation_space(), env.action_space(), alg.buffer_capacity)
rb.handle = pkg.SacHandle(pkg.make_sac_config(env, n_envs, alg, agent.layer, seed=0), env_module=code_object)
rb.handle.set_params(pkg.sac_flatten_params(agent.parameters))
before = episode_return(rb.handle)
agent, rb, stats, timer = pkg.sac_train_(agent, env, alg, max_steps, replay_buffer=rb)
after = episode_return(rb.handle)
print(f"trained {agent.steps_taken} env steps, {agent.gradient_updates} gradient steps in {timer['training_loop']:.2f} s; "
      f"critic loss {stats['critic_losses'][-1]:.4f}, entropy coefficient {stats['entropy_coefficients'][-1]:.4f}")
print(f"episode return: {before:.1f} before -> {after:.1f} after")
